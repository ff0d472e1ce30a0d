"""clx_k_resample in the gfx950 code object (read on the CPU): the resampler keeps its taps and its accumulator in vector registers --
no scratch, no spill of any kind (scalar spills into vector lanes are the fault ADVICE.md traces), no accumulation registers -- is
wave64 code, and whatever LDS it has leaves room for two workgroups on a CU."""
from test_code_object import kernel_notes


def test_resampler_stays_in_registers():
    k = kernel_notes()["clx_k_resample"]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert k["group_segment_fixed_size"] <= 65536, k
