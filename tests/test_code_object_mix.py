"""clx_k_mix in the gfx950 code object (read on the CPU): like clx_k_resample it keeps its taps, the channels it averages and its
accumulator in vector registers -- no scratch, no spill of any kind, no accumulation registers, no dynamic stack -- is wave64 code
for workgroups of 256, and has no LDS at all: its loads are direct global loads."""
from test_code_object import kernel_notes


def test_mixer_stays_in_registers_and_off_lds():
    k = kernel_notes()["clx_k_mix"]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert k["group_segment_fixed_size"] == 0, k
