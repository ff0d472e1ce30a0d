"""clx_k_window in the gfx950 code object (read on the CPU): the gather keeps its vectors in vector registers -- no scratch, no spill
of any kind (scalar spills into vector lanes are the fault ADVICE.md traces), no accumulation registers -- and transposes the
channels-first layout in registers: no LDS."""
from test_code_object import kernel_notes


def test_window_gather_stays_in_registers():
    k = kernel_notes()["clx_k_window"]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k["group_segment_fixed_size"] == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
