"""The kernel of clx_splice_windows in the gfx950 code object (read on the CPU), against what clx_splice.hip's header and DESIGN.md
4.21 state: clx_k_splice in no more than 40 vector registers, no scratch, no spill of either kind, no accumulation registers, wave64
code for workgroups of 256, and 37 504 bytes of LDS (the staged span, the blocks and the coefficients): four workgroups a CU."""
from test_code_object import kernel_notes

LDS_BYTES, VGPRS = 37504, 40


def test_the_kernel_stays_in_registers_and_within_its_lds():
    k = kernel_notes()["clx_k_splice"]
    print("clx_k_splice: %d VGPRs, %d SGPRs, %d bytes of LDS" % (k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert k["group_segment_fixed_size"] == LDS_BYTES, k
    assert k["vgpr_count"] <= VGPRS, k
    assert 4 * LDS_BYTES <= 160 * 1024 < 5 * LDS_BYTES       # four workgroups a CU by LDS


def test_the_stated_lds_is_the_sources():
    import simlib_splice as sp
    assert sp.lib().sim_splice_lds_bytes() == LDS_BYTES == sp.LDS_BYTES
    assert sp.lib().sim_splice_threads() == 256
