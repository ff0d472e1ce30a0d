"""The kernels of clx_cmvn_global_windows and clx_cmvn_sliding_windows in the gfx950 code object (read on the CPU), against what
clx_cmvn.hip's header and DESIGN.md 4.22 state: no scratch, no spill of either kind, no accumulation registers, wave64 code for
workgroups of 256; clx_k_cmvn_sliding with 48 608 bytes of LDS (8 staged rows of 1351 words, the groups' double sums and sums of
squares): three workgroups a CU; clx_k_cmvn_global with none."""
import pytest

from test_code_object import kernel_notes

SLIDING_LDS_BYTES, GLOBAL_LDS_BYTES = 48608, 0


@pytest.mark.parametrize("name,lds", (("clx_k_cmvn_global", GLOBAL_LDS_BYTES), ("clx_k_cmvn_sliding", SLIDING_LDS_BYTES)))
def test_the_kernels_stay_in_registers_and_within_their_lds(name, lds):
    k = kernel_notes()[name]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert k["group_segment_fixed_size"] == lds, k
    assert k["vgpr_count"] <= 128, k                          # (four waves a SIMD by registers: more than the LDS lets in)


def test_the_stated_lds_is_the_sources():
    import simlib_cmvn as sc
    assert sc.lib().sim_cmvn_sliding_lds_bytes() == SLIDING_LDS_BYTES == sc.SLIDING_LDS_BYTES
    assert sc.lib().sim_cmvn_global_lds_bytes() == GLOBAL_LDS_BYTES == sc.GLOBAL_LDS_BYTES
    assert sc.lib().sim_cmvn_threads() == 256 and sc.lib().sim_cmvn_tile() == 256
    assert sc.lib().sim_cmvn_row_chunk() == sc.RC and sc.lib().sim_cmvn_max_span() == sc.MAX_SPAN
    assert 3 * SLIDING_LDS_BYTES <= 160 * 1024 < 4 * SLIDING_LDS_BYTES      # three workgroups a CU by LDS (at least two are asked for)
