"""The kernels of clx_vad_windows and clx_select_windows in the gfx950 code object (read on the CPU), against what clx_vad.hip's
header and DESIGN.md 4.23 state: no scratch, no spill of either kind, no accumulation registers, wave64 code for workgroups of
256; clx_k_vad_decide with 2 080 bytes of LDS (the prefix counts of a span of 512 frames and its eight segment totals),
clx_k_select_move with 1 040 (a tile's list of selected frames and the four waves' counts), clx_k_select_rank with 16, the sum and
the scan with none."""
import pytest

from test_code_object import kernel_notes

LDS = {"clx_k_vad_sum": 0, "clx_k_vad_decide": 2080, "clx_k_select_rank": 16, "clx_k_select_scan": 0, "clx_k_select_move": 1040}


@pytest.mark.parametrize("name", sorted(LDS))
def test_the_kernels_stay_in_registers_and_within_their_lds(name):
    k = kernel_notes()[name]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert k["group_segment_fixed_size"] == LDS[name], k
    assert k["vgpr_count"] <= 64, k                           # (eight waves a SIMD by registers)


def test_the_stated_lds_is_the_sources():
    import simlib_vad as sv
    L = sv.lib()
    assert L.sim_vad_sum_lds_bytes() == LDS["clx_k_vad_sum"] == sv.SUM_LDS_BYTES
    assert L.sim_vad_decide_lds_bytes() == LDS["clx_k_vad_decide"] == sv.DECIDE_LDS_BYTES
    assert L.sim_vad_rank_lds_bytes() == LDS["clx_k_select_rank"] == sv.RANK_LDS_BYTES
    assert L.sim_vad_scan_lds_bytes() == LDS["clx_k_select_scan"] == sv.SCAN_LDS_BYTES
    assert L.sim_vad_move_lds_bytes() == LDS["clx_k_select_move"] == sv.MOVE_LDS_BYTES
    assert L.sim_vad_threads() == 256 and L.sim_vad_tile() == sv.TILE == 256
    assert L.sim_vad_span() == sv.SPAN == sv.TILE + 2 * sv.MAX_CONTEXT and L.sim_vad_max_context() == sv.MAX_CONTEXT
    assert max(LDS.values()) <= 50 * 1024
