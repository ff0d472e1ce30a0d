"""The kernels of clx_cmvn_stats_windows and clx_cmvn_grouped_windows in the gfx950 code object (read on the CPU), against what
clx_cmvn_stats.hip's header and DESIGN.md 4.24 state: no scratch, no spill of either kind, no accumulation registers, wave64 code
for workgroups of 256; clx_k_cmvn_stats_sum_tc with 4 352 bytes of LDS (clx_norm's tile of 64 frames x 16 rows, rows 17 floats
apart), the CT sum, the fold, the solve and the apply with none."""
import pytest

from test_code_object import kernel_notes

LDS = {"clx_k_cmvn_stats_sum": 0, "clx_k_cmvn_stats_sum_tc": 4352, "clx_k_cmvn_stats_fold": 0, "clx_k_cmvn_stats_solve": 0, "clx_k_cmvn_grouped": 0}


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
    import simlib_cmvn_stats as ss
    L = ss.lib()
    assert L.sim_cmvn_stats_sum_lds_bytes() == LDS["clx_k_cmvn_stats_sum"] == ss.SUM_LDS_BYTES
    assert L.sim_cmvn_stats_sum_tc_lds_bytes() == LDS["clx_k_cmvn_stats_sum_tc"] == ss.SUM_TC_LDS_BYTES
    assert L.sim_cmvn_stats_fold_lds_bytes() == LDS["clx_k_cmvn_stats_fold"] == ss.FOLD_LDS_BYTES
    assert L.sim_cmvn_stats_solve_lds_bytes() == LDS["clx_k_cmvn_stats_solve"] == ss.SOLVE_LDS_BYTES
    assert L.sim_cmvn_stats_apply_lds_bytes() == LDS["clx_k_cmvn_grouped"] == ss.APPLY_LDS_BYTES
    assert L.sim_cmvn_stats_threads() == 256
