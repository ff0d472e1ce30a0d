"""The kernels of clx_norm_windows in the gfx950 code object (read on the CPU), against what DESIGN.md 4.15 states: every one of
them in at most 64 vector registers (eight waves a SIMD), no scratch, no spill of either kind, no accumulation registers, wave64
code for workgroups of 256; no LDS in the CT sum kernels, 4 352 bytes (the 64 x 17 tile) in the TC ones, 2 048 bytes (mean and
scale of up to 256 rows) in the apply pass."""
import pytest

from test_code_object import kernel_notes

TC_LDS, APPLY_LDS, VGPRS = 4352, 2048, 64
LDS = {"clx_k_norm_sum": 0, "clx_k_norm_sq": 0, "clx_k_norm_sum_tc": TC_LDS, "clx_k_norm_sq_tc": TC_LDS, "clx_k_norm_apply": APPLY_LDS}


@pytest.mark.parametrize("name", sorted(LDS))
def test_the_kernel_stays_in_registers_and_within_its_lds(name):
    k = kernel_notes()[name]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert k["group_segment_fixed_size"] == LDS[name], k
    assert k["vgpr_count"] <= VGPRS, k


def test_the_stated_lds_is_the_sources():
    import simlib_norm as sn
    assert sn.lib().sim_norm_tc_lds_bytes() == TC_LDS and sn.lib().sim_norm_apply_lds_bytes() == APPLY_LDS
