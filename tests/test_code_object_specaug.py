"""The kernels of clx_specaug_windows in the gfx950 code object (read on the CPU), against what DESIGN.md 4.20 states: clx_k_specaug
and clx_k_specaug_fill in at most 64 vector registers (eight waves a SIMD), no scratch, no spill of either kind, no accumulation
registers, wave64 code for workgroups of 256; 9 248 bytes of LDS in clx_k_specaug (the per-frame sources, weights and flags of a
256-frame tile and the 256-bit row mask), none in the fill step; and clx_norm's sum kernels, which the mean reuses, keep the figures
test_code_object_norm.py pins."""
import pytest

from test_code_object import kernel_notes

LDS_BYTES, VGPRS = 9248, 64
LDS = {"clx_k_specaug": LDS_BYTES, "clx_k_specaug_fill": 0, "clx_k_norm_sum": 0, "clx_k_norm_sum_tc": 4352}


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
    import simlib_specaug as ss
    assert ss.lib().sim_specaug_lds_bytes() == LDS_BYTES == ss.LDS_BYTES
    assert ss.lib().sim_specaug_threads() == 256
