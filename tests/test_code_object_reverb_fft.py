"""The kernels of clx_reverb_windows_fft in the gfx950 code object (read on the CPU), against what DESIGN.md 4.19 states: no scratch,
no spill of either kind, no accumulation registers, wave64 code for workgroups of 256; at most 64 vector registers (eight waves a
SIMD) and exactly 16 384 bytes of LDS (the N complex words of one transform): eight workgroups of four waves -- one wave a SIMD each
-- share a CU's 160 KiB.  The power sums, the gain and the scale are clx_add's and clx_reverb's kernels: there is no kernel of this
call's beyond the two."""
import pytest

from test_code_object import kernel_notes

VGPRS = {"clx_k_rvfft_fwd": 64, "clx_k_rvfft_mac": 64}
LDS = {"clx_k_rvfft_fwd": 16384, "clx_k_rvfft_mac": 16384}


@pytest.mark.parametrize("name", sorted(LDS))
def test_the_kernel_stays_in_registers_and_within_its_lds(name):
    k = kernel_notes()[name]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert k["group_segment_fixed_size"] == LDS[name], k
    assert k["vgpr_count"] <= VGPRS[name], k
    assert 8 * k["group_segment_fixed_size"] <= 160 * 1024


def test_the_library_has_no_other_fft_kernel():
    assert sorted(n for n in kernel_notes() if n.startswith("clx_k_rvfft")) == sorted(LDS)
