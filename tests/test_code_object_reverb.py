"""The kernels of clx_reverb_windows in the gfx950 code object (read on the CPU), against what DESIGN.md 4.18 states: no scratch, no
spill of either kind, no accumulation registers, wave64 code for workgroups of 256; the FIR in at most 128 vector registers (four
waves a SIMD: eight accumulators, a sixteen-word window and eight taps, twice over for the guarded form) and exactly 10 240 bytes of
LDS (the source span of a tile and a chunk, and the chunk's taps), the gain and the scale steps in at most 64 and no LDS.  The power
sums are clx_add's kernels: there is no kernel of this call's beyond the three."""
import pytest

from test_code_object import kernel_notes

VGPRS = {"clx_k_reverb": 128, "clx_k_reverb_gain": 64, "clx_k_reverb_scale": 64}
LDS = {"clx_k_reverb": 10240, "clx_k_reverb_gain": 0, "clx_k_reverb_scale": 0}


@pytest.mark.parametrize("name", sorted(LDS))
def test_the_kernel_stays_in_registers_and_within_its_lds(name):
    k = kernel_notes()[name]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert k["group_segment_fixed_size"] == LDS[name], k
    assert k["vgpr_count"] <= VGPRS[name], k


def test_the_library_has_no_other_reverb_kernel():
    assert sorted(n for n in kernel_notes() if n.startswith("clx_k_reverb")) == sorted(LDS)
