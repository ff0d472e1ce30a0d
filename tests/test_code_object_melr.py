"""clx_k_mel_fr and clx_k_mel_qr in the gfx950 code object (read on the CPU).  The reflected forms of the feature kernel keep what their
siblings keep -- accumulators, operands and prefetch in vector registers: no scratch, no spill of either kind, no accumulation
registers, wave64 code for workgroups of 256 -- and no more LDS than the staging area: the index map costs a few registers (the
window's valid samples, two 64-bit first taps in place of two pointers) and no memory.  Three waves per SIMD, as for the other five:
512 / 3 registers, rounded down to the allocation granule of 8."""
import pytest

from test_code_object import kernel_notes

LDS_BYTES = 35072                # DESIGN.md 4.10 / 4.16; clx_mel::kLdsBytes
VGPRS = 168                      # 512 // 3 // 8 * 8


@pytest.mark.parametrize("name", ("clx_k_mel_fr", "clx_k_mel_qr"))
def test_the_reflected_kernels_stay_in_registers_and_within_the_lds(name):
    k = kernel_notes()[name]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert 0 < k["group_segment_fixed_size"] <= LDS_BYTES, k
    assert k["vgpr_count"] <= VGPRS == 512 // 3 // 8 * 8, k


def test_the_stated_lds_is_the_sources():
    import simlib_melr as sr
    assert sr.lib().sim_melr_lds_bytes() == LDS_BYTES
