"""clx_k_mel_q in the gfx950 code object (read on the CPU).  The cepstral form of the feature kernel keeps what the other three keep --
accumulators, operands and prefetch in vector registers: no scratch, no spill of either kind, no accumulation registers, wave64
code for workgroups of 256 -- and no more LDS than the staging area: a lane's 16 finished log-mel cells wait in the registers the
GEMM's accumulators have left, and Y and the 32 log energies take the staging area's place once P has been read.  Three waves per
SIMD, as for the other three: 512 / 3 registers, rounded down to the allocation granule of 8."""
from test_code_object import kernel_notes

LDS_BYTES = 35072                # DESIGN.md 4.10 / 4.13; clx_mel::kLdsBytes
VGPRS = 168                      # 512 // 3 // 8 * 8


def test_the_cepstral_kernel_stays_in_registers_and_within_the_lds():
    k = kernel_notes()["clx_k_mel_q"]
    print("clx_k_mel_q: %d VGPRs, %d bytes of LDS" % (k["vgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert 0 < k["group_segment_fixed_size"] <= LDS_BYTES, k
    assert k["vgpr_count"] <= VGPRS == 512 // 3 // 8 * 8, k


def test_the_stated_lds_is_the_sources():
    import simlib_melq as sq
    assert sq.lib().sim_melq_lds_bytes() == LDS_BYTES
