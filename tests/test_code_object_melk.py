"""clx_k_mel_f in the gfx950 code object (read on the CPU).  The conditioning form of the feature kernel keeps what clx_k_mel keeps --
accumulators, operands and prefetch in vector registers: no scratch, no spill of either kind, no accumulation registers, wave64
code for workgroups of 256 -- and no more LDS than the staging area: the prologue adds none (the 32 frame means cross the block
through the staging area's first words before the staging begins, and then live in registers)."""
from test_code_object import kernel_notes

LDS_BYTES = 35072                # DESIGN.md 4.10 / 4.12; clx_mel::kLdsBytes
PROLOGUE_LDS_BYTES = 0


def test_the_conditioning_kernel_stays_in_registers_and_within_the_lds():
    k = kernel_notes()["clx_k_mel_f"]
    print("clx_k_mel_f: %d VGPRs, %d bytes of LDS" % (k["vgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert 0 < k["group_segment_fixed_size"] <= LDS_BYTES + PROLOGUE_LDS_BYTES, k
    assert k["vgpr_count"] <= 256, k


def test_the_stated_lds_is_the_sources():
    import simlib_melk as sk
    assert sk.lib().sim_melk_lds_bytes() == LDS_BYTES
