"""clx_k_mel_c and clx_k_mel_range in the gfx950 code object (read on the CPU).  The centred and ranged form of the feature kernel
keeps what clx_k_mel keeps -- accumulators, operands and prefetch in vector registers: no scratch, no spill of either kind, no
accumulation registers, wave64 code for workgroups of 256, and no more LDS than the staging area (35 072 bytes: the four words of
the maximum's reduction alias it).  The range step is pure streaming: no LDS, no scratch, no spills."""
from test_code_object import kernel_notes

LDS_BYTES = 35072                # DESIGN.md 4.10 / 4.11; clx_mel::kLdsBytes


def test_the_centred_kernel_stays_in_registers_and_within_the_lds():
    k = kernel_notes()["clx_k_mel_c"]
    print("clx_k_mel_c: %d VGPRs, %d bytes of LDS" % (k["vgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert 0 < k["group_segment_fixed_size"] <= LDS_BYTES, k
    assert k["vgpr_count"] <= 256, k


def test_the_range_step_is_pure_streaming():
    k = kernel_notes()["clx_k_mel_range"]
    print("clx_k_mel_range: %d VGPRs" % k["vgpr_count"])
    assert k["group_segment_fixed_size"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k


def test_the_stated_lds_is_the_sources():
    import simlib_melc as sc
    assert sc.lib().sim_melc_lds_bytes() == LDS_BYTES and sc.lib().sim_melc_range_vectors() == 1024
