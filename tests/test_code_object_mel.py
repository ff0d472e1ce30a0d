"""clx_k_mel in the gfx950 code object (read on the CPU): its 64 accumulators, its operands and the next slice's prefetch stay in
vector registers -- no scratch, no spill of any kind, no accumulation registers, no dynamic stack -- it is wave64 code for workgroups
of 256, and its LDS is the staging area DESIGN.md 4.10 states (35 072 bytes: at least two workgroups share a CU's 160 KiB)."""
from test_code_object import kernel_notes

LDS_BYTES = 35072                # DESIGN.md 4.10; clx_mel::kLdsBytes


def test_mel_stays_in_registers_and_within_its_lds():
    k = kernel_notes()["clx_k_mel"]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert 0 < k["group_segment_fixed_size"] <= LDS_BYTES and 2 * k["group_segment_fixed_size"] <= 160 * 1024, k
    assert k["vgpr_count"] <= 256, k                         # (two waves per SIMD by registers: the two workgroups' eight waves)


def test_the_stated_lds_is_the_sources():
    import simlib_mel as sm
    assert sm.lib().sim_mel_lds_bytes() == LDS_BYTES and sm.lib().sim_mel_group_frames() == 32
