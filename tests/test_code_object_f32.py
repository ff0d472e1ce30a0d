"""The float builds of the tiers in the gfx950 code object (read on the CPU): no vector register spilled, the register files and LDS of
their integer twins' occupancy, and no more scalar spills than the twins (the row scale is worked out per store call, not kept live)."""
import pytest

from test_code_object import kernel_notes


@pytest.fixture(scope="module")
def notes():
    return kernel_notes()


def test_lean_f32_stays_off_scratch(notes):
    k = notes["clx_k_lean_f32"]
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 168 and k["agpr_count"] == 0, k
    assert k["group_segment_fixed_size"] == 15360, k
    assert k["sgpr_spill_count"] <= notes["clx_k_lean"]["sgpr_spill_count"], (k, notes["clx_k_lean"])


def test_lean24_f32_stays_off_scratch(notes):
    k = notes["clx_k_lean24_f32"]
    assert k["vgpr_spill_count"] == 0 and k["vgpr_count"] <= 256, k
    assert k["group_segment_fixed_size"] == 15360, k
    assert k["sgpr_spill_count"] <= notes["clx_k_lean24"]["sgpr_spill_count"], (k, notes["clx_k_lean24"])
