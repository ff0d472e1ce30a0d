"""The kernels of clx_addn_windows in the gfx950 code object (read on the CPU), against what DESIGN.md 4.25 states: every one of
them within a few vector registers of what the build gives (21 / 36 / 26 / 36; the bounds are 24 / 40 / 32 / 40, all far inside the
64 that still give eight waves a SIMD: the passes stream and live on the loads in flight), no scratch, no spill
of either kind, no accumulation registers, wave64 code for workgroups of 256, and no LDS at all: the sums fold through shuffles,
the gain step is one lane per term, and the apply pass reads the window's term records through the scalar path."""
import pytest

from test_code_object import kernel_notes

VGPRS = {"clx_k_addn_sum": 24, "clx_k_addn_sum_tc": 40, "clx_k_addn_gain": 32, "clx_k_addn_apply": 40}
LDS = {"clx_k_addn_sum": 0, "clx_k_addn_sum_tc": 0, "clx_k_addn_gain": 0, "clx_k_addn_apply": 0}


@pytest.mark.parametrize("name", sorted(LDS))
def test_the_kernel_stays_in_registers_and_within_its_lds(name):
    k = kernel_notes()[name]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"]))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0 and k.get("uses_dynamic_stack", 0) == 0, k
    assert k["wavefront_size"] == 64 and k["max_flat_workgroup_size"] == 256, k
    assert k["group_segment_fixed_size"] == LDS[name], k
    assert k["vgpr_count"] <= VGPRS[name], k


def test_the_library_has_no_other_addn_kernel():
    assert sorted(n for n in kernel_notes() if n.startswith("clx_k_addn_")) == sorted(LDS)
