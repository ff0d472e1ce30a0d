"""The segmented indexer's kernels (clx_index.hip) in the gfx950 code object, read on the CPU: wave64 code, no private segment, no
spill of any kind (scalar spills into vector lanes are the fault ADVICE.md traces), no dynamic stack."""
import pytest

from test_code_object import kernel_notes

KERNELS = ("clx_k_idx_scan", "clx_k_idx_offsets", "clx_k_idx_compact", "clx_k_idx_span_crc")


@pytest.fixture(scope="module")
def notes():
    return kernel_notes()


@pytest.mark.parametrize("name", KERNELS)
def test_index_kernel_stays_in_registers(notes, name):
    k = notes[name]
    assert k["wavefront_size"] == 64, k
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k.get("uses_dynamic_stack", 0) == 0, k
