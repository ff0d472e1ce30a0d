"""The window gather (clx_window.hip: clx_window_check and clx_k_window) under the wave simulator, against numpy slicing of the same
source, bit for bit (as uint32): window lengths round the vector, wave and tile sizes, 1..8 channels, both layouts, every alignment
of a window's start, valid counts 0 / 1 / L-1 / L, more windows than a workgroup has lanes, overlapping and descending windows, an
output the test fills with NaN patterns (every element is overwritten, the words round the output are not), loads that stay inside
[src_first, src_first + valid * C) next to an inaccessible page, and the refused arguments."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_window as sw
import window_cases as wc

NAN_FILL = wc.NAN_FILL
GUARD = 0xffc0beef               # the words round the output
LAYOUTS = (sw.TC, sw.CT)
assert LAYOUTS == wc.LAYOUTS
_aligned = lambda n_words: wc.aligned(n_words)[1]
_expect = wc.expect


def run_sim(src, src_first, valid, L, C, layout, out_offset_words=0):
    """The runner of window_cases' checks: the call on an output pre-filled with NaN patterns inside an array of guard words."""
    n = len(src_first) * L * C
    raw, buf = wc.aligned(n, out_offset_words, fill=GUARD)
    assert buf.ctypes.data % 16 == 4 * out_offset_words
    buf[:] = NAN_FILL
    sw.gather_windows(src, src_first, valid, L, C, layout, buf)
    at = (buf.ctypes.data - raw.ctypes.data) // 4 if n else 0
    return buf.copy(), bool(np.all(raw[:at] == GUARD) and np.all(raw[at + n:] == GUARD))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", wc.CHANNELS)
def test_lengths_alignments_and_valid_counts(C, layout):
    """Every L, with one call of 32 windows each: src_first mod 8 over 0..7 times valid in {0, 1, L-1, L}."""
    assert wc.check_lengths_alignments_and_valid_counts(run_sim, C, layout) == (11, 32 * C * sum(wc.LENGTHS))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_output_on_a_4_byte_boundary_only(layout):
    """An output 1..3 words off the 16-byte grid: the first window has a ragged head too."""
    assert wc.check_output_on_a_4_byte_boundary_only(run_sim, layout)[0] == 15


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", wc.BATCHES)
def test_batch_sizes(B, layout):
    """No window, one, and 70 (more than one workgroup has lanes... and than a wave) with mixed valid counts in one call."""
    assert wc.check_batch_sizes(run_sim, B, layout) == (3, B * (257 * 2 + 256 * 3 + 1000 * 2))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_window_of_several_tiles(layout):
    """Windows longer than one tile of 4096 floats / samples: the tiles of a window meet without a gap, the last one is partial."""
    assert wc.check_a_window_of_several_tiles(run_sim, layout)[0] == 4


@pytest.mark.parametrize("layout", LAYOUTS)
def test_overlapping_and_descending_windows(layout):
    assert wc.check_overlapping_and_descending_windows(run_sim, layout) == (1, 10 * 65 * 2)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", (1, 2, 3, 8))
def test_loads_stay_inside_the_valid_region(C, layout):
    """The valid region ends on the last float before an inaccessible page, for every tail 1..9 samples past a whole number of
    vectors, waves and none at all; and it begins on the first float behind an inaccessible page.  A stray load would fault."""
    rng = np.random.default_rng(17 + C)
    for whole in (0, 64, 256):
        for tail in range(1, 10):
            valid = whole + tail
            for L in (valid, valid + 1, (valid + 3) // 4 * 4, valid + 7):
                data = rng.integers(0, 1 << 32, size=valid * C, dtype=np.uint64).astype(np.uint32)
                want = _expect(data, [0], [valid], L, C, layout).reshape(-1)
                for at_end in (True, False):
                    out = _aligned(L * C)
                    out[:] = NAN_FILL
                    sw.window_guarded(data, valid, L, C, layout, at_end, out)
                    assert np.array_equal(out, want), (C, layout, valid, L, at_end)


def test_refused_arguments_and_empty_calls():
    src = np.zeros(64, dtype=np.uint32)
    out = np.zeros(64, dtype=np.uint32)
    for args, why in (((src, [0], [4], 4, 0, sw.TC, out), "channels"), ((src, [0], [4], 4, 9, sw.TC, out), "channels"),
                      ((src, [0], [4], 4, 2, 2, out), "layout"), ((src, [0], [4], 4, 2, 7, out), "layout"),
                      ((src, [0], [5], 4, 2, sw.TC, out), "valid"), ((src, [0, 0], [4, 5], 4, 2, sw.CT, out), "valid"),
                      ((None, [0], [4], 4, 2, sw.TC, out), "null"), ((src, [0], [4], 4, 2, sw.CT, None), "null")):
        with pytest.raises(cx.ClaxonError) as e:
            sw.gather_windows(*args)
        assert e.value.status == cx.API_ERROR and e.value.message and why in e.value.message, (args[1:6], e.value.message)
    L = sw.lib()
    one64, one32 = np.zeros(1, dtype=np.uint64), np.full(1, 4, dtype=np.uint32)
    for first, valid in ((None, one32.ctypes.data), (one64.ctypes.data, None)):          # (a null host array)
        assert L.sim_gather_windows(src.ctypes.data, first, valid, 1, 4, 2, sw.TC, out.ctypes.data) == cx.API_ERROR
        assert b"null" in L.sim_window_error()
    # the empty calls succeed, touch nothing and need no pointer
    out[:] = NAN_FILL
    sw.gather_windows(src, [], [], 4, 2, sw.TC, out)
    sw.gather_windows(None, [], [], 4, 2, sw.CT, None)
    sw.gather_windows(src, [0, 8], [0, 0], 0, 2, sw.TC, out)
    sw.gather_windows(None, [0], [0], 0, 8, sw.CT, None)
    assert np.all(out == NAN_FILL)
    with pytest.raises(cx.ClaxonError):
        sw.gather_windows(None, [], [], 4, 0, sw.TC, None)                               # (channels and layout are checked first)
