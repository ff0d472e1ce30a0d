"""The window gather (clx_window.hip: clx_window_check and clx_k_window) under the wave simulator, against numpy slicing of the same
source, bit for bit (as uint32): window lengths round the vector, wave and tile sizes, 1..8 channels, both layouts, every alignment
of a window's start, valid counts 0 / 1 / L-1 / L, more windows than a workgroup has lanes, overlapping and descending windows, an
output the test fills with NaN patterns (every element is overwritten, the float behind the output is not), loads that stay inside
[src_first, src_first + valid * C) next to an inaccessible page, and the refused arguments."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_window as sw

NAN_FILL = 0x7fc0dead            # a quiet NaN with a payload: what the output holds before the call
GUARD = 0xffc0beef               # the word behind the output
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000)
CHANNELS = (1, 2, 3, 8)
LAYOUTS = (sw.TC, sw.CT)


def _aligned(n_words, offset_words=0, align=64):
    """A uint32 array of n_words whose first word sits offset_words words behind an `align`-byte boundary."""
    raw = np.zeros(n_words + align // 4 + offset_words + 4, dtype=np.uint32)
    at = ((-raw.ctypes.data) % align) // 4 + offset_words
    return raw[at:at + n_words]


def _source(rng, n_words):
    src = _aligned(n_words)
    src[:] = rng.integers(0, 1 << 32, size=n_words, dtype=np.uint64).astype(np.uint32)     # (any bit pattern: NaNs and denormals too)
    return src


def _expect(src, src_first, valid, L, C, layout):
    out = np.zeros((len(src_first), L, C), dtype=np.uint32)
    for k, (s, v) in enumerate(zip(src_first, valid)):
        out[k, :v] = src[int(s):int(s) + int(v) * C].reshape(int(v), C)
    return np.ascontiguousarray(out.transpose(0, 2, 1)) if layout == sw.CT else out


def _run(src, src_first, valid, L, C, layout, out_offset_words=0):
    """The call on an output pre-filled with NaN patterns and followed by a guard word; returns the output, flat."""
    n = len(src_first) * L * C
    buf = _aligned(n + 1, out_offset_words)
    buf[:] = NAN_FILL
    buf[n] = GUARD
    sw.gather_windows(src, src_first, valid, L, C, layout, buf)
    assert buf[n] == GUARD, "the word behind the output was written"
    return buf[:n]


def _check(src, src_first, valid, L, C, layout, out_offset_words=0):
    got = _run(src, src_first, valid, L, C, layout, out_offset_words)
    want = _expect(src, src_first, valid, L, C, layout).reshape(-1)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (L, C, layout, out_offset_words, "first difference at word %d: %#x, expected %#x" % (bad[0], got[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_lengths_alignments_and_valid_counts(C, layout):
    """Every L, with one call of 32 windows each: src_first mod 8 over 0..7 times valid in {0, 1, L-1, L}."""
    rng = np.random.default_rng(100 * C + layout)
    for L in LENGTHS:
        src = _source(rng, 32 * (L * C + 16) + 64)
        first, valid, at = [], [], 0
        for a in range(8):
            for v in (0, 1, L - 1, L):
                at = (at + 7) // 8 * 8 + a
                first.append(at)
                valid.append(v)
                at += L * C
        assert all(f % 8 == k // 4 for k, f in enumerate(first))
        _check(src, first, valid, L, C, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_output_on_a_4_byte_boundary_only(layout):
    """An output 1..3 words off the 16-byte grid: the first window has a ragged head too."""
    rng = np.random.default_rng(7)
    for off in (1, 2, 3):
        for L, C in ((5, 3), (64, 2), (257, 1), (256, 8)):
            src = _source(rng, 4 * L * C + 16)
            _check(src, [3, L * C + 2, 1], [L, L - 1, L], L, C, layout, out_offset_words=off)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", (0, 1, 70))
def test_batch_sizes(B, layout):
    """No window, one, and 70 (more than one workgroup has lanes... and than a wave) with mixed valid counts in one call."""
    rng = np.random.default_rng(B)
    for L, C in ((257, 2), (256, 3), (1000, 2)):
        src = _source(rng, 8192)
        first = rng.integers(0, 8192 - L * C, size=B)
        valid = rng.integers(0, L + 1, size=B)
        if B:
            valid[0] = L
            valid[-1] = 0
        _check(src, first, valid, L, C, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_window_of_several_tiles(layout):
    """Windows longer than one tile of 4096 floats / samples: the tiles of a window meet without a gap, the last one is partial."""
    rng = np.random.default_rng(11)
    for L, C in ((4096 + 5, 2), (2 * 4096, 1), (4099, 3)):
        src = _source(rng, 2 * L * C + 64)
        _check(src, [5, L * C - 7, 0], [L, L - 3, 4097], L, C, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_overlapping_and_descending_windows(layout):
    rng = np.random.default_rng(13)
    L, C = 65, 2
    src = _source(rng, 2048)
    first = [1000, 1001, 1002, 1064, 900, 500, 499, 2, 0, 0]         # (overlapping in src, then descending, then the same twice)
    valid = [L, L, L - 1, L, 1, L, L, 0, L, L]
    _check(src, first, valid, L, C, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
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
