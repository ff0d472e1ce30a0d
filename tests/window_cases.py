"""The case matrix of the window gather (clx_k_window), shared by the wave simulator (test_window_sim.py) and the GPU
(test_gpu_window_edges.py).  The reference is numpy slicing of the same 32-bit words.

Every check takes a runner, run(src_u32, src_first, valid, L, C, layout, out_offset_words=0) -> (output words, guards intact):
clx_gather_windows over the host array `src_u32` into an output of the runner's own that starts out_offset_words words behind a
16-byte boundary, holds NAN_FILL in every word before the call and has guard words round it.  Each check returns (calls, words
compared)."""
import numpy as np

NAN_FILL = 0x7fc0dead            # a quiet NaN with a payload: what the output holds before the call
TC, CT = 0, 1                    # CLX_WINDOW_TC, CLX_WINDOW_CT
LAYOUTS = (TC, CT)
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000)
CHANNELS = (1, 2, 3, 4, 5, 6, 7, 8)                                   # each instance of put_tile_ct<C> and the one-channel path
OFF_GRID = ((5, 3), (64, 2), (257, 1), (256, 8))                      # (L, C) of the outputs 1..3 words off the 16-byte grid ...
OFF_GRID_MORE = ((64, 5),)                                           # ... and, with a seed of their own, these
TILES = ((4096 + 5, 2), (2 * 4096, 1), (4099, 3), (2 * 4096, 2))      # (L, C) of windows of several tiles; the last: CT's fast path
BATCHES = (0, 1, 70)


def aligned(n_words, offset_words=0, align=64, fill=0):
    """A uint32 array of n_words whose first word sits offset_words words behind an `align`-byte boundary, cut from a larger array
    that holds `fill`: (the larger array, the n_words of it)."""
    raw = np.full(n_words + align // 4 + offset_words + 4, fill, dtype=np.uint32)
    at = ((-raw.ctypes.data) % align) // 4 + offset_words
    return raw, raw[at:at + n_words]


def source(rng, n_words):
    """Any bit pattern, NaNs and denormals too -- but for the fill pattern, which no output word may keep."""
    src = aligned(n_words)[1]
    src[:] = rng.integers(0, 1 << 32, size=n_words, dtype=np.uint64).astype(np.uint32)
    src[src == NAN_FILL] ^= 1
    return src


def expect(src, src_first, valid, L, C, layout):
    out = np.zeros((len(src_first), L, C), dtype=np.uint32)
    for k, (s, v) in enumerate(zip(src_first, valid)):
        out[k, :v] = src[int(s):int(s) + int(v) * C].reshape(int(v), C)
    return np.ascontiguousarray(out.transpose(0, 2, 1)) if layout == CT else out


def check(run, src, src_first, valid, L, C, layout, out_offset_words=0):
    """One call: the guards are intact, no output word keeps the fill, every word is numpy's (so the words past valid are 0)."""
    what = (len(src_first), L, C, "ct" if layout == CT else "tc", out_offset_words)
    got, guards_intact = run(src, src_first, valid, L, C, layout, out_offset_words)
    assert guards_intact, (what, "a word outside the output was written")
    got = np.asarray(got).reshape(-1)
    want = expect(src, src_first, valid, L, C, layout)
    for k, v in enumerate(valid):
        tail = want[k, :, int(v):] if layout == CT else want[k, int(v):]
        assert not tail.any()
    want = want.reshape(-1)
    assert got.dtype == np.uint32 and got.size == want.size, (what, got.dtype, got.size)
    left = int(np.count_nonzero(got == NAN_FILL))
    assert left == 0, (what, "%d of %d output words still hold the fill pattern" % (left, got.size))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, "%d words differ; the first is word %d: %#x, expected %#x" % (bad.size, bad[0], got[bad[0]], want[bad[0]]))
    return want.size


def check_lengths_alignments_and_valid_counts(run, C, layout):
    """Every L, with one call of 32 windows each: src_first mod 8 over 0..7 times valid in {0, 1, L-1, L}."""
    rng = np.random.default_rng(100 * C + layout)
    words = 0
    for L in LENGTHS:
        src = source(rng, 32 * (L * C + 16) + 64)
        first, valid, at = [], [], 0
        for a in range(8):
            for v in (0, 1, L - 1, L):
                at = (at + 7) // 8 * 8 + a
                first.append(at)
                valid.append(v)
                at += L * C
        assert all(f % 8 == k // 4 for k, f in enumerate(first))
        words += check(run, src, first, valid, L, C, layout)
    return len(LENGTHS), words


def check_output_on_a_4_byte_boundary_only(run, layout):
    """An output 1..3 words off the 16-byte grid: every row has a ragged head and tail, the first window's head shares its vector
    with the words in front of the output, and neighbouring rows share a vector."""
    calls = words = 0
    for seed, pairs in ((7, OFF_GRID), (8, OFF_GRID_MORE)):
        rng = np.random.default_rng(seed)
        for off in (1, 2, 3):
            for L, C in pairs:
                src = source(rng, 4 * L * C + 16)
                words += check(run, src, [3, L * C + 2, 1], [L, L - 1, L], L, C, layout, out_offset_words=off)
                calls += 1
    return calls, words


def check_batch_sizes(run, B, layout):
    """No window, one, and 70 (more than a wave has lanes) with mixed valid counts in one call."""
    rng = np.random.default_rng(B)
    words = 0
    for L, C in ((257, 2), (256, 3), (1000, 2)):
        src = source(rng, 8192)
        first = rng.integers(0, 8192 - L * C, size=B)
        valid = rng.integers(0, L + 1, size=B)
        if B:
            valid[0] = L
            valid[-1] = 0
        words += check(run, src, first, valid, L, C, layout)
    return 3, words


def check_a_window_of_several_tiles(run, layout):
    """Windows longer than one tile of 4096 floats / samples: the tiles of a window meet without a gap, the last one is partial;
    valid = L, L - 3 and 4097 (one sample into the second tile)."""
    rng = np.random.default_rng(11)
    words = 0
    for L, C in TILES:
        src = source(rng, 2 * L * C + 64)
        words += check(run, src, [5, L * C - 7, 0], [L, L - 3, 4097], L, C, layout)
    return len(TILES), words


def check_overlapping_and_descending_windows(run, layout):
    rng = np.random.default_rng(13)
    L, C = 65, 2
    src = source(rng, 2048)
    first = [1000, 1001, 1002, 1064, 900, 500, 499, 2, 0, 0]         # (overlapping in src, then descending, then the same twice)
    valid = [L, L, L - 1, L, 1, L, L, 0, L, L]
    return 1, check(run, src, first, valid, L, C, layout)
