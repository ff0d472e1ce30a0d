"""The stream MD5 (clx_md5.hip: clx_md5_plan and clx_k_md5) under the wave simulator, against hashlib: every message length of the
padding's edges, every source format with every width it can hold, F32 sources, any alignment of a stream's start, many streams of
very different lengths in one call, loads that stay inside each stream, and the refused arguments."""
import numpy as np
import pytest

import claxon_amd as cx
import md5_cases as mc
import simlib_md5 as sm


def _flat(streams, fmt, bps_list, rng=None, gap=0):
    """Streams of samples packed one after another (with `gap` samples between) in one source buffer: (buffer, first, counts)."""
    parts, first, counts, at = [], [], [], 0
    for vals, bps in zip(streams, bps_list):
        if gap:
            parts.append(mc.encode(np.zeros(gap, dtype=np.int64), fmt, bps))
            at += gap
        parts.append(mc.encode(vals, fmt, bps))
        first.append(at)
        counts.append(len(vals))
        at += len(vals)
    buf = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return buf, np.array(first, dtype=np.uint64), np.array(counts, dtype=np.uint64)


def _check(streams, fmt, bps_list, gap=0):
    buf, first, counts = _flat(streams, fmt, bps_list, gap=gap)
    got = sm.md5_streams(buf, fmt, first, counts, bps_list)
    for k, (vals, bps) in enumerate(zip(streams, bps_list)):
        assert bytes(got[k]) == mc.ref_md5(vals, bps), (k, len(vals), bps, fmt)


def test_every_message_length_to_300_bytes():
    """0..300 message bytes at each width: the padding's edges 55/56/63/64/119/120 and every partial group."""
    rng = np.random.default_rng(1)
    for w in (1, 2, 3, 4):
        bps = 8 * w
        streams = [mc.random_samples(rng, nb // w, bps) for nb in range(0, 301) if nb % w == 0]
        _check(streams, w, [bps] * len(streams))


def test_every_format_with_every_width_it_holds():
    rng = np.random.default_rng(2)
    for fmt in mc.FORMATS:
        for bps in mc.valid_bps(fmt):
            lens = [0, 1, 15, 16, 17, 63, 64, 65, 191, 192, 193, 1000, int(rng.integers(2000, 5000))]
            _check([mc.random_samples(rng, n, bps) for n in lens], fmt, [bps] * len(lens))


def test_f32_extremes_scale_back_exactly():
    """The floats of -2^(bps-1) and 2^(bps-1) - 1 (the full range), 0 and +-1 for every width F32 holds."""
    for bps in (1, 2, 8, 12, 16, 20, 23, 24):
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        vals = np.array([lo, hi, 0, 1, -1, lo + 1, hi - 1] * 37, dtype=np.int64)
        vals = np.clip(vals, lo, hi)
        _check([vals, vals[:5], vals[:64]], cx.SAMPLE_F32, [bps] * 3)


def test_any_alignment_of_a_stream_start():
    """Streams at odd sample indices, and the whole buffer at byte offsets 1..15 from a 16-byte boundary."""
    rng = np.random.default_rng(3)
    for fmt in mc.FORMATS:
        bps = 8 * min(mc.sample_size(fmt), 3)
        streams = [mc.random_samples(rng, n, bps) for n in (100, 257, 31, 640, 3)]
        _check(streams, fmt, [bps] * len(streams), gap=1)
        buf, first, counts = _flat(streams, fmt, [bps] * len(streams), gap=3)
        for off in range(1, 16):
            big = np.zeros(buf.size + 64, dtype=np.uint8)
            base = (-big.ctypes.data) % 16 + off
            big[base:base + buf.size] = buf
            got = sm.md5_streams(big[base:base + buf.size], fmt, first, counts, [bps] * len(streams))
            for k, vals in enumerate(streams):
                assert bytes(got[k]) == mc.ref_md5(vals, bps), (fmt, off, k)


def test_many_streams_of_very_different_lengths_in_one_call():
    """150 streams, empty ones among them, of lengths from 0 to 40000 samples and widths 1..4 (every width class, one launch each)."""
    rng = np.random.default_rng(4)
    lens = [0, 0, 1, 40000, 7] + [int(x) for x in rng.integers(0, 3000, size=145)]
    bps = [int(b) for b in rng.choice([4, 8, 12, 16, 20, 24, 28, 32], size=len(lens))]
    streams = [mc.random_samples(rng, n, b) for n, b in zip(lens, bps)]
    _check(streams, 4, bps)
    bps24 = [min(b, 24) for b in bps]
    _check([np.clip(s, -(1 << (b - 1)), (1 << (b - 1)) - 1) for s, b in zip(streams, bps24)], cx.SAMPLE_F32, bps24)


def test_loads_stay_inside_the_stream():
    """A stream flush against an inaccessible page on either side: whole groups, a partial group and the padding read nothing
    outside its bytes (a stray load would fault)."""
    rng = np.random.default_rng(5)
    for fmt in mc.FORMATS:
        for bps in mc.valid_bps(fmt):
            w = mc.width(bps)
            g = 64 if w == 3 else 64 // w
            for n in (0, 1, g - 1, g, 3 * g + 5, 4 * g):
                vals = mc.random_samples(rng, n, bps)
                data = mc.encode(vals, fmt, bps)
                for at_end in (True, False):
                    assert bytes(sm.md5_guarded(data, fmt, n, bps, at_end)) == mc.ref_md5(vals, bps), (fmt, bps, n, at_end)


def test_refused_arguments():
    buf = np.zeros(64, dtype=np.uint8)
    one = ([0], [4])
    for fmt, bps, why in ((0, 8, "sample_format"), (5, 8, "sample_format"), (0x105, 8, "sample_format"), (2, 0, "1..32"), (4, 33, "1..32"),
                          (1, 9, "wider"), (2, 17, "wider"), (3, 25, "wider"), (cx.SAMPLE_F32, 25, "24"), (cx.SAMPLE_F32, 32, "24")):
        with pytest.raises(cx.ClaxonError) as e:
            sm.md5_streams(buf, fmt, one[0], one[1], [bps])
        assert e.value.status == cx.API_ERROR and why in e.value.message, (fmt, bps, e.value.message)
    with pytest.raises(cx.ClaxonError) as e:
        sm.md5_streams(None, 2, [0], [4], [16])
    assert "null" in e.value.message
    assert sm.md5_streams(None, 2, [], [], []).shape == (0, 16)          # (no streams: nothing to read, success)
    with pytest.raises(cx.ClaxonError):
        sm.md5_streams(None, 7, [], [], [])                             # (the format is checked first)
