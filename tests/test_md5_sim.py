"""The stream MD5 (clx_md5.hip: clx_md5_plan and clx_k_md5) under the wave simulator, against hashlib: every message length of the
padding's edges, every source format with every width it can hold, F32 sources, any alignment of a stream's start, many streams of
very different lengths in one call, loads that stay inside each stream, and the refused arguments."""
import numpy as np
import pytest

import claxon_amd as cx
import md5_cases as mc
import simlib_md5 as sm


def run_sim(buf, fmt, first, counts, bps, byte_offset=0):
    """The runner of md5_cases' checks: the source bytes as they are, or byte_offset bytes behind a 16-byte boundary of a larger array."""
    if byte_offset:
        big = np.zeros(buf.size + 64, dtype=np.uint8)
        base = (-big.ctypes.data) % 16 + byte_offset
        big[base:base + buf.size] = buf
        buf = big[base:base + buf.size]
        assert buf.ctypes.data % 16 == byte_offset
    return sm.md5_streams(buf, fmt, first, counts, bps)


def test_every_message_length_to_300_bytes():
    """0..300 message bytes at each width: the padding's edges 55/56/63/64/119/120 and every partial group."""
    assert mc.check_every_message_length(run_sim) == (4, 301 + 151 + 101 + 76)


def test_every_format_with_every_width_it_holds():
    assert mc.check_every_format_and_width(run_sim) == (3 + 6 + 9 + 12 + 9, 39 * 13)


def test_f32_extremes_scale_back_exactly():
    """The floats of -2^(bps-1) and 2^(bps-1) - 1 (the full range), 0 and +-1 for every width F32 holds."""
    assert mc.check_f32_extremes(run_sim) == (8, 24)


def test_any_alignment_of_a_stream_start():
    """Streams at odd sample indices, and the whole buffer at byte offsets 1..15 from a 16-byte boundary."""
    assert mc.check_any_alignment_of_a_stream_start(run_sim) == (5 * 16, 5 * 16 * 5)


def test_many_streams_of_very_different_lengths_in_one_call():
    """150 streams, empty ones among them, of lengths from 0 to 40000 samples and widths 1..4 (every width class, one launch each)."""
    assert mc.check_many_streams_of_mixed_width(run_sim) == (2, 300)


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
