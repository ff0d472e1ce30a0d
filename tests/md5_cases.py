"""Shared pieces of the stream MD5 tests: the FLAC rule on the host (hashlib) and source buffers in every sample format."""
import hashlib

import numpy as np

import claxon_amd as cx

FORMATS = (1, 2, 3, 4, cx.SAMPLE_F32)


def width(bps):
    return (int(bps) + 7) // 8


def ref_md5(vals, bps):
    """FLAC's signature of the interleaved samples `vals`: each as its low ceil(bps / 8) bytes, little-endian."""
    v = np.asarray(vals, dtype=np.int64).reshape(-1)
    w = width(bps)
    b = np.stack([(v >> (8 * k)) & 0xff for k in range(w)], axis=1).astype(np.uint8) if v.size else np.zeros(0, np.uint8)
    return hashlib.md5(b.tobytes()).digest()


def random_samples(rng, n, bps):
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1))
    return rng.integers(lo, hi, size=n, dtype=np.int64)


def encode(vals, fmt, bps):
    """The samples as a source buffer of `fmt` (uint8): little-endian PCM of fmt bytes, or the floats of CLX_OUT_F32."""
    v = np.asarray(vals, dtype=np.int64).reshape(-1)
    if fmt == cx.SAMPLE_F32:
        return (v.astype(np.float64) * 2.0 ** -(bps - 1)).astype(np.float32).view(np.uint8)
    return np.stack([(v >> (8 * k)) & 0xff for k in range(fmt)], axis=1).astype(np.uint8).reshape(-1)


def sample_size(fmt):
    return 4 if fmt == cx.SAMPLE_F32 else fmt


def valid_bps(fmt):
    top = 24 if fmt == cx.SAMPLE_F32 else 8 * fmt
    return [b for b in (1, 5, 8, 9, 12, 16, 17, 20, 24, 25, 31, 32) if b <= top]


# ---- the case matrix, shared by the wave simulator (test_md5_sim.py) and the GPU (test_gpu_md5_edges.py) ----------------------------
#
# Every check takes a runner, run(buf_u8, fmt, first, counts, bps, byte_offset=0) -> uint8 [n, 16]: clx_md5_streams over the source
# bytes `buf_u8` (a host array), which the runner places byte_offset bytes behind a 16-byte boundary of its own memory.  The expected
# digests are hashlib's (ref_md5), every stream of every call is compared, and each check returns (calls, streams compared).

LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 191, 192, 193, 1000)      # samples, then one of 2000..5000 (check_every_format_and_width)
F32_EXTREME_BPS = (1, 2, 8, 12, 16, 20, 23, 24)


def flat(streams, fmt, bps_list, gap=0):
    """Streams of samples packed one after another (with `gap` samples between) in one source buffer: (buffer, first, counts)."""
    parts, first, counts, at = [], [], [], 0
    for vals, bps in zip(streams, bps_list):
        if gap:
            parts.append(encode(np.zeros(gap, dtype=np.int64), fmt, bps))
            at += gap
        parts.append(encode(vals, fmt, bps))
        first.append(at)
        counts.append(len(vals))
        at += len(vals)
    buf = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return buf, np.array(first, dtype=np.uint64), np.array(counts, dtype=np.uint64)


def compare(got, streams, bps_list, what):
    """Every digest of one call against hashlib; returns the streams compared."""
    assert got.shape == (len(streams), 16), (what, got.shape)
    for k, (vals, bps) in enumerate(zip(streams, bps_list)):
        assert bytes(got[k]) == ref_md5(vals, bps), (what, "stream %d: %d samples of %d bits" % (k, len(vals), bps))
    return len(streams)


def check(run, streams, fmt, bps_list, gap=0):
    buf, first, counts = flat(streams, fmt, bps_list, gap=gap)
    return compare(run(buf, fmt, first, counts, bps_list), streams, bps_list, (fmt, gap))


def check_every_message_length(run):
    """0..300 message bytes at each width, one call per width: the padding's edges 55/56/63/64/119/120 and every partial group.
    Width 1 is 301 streams of one class: five workgroups, the last of 45 lanes."""
    rng = np.random.default_rng(1)
    calls = n = 0
    for w in (1, 2, 3, 4):
        bps = 8 * w
        streams = [random_samples(rng, nb // w, bps) for nb in range(0, 301) if nb % w == 0]
        n += check(run, streams, w, [bps] * len(streams))
        calls += 1
    return calls, n


def check_every_format_and_width(run):
    """Every source format with every width it can hold (the 13 instances of clx_md5::stream), lengths round the group sizes."""
    rng = np.random.default_rng(2)
    calls = n = 0
    for fmt in FORMATS:
        for bps in valid_bps(fmt):
            lens = list(LENGTHS) + [int(rng.integers(2000, 5000))]
            n += check(run, [random_samples(rng, x, bps) for x in lens], fmt, [bps] * len(lens))
            calls += 1
    return calls, n


def check_f32_extremes(run):
    """The floats of -2^(bps-1) and 2^(bps-1) - 1 (the full range), 0 and +-1 for every width F32 holds."""
    calls = n = 0
    for bps in F32_EXTREME_BPS:
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        vals = np.array([lo, hi, 0, 1, -1, lo + 1, hi - 1] * 37, dtype=np.int64)
        vals = np.clip(vals, lo, hi)
        n += check(run, [vals, vals[:5], vals[:64]], cx.SAMPLE_F32, [bps] * 3)
        calls += 1
    return calls, n


def check_any_alignment_of_a_stream_start(run):
    """Streams at odd sample indices, and the whole buffer at byte offsets 1..15 from a 16-byte boundary, for every format."""
    rng = np.random.default_rng(3)
    calls = n = 0
    for fmt in FORMATS:
        bps = 8 * min(sample_size(fmt), 3)
        streams = [random_samples(rng, x, bps) for x in (100, 257, 31, 640, 3)]
        n += check(run, streams, fmt, [bps] * len(streams), gap=1)
        buf, first, counts = flat(streams, fmt, [bps] * len(streams), gap=3)
        for off in range(1, 16):
            got = run(buf, fmt, first, counts, [bps] * len(streams), byte_offset=off)
            n += compare(got, streams, [bps] * len(streams), (fmt, "byte offset %d" % off))
        calls += 16
    return calls, n


def check_many_streams_of_mixed_width(run):
    """150 streams, empty ones among them, of lengths from 0 to 40000 samples and widths 1..4 (every width class, one launch each)
    through format 4, and clipped to 24 bits through F32: each digest at the caller's index, whatever order the plan sorts into."""
    rng = np.random.default_rng(4)
    lens = [0, 0, 1, 40000, 7] + [int(x) for x in rng.integers(0, 3000, size=145)]
    bps = [int(b) for b in rng.choice([4, 8, 12, 16, 20, 24, 28, 32], size=len(lens))]
    streams = [random_samples(rng, x, b) for x, b in zip(lens, bps)]
    n = check(run, streams, 4, bps)
    bps24 = [min(b, 24) for b in bps]
    n += check(run, [np.clip(s, -(1 << (b - 1)), (1 << (b - 1)) - 1) for s, b in zip(streams, bps24)], cx.SAMPLE_F32, bps24)
    return 2, n


def streaminfo(bs, ch, bps, samples, md5):
    """fLaC + a STREAMINFO block (the last metadata block) of min = max block size `bs`, 44.1 kHz, `samples` per channel, `md5`."""
    si = bytearray(34)
    si[0:2] = bs.to_bytes(2, "big"); si[2:4] = bs.to_bytes(2, "big")
    si[10:14] = ((44100 << 12) | ((ch - 1) << 9) | ((bps - 1) << 4) | (samples >> 32)).to_bytes(4, "big")
    si[14:18] = (samples & 0xffffffff).to_bytes(4, "big")
    si[18:34] = md5
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + bytes(si)


def stream(w, bs, ch, bps, vals, frames=None):
    """fLaC + STREAMINFO (sample count and MD5 of the source PCM `vals`) + the workload's frames (or the frame order `frames`)."""
    order = range(w.n) if frames is None else frames
    body = b"".join(w.arena[int(w.offs[i]):int(w.offs[i] + w.lens[i])].tobytes() for i in order)
    return streaminfo(bs, ch, bps, vals.size // ch, ref_md5(vals, bps)) + body
