"""The shard of the batched-indexer tests (simulator and GPU): many streams at 16-byte aligned places of one arena, and the yardstick
for each -- the host indexer on that stream alone (claxon_amd.index_frames), which the batched indexer never sees."""
import glob
import os

import numpy as np

import claxon_amd as cx
import md5_cases as mc
import synth
import test_indexer
from conftest import FIXTURES


def sync_dense(n_bytes=64 << 10):
    """One valid 6-byte frame header (CRC-8 correct) repeated back to back: a candidate every 6 bytes, more than one per 16."""
    h = bytes([0xff, 0xf8, 0xc9, 0xa8, 0x00])
    h += bytes([cx.crc8(h)])
    assert cx.parse_frame_header(h + bytes(14))[0] == cx.OK
    return np.frombuffer(h * (n_bytes // 6), dtype=np.uint8)


def _md5_stream(seed, n, ch, bs, bps):
    rng = np.random.default_rng(seed)
    lim = 1 << (bps - 1)
    t = np.arange(n * bs)
    pcm = np.empty((ch, n * bs), dtype=np.int64)
    for c in range(ch):
        pcm[c] = np.clip(np.round(0.5 * lim * np.sin(2 * np.pi * (70 + 40 * c + seed) * t / 44100.0) + rng.normal(0, max(1.0, lim / 256), n * bs)),
                         -lim, lim - 1)
    fp = [synth.FrameParams() for _ in range(n)]
    for i, f in enumerate(fp):
        f.number = i
        for c in range(ch):
            f.sf[c] = synth.sf(synth.SF_LPC if (i + c) % 3 else synth.SF_FIXED, order=8 if (i + c) % 3 else 2, precision=12, partition_order=3)
    w = synth.encode_frames("index", pcm.reshape(ch, n, bs).transpose(1, 0, 2).astype(np.int32), ch, bs, bps, fp)
    return np.frombuffer(mc.stream(w, bs, ch, bps, pcm.T.reshape(-1)), dtype=np.uint8)


_STREAMS = None


def streams():
    """[(name, bytes uint8, start offset)] -- built once."""
    global _STREAMS
    if _STREAMS is not None:
        return _STREAMS
    out = [(n, np.ascontiguousarray(d), int(s)) for n, d, s in test_indexer.streams() if n != "empty"]
    for p in sorted(glob.glob(os.path.join(FIXTURES, "fuzz", "*.flac"))):
        data = np.frombuffer(open(p, "rb").read(), dtype=np.uint8)
        st, _, _, off = cx.read_stream_header(data)
        if st == cx.OK:
            out.append(("fuzz/" + os.path.basename(p)[:8], data, off))
    k = 0
    for bps in (8, 16, 24):
        for ch in (1, 2):
            data = _md5_stream(300 + k, 3 + k, ch, 576, bps)
            st, _, _, off = cx.read_stream_header(data)
            assert st == cx.OK
            out.append(("md5_%d_%d" % (bps, ch), data, off))
            k += 1
    w = synth.config5_unique(24)
    body = w.arena[:w.arena_len].copy()
    out.append(("len0", body[:0], 0))
    out.append(("len1", body[:1], 0))
    whole = int(w.offs[16])                                  # 16 frames, zero padded to a multiple of 16: the next stream lies flush
    flush = np.concatenate([body[:whole], np.zeros((-whole) % 16, dtype=np.uint8)])
    assert flush.size % 16 == 0
    out.append(("flush", flush, 0))
    out.append(("twice_a", body, 0))
    out.append(("twice_b", body, 0))
    cut = (int(w.offs[9]) + 15) // 16 * 16 + 160             # a multiple of 16 inside frame 9
    assert cut % 16 == 0 and int(w.offs[9]) < cut < int(w.offs[10]) and not np.any(w.offs == cut)
    out.append(("cut_head", body[:cut], 0))
    out.append(("cut_tail", body[cut:], 0))
    out.append(("truncated", body[:int(w.offs[23]) + 100], 0))
    out.append(("sync_dense", sync_dense(), 0))
    _STREAMS = out
    return out


def host_answers(cases):
    """The yardstick: per stream (descs, headers, stop) of the host indexer on that stream alone."""
    return [cx.index_frames(d, s) for _, d, s in cases]


def shard(cases, order=None):
    """The cases laid out in `order` at 16-byte aligned places: (arena uint8, offs, lens, starts, order)."""
    order = list(range(len(cases))) if order is None else list(order)
    offs, at = [], 0
    for k in order:
        offs.append(at)
        at = (at + cases[k][1].size + 15) // 16 * 16
    arena = np.zeros(at, dtype=np.uint8)
    for o, k in zip(offs, order):
        arena[o:o + cases[k][1].size] = cases[k][1]
    # the arena's length is the last stream's end (no padding counted): a stream flush against it is a case too
    arena_len = max([o + cases[k][1].size for o, k in zip(offs, order)] + [0])
    return (arena[:arena_len], np.array(offs, dtype=np.uint64), np.array([cases[k][1].size for k in order], dtype=np.uint64),
            np.array([cases[k][2] for k in order], dtype=np.uint64), order)


def expected(cases, answers, offs, order):
    """What the batched indexer must return for the shard, from the per-stream host answers: (descs, headers, first_frame, stop_offs)."""
    descs, hdrs, first, stops = [], [], [0], []
    for o, k in zip(offs.tolist(), order):
        d, h, stop = answers[k]
        d = d.copy()
        d["byte_off"] += np.uint64(o)
        descs.append(d)
        hdrs.append(h)
        first.append(first[-1] + d.size)
        stops.append(o + stop)
    return (np.concatenate(descs), np.concatenate(hdrs), np.array(first, dtype=np.uint64), np.array(stops, dtype=np.uint64))


def check_shape(cases, answers):
    """The conditions that keep a test from hiding a failure."""
    assert len(cases) >= 24, len(cases)
    total = sum(a[0].size for a in answers)
    assert total >= 300, total
    by = {n: a for (n, _, _), a in zip(cases, answers)}
    assert [by[n][0].size for n in ("synthetic", "garbage_tail", "broken_frame", "mid_start", "not_a_frame")] == [120, 119, 40, 113, 0]
    assert by["cut_head"][0].size == 9 and by["cut_tail"][0].size == 0 and by["flush"][0].size == 16 and by["truncated"][0].size == 23
    assert by["len0"][0].size == 0 and by["len1"][0].size == 0


def assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, ("descs", "headers", "first_frame", "stop_offs")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)
