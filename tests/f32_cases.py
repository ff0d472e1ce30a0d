"""The float output (CLX_OUT_F32 / CLX_SAMPLE_F32) against the oracle: workloads and checks shared by the simulator's tests
(test_f32_output.py) and the GPU's (test_gpu_f32.py).  The reference value of sample v of a frame of `bps` bits is
v.astype(np.float32) * np.float32(2.0 ** (1 - bps)), compared bit for bit."""
import numpy as np

import claxon_amd as cx
import parity_cases as pc
import synth


def to_f32(v, bps):
    """The contract's formula (claxon_hip.h, CLX_OUT_F32)."""
    return np.asarray(v, dtype=np.int32).astype(np.float32) * np.float32(2.0 ** (1 - int(bps)))


def reference(oracle, arena, w, lens=None, check_crc=True):
    """The oracle's planar i32 decode of the workload's frames (out, statuses, msgs, end bits)."""
    ref = np.zeros(w.pcm.size, dtype=np.int32)
    r = oracle.decode_batch(arena[:w.arena_len], w.offs, w.lens if lens is None else lens, out=ref, out_offs=w.out_offs, check_crc=check_crc)
    return ref, r


def f32_of_frames(ref, descs, out_offs, n_total):
    """The interleaved float output the oracle's samples give (NaN where no frame writes)."""
    want = np.full(n_total, np.nan, dtype=np.float32)
    for i in range(descs.size):
        a, c, bs = int(out_offs[i]), int(descs["n_channels"][i]), int(descs["block_size"][i])
        want[a:a + c * bs] = to_f32(ref[a:a + c * bs].reshape(c, bs).T.reshape(-1), descs["bps"][i])
    return want


def check_f32(oracle, backend, w, damage=0.0, seed=1, truncate=0.0, verify_crc=True):
    """Every OK frame's floats are the oracle's samples through the formula, bit for bit; statuses, messages and end bits are the
    oracle's (= the planar run's).  damage: the share of frames with one bit flipped behind their header; truncate: the share whose
    max_bytes is cut short.  Returns the number of OK frames."""
    rng = np.random.default_rng(seed)
    arena = w.arena.copy()
    descs, _ = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)
    lens = np.asarray(w.lens, dtype=np.uint32).copy()
    for i in range(w.n):
        if rng.uniform() < damage:
            lo, hi = int(w.offs[i]) + int(descs["header_bytes"][i]), int(w.offs[i] + w.lens[i])
            pos = int(rng.integers(8 * lo, 8 * hi))
            arena[pos >> 3] ^= (0x80 >> (pos & 7))
        if rng.uniform() < truncate:
            lens[i] = int(rng.integers(int(descs["header_bytes"][i]) + 1, int(lens[i])))
    descs["max_bytes"] = lens
    out, res = backend.decode(arena, w.arena_len, descs, w.out_offs, verify_crc)
    ref, r = reference(oracle, arena, w, lens=lens, check_crc=verify_crc)
    st, ms = np.asarray(res["status"]), np.asarray(res["msg"])
    assert np.array_equal(st, r["statuses"]) and np.array_equal(ms, r["msgs"])
    ok = np.nonzero(st == cx.OK)[0]
    assert np.array_equal(np.asarray(res["end_bit"])[ok], r["end_bits"][ok])
    out = np.asarray(out).view(np.float32)
    for i in ok:
        a, c, bs = int(w.out_offs[i]), int(w.channels[i]), int(w.block_sizes[i])
        want = to_f32(ref[a:a + c * bs].reshape(c, bs).T.reshape(-1), descs["bps"][i])
        assert np.array_equal(out[a:a + c * bs].view(np.uint32), want.view(np.uint32)), "frame %d (%d ch, bs %d, %d bits)" % (int(i), c, bs, int(descs["bps"][i]))
    return int(ok.size)


def _lpc_frames(name, pcm, ch, bs, bps, seed, assign=None):
    S = synth
    n = pcm.shape[0]
    fp = [S.FrameParams() for _ in range(n)]
    for i, f in enumerate(fp):
        f.channel_assignment = (i % 4 if assign is None else assign) if ch == 2 else 0
        for c in range(ch):
            f.sf[c] = S.sf(S.SF_LPC if (i + c) % 3 else S.SF_FIXED, order=8 if (i + c) % 3 else 2, precision=12,
                           partition_order=min(3, max(0, int(np.log2(bs)) - 5)))
    return S.encode_frames(name, pcm, ch, bs, bps, fp)


def _tone(rng, n, ch, bs, bps, amp):
    t = np.arange(bs)
    lim = 1 << (bps - 1)
    pcm = np.empty((n, ch, bs), dtype=np.int32)
    for i in range(n):
        for c in range(ch):
            pcm[i, c] = np.clip(np.round(amp * lim * np.sin(2 * np.pi * (60 + 13 * i + 7 * c) * t / 44100.0 + 0.3 * c) + rng.normal(0, 2.0, bs)), -lim, lim - 1)
    return pcm


def narrow_widths_workload():
    """Stereo frames of 8, 12 and 16 bits side by side in the 16-bit tier's waves (every row's own scale), one block size; mono frames of
    8 and 16 bits with lone last tiles (block sizes 16 mod 32); stereo frames with a lone last tile."""
    S = synth
    rng = np.random.default_rng(3232)
    parts = []
    for k in range(3):
        for bps in (8, 12, 16):
            parts.append(_lpc_frames("stereo %d bits #%d" % (bps, k), _tone(rng, 12, 2, 1024, bps, 0.4), 2, 1024, bps, k))
    for bps in (8, 16):
        parts.append(_lpc_frames("mono %d bits lone tile" % bps, _tone(rng, 40, 1, 1024 + 16, bps, 0.5), 1, 1024 + 16, bps, 5))
    parts.append(_lpc_frames("stereo lone tile", _tone(rng, 40, 2, 2048 + 16, 16, 0.5), 2, 2048 + 16, 16, 6))
    return S.concat("f32 widths", parts)


def split_workload():
    """The split tier's float build: config 4 (24-bit stereo, 32 taps), 16-bit groups of more than 12 taps, mono frames of 24 bits and
    multichannel / odd frames (the general kernels), config 5's real-world 16-bit shapes."""
    S = synth
    return S.concat("f32 split", [S.config4(48), pc.lean24_workload(), S.small_mixed(60), S.config5_unique(48)])


def fixture_workload(path):
    """A whole FLAC file's frames as a workload (synth.Workload), the frames indexed on the host."""
    data = np.fromfile(path, dtype=np.uint8)
    st, _, _, off = cx.read_stream_header(data)
    assert st == cx.OK
    descs, _, stop = cx.index_frames(data, start=off)
    ends = np.append(descs["byte_off"][1:], stop).astype(np.uint64)
    lens = (ends - descs["byte_off"]).astype(np.uint32)
    bs = descs["block_size"].astype(np.uint64) * descs["n_channels"].astype(np.uint64)
    out_offs = np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64)
    arena = np.zeros(((data.size + 15) // 16) * 16 + 64, dtype=np.uint8)
    arena[:data.size] = data
    return synth.Workload(path, arena, descs["byte_off"], lens, descs["n_channels"], descs["block_size"], descs["bps"],
                          descs["channel_assignment"], np.zeros(int(bs.sum()), dtype=np.int32), out_offs)
