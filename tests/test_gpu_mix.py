"""Windows at one channel count on the GPU: StreamSet.read(..., channels=K) over mono, stereo and three-channel streams of three sample
rates in one set, and clx_mix_windows itself.  The reference input is cx.load()'s tensor of each stream.  At the native rate a window
is bit-equal to the mix's definition in numpy float32 (simlib_mix.mix); at a target rate it is within the resampler's bound
(simlib_resample.assert_close: gamma = N u / (1 - N u), N = 2W + 2, unchanged because the mixed values are exact by definition) of
the definition evaluated in float64 on the mixed signal, and windows whose stream has the asked-for shape already are torch.equal to
read() without `channels`."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import md5_cases as mc
import simlib_mix as sm
import simlib_resample as sr
import synth

pytestmark = pytest.mark.gpu
R = 16000
L = 300


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _frames(rng, n, ch, bs, bps, rate, number0=0):
    """n frames (numbered from number0) of a tone with noise at `rate`: (workload, interleaved samples)."""
    lim = 1 << (bps - 1)
    t = np.arange(n * bs)
    pcm = np.empty((ch, n * bs), dtype=np.int64)
    for c in range(ch):
        pcm[c] = np.clip(np.round(0.6 * lim * np.sin(2 * np.pi * (50 + 31 * c + rng.integers(0, 200)) * t / float(rate)) +
                                  rng.normal(0, max(1.0, lim / 512), n * bs)), -lim, lim - 1)
    frames = pcm.reshape(ch, n, bs).transpose(1, 0, 2).astype(np.int32)
    fp = [synth.FrameParams() for _ in range(n)]
    po = max(p for p in range(4) if bs % (1 << p) == 0 and (bs >> p) >= 32 or p == 0)
    for i, f in enumerate(fp):
        f.number = number0 + i
        f.channel_assignment = (i % 4) if ch == 2 and bps <= 16 else 0
        for c in range(ch):
            f.sf[c] = synth.sf(synth.SF_LPC if (i + c) % 3 else synth.SF_FIXED, order=8 if (i + c) % 3 else 2, precision=12,
                               partition_order=po)
    return synth.encode_frames("mix", frames, ch, bs, bps, fp, sample_rate=rate), pcm.T.reshape(-1)


def _streaminfo(bs, ch, bps, rate, samples, md5):
    """fLaC + a STREAMINFO block (the last metadata block) of min = max block size `bs` at `rate` Hz."""
    si = bytearray(34)
    si[0:2] = bs.to_bytes(2, "big"); si[2:4] = bs.to_bytes(2, "big")
    si[10:14] = ((rate << 12) | ((ch - 1) << 9) | ((bps - 1) << 4) | (samples >> 32)).to_bytes(4, "big")
    si[14:18] = (samples & 0xffffffff).to_bytes(4, "big")
    si[18:34] = md5
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + bytes(si)


def _stream(rng, n, ch, bs, bps, rate, last=0):
    """A FLAC stream at `rate` of n frames of bs samples, then one of `last` samples when that is not 0: (bytes, frame boundaries)."""
    w, vals = _frames(rng, n, ch, bs, bps, rate)
    if last:
        w2, v2 = _frames(rng, 1, ch, last, bps, rate, number0=n)
        w, vals = synth.concat("mix", [w, w2]), np.concatenate([vals, v2])
    body = b"".join(w.arena[int(w.offs[i]):int(w.offs[i] + w.lens[i])].tobytes() for i in range(w.n))
    return (_streaminfo(bs, ch, bps, rate, vals.size // ch, mc.ref_md5(vals, bps)) + body,
            [bs * i for i in range(n + 1)] + ([bs * n + last] if last else []))


NAMES = ("s44", "m44", "s16", "m16", "t48")
SHAPES = dict(s44=(8, 2, 256, 16, 44100, 77), m44=(6, 1, 192, 24, 44100, 0), s16=(8, 2, 256, 16, 16000, 0), m16=(8, 1, 256, 16, 16000, 0),
              t48=(6, 3, 192, 16, 48000, 0))


class Stream:
    """One stream of the shard: its id in the set, its frame boundaries and its whole decode by load() (computed once, kept on the host)."""

    def __init__(self, ctx, sid, data, bounds):
        self.sid, self.data, self.bounds = sid, data, bounds
        ref, self.rate = cx.load(ctx, data)
        self.x = ref.cpu().numpy()
        self.T, self.C = self.x.shape
        assert self.T == bounds[-1]
        self.mixed = {K: sm.mix(self.x, K) for K in (1, 2) if self.C in (1, K) or K == 1}      # (the references' inputs, computed once)

    def length(self, at):
        return self.T if at in (None, self.rate) else sr.length_at(self.T, self.rate, at)

    def valid(self, st, at):
        return min(max(self.length(at) - st, 0), L)

    def frames_for(self, st, at):
        """The frames that cover the source span of the window at st, counted from the frame boundaries."""
        valid = self.valid(st, at)
        if valid == 0:
            return 0
        lo, hi = (st, st + valid) if at in (None, self.rate) else sr.span(st, st + valid - 1, self.T, self.rate, at)
        return sum(1 for a, b in zip(self.bounds[:-1], self.bounds[1:]) if a < hi and b > lo)

    def starts(self, at):
        """0, every frame boundary mapped to the output rate and +-1 around it, across the stream's end, at it and behind it."""
        o, n, _ = cx.resample_pair(self.rate, self.rate if at is None else at)
        T_R = self.length(at)
        st = {0, T_R - L // 2, T_R - 1, T_R, T_R + 5}
        for b in self.bounds:
            st |= {b * n // o + d for d in (-1, 0, 1)}
        return sorted(s for s in st if s >= 0)

    def check(self, got, st, K, at, what):
        """got [L, K] (a numpy array): the window at st of this stream brought to K channels, at its own rate (at None) or at `at`."""
        valid = self.valid(st, at)
        assert np.all(got[valid:].view(np.uint32) == 0), (what, "the window's tail is not zeros")
        want = self.mixed[K]
        if at in (None, self.rate):
            assert np.array_equal(got[:valid].view(np.uint32), want[st:st + valid].view(np.uint32)), (what, "not the mix of the copy")
        elif valid:
            sr.assert_close(got[:valid], want, self.rate, at, np.arange(st, st + valid), what)
        if self.C == 1:
            for c in range(1, K):
                assert np.array_equal(got[:, c].view(np.uint32), got[:, 0].view(np.uint32)), (what, "replicated channels differ")
        return valid


@pytest.fixture(scope="module")
def shard(ctx):
    rng = np.random.default_rng(2026)
    made = [_stream(rng, *SHAPES[name]) for name in NAMES]
    streams = {name: Stream(ctx, i, *made[i]) for i, name in enumerate(NAMES)}
    s = cx.open_streams(ctx, [m[0] for m in made])
    assert s.problems == [None] * 5 and s.channels == [2, 1, 2, 1, 3] and s.sample_rates == [44100, 44100, 16000, 16000, 48000]
    return s, streams


def _windows(streams, names, at):
    """(names, stream ids, starts) of every start of every named stream."""
    who = [n for n in names for _ in streams[n].starts(at)]
    return who, [streams[n].sid for n in who], [st for n in names for st in streams[n].starts(at)]


def _read(s, streams, names, K, at, layout="tc"):
    """One read(channels=K) over every start of the named streams, checked window by window; returns (who, sid, starts, out as
    [B, L, K] on the device)."""
    who, sid, starts = _windows(streams, names, at)
    n0 = s.frames_decoded
    out, valid = s.read(sid, starts, L, layout=layout, sample_rate=at, channels=K)
    assert s.frames_decoded - n0 == sum(streams[n].frames_for(st, at) for n, st in zip(who, starts))
    assert out.shape == ((len(sid), L, K) if layout == "tc" else (len(sid), K, L)) and out.is_contiguous() and out.dtype == torch.float32
    assert valid.dtype == torch.int64 and valid.tolist() == [streams[n].valid(st, at) for n, st in zip(who, starts)]
    out = out if layout == "tc" else out.transpose(1, 2)
    h = out.cpu().numpy()
    for k, (n, st) in enumerate(zip(who, starts)):
        streams[n].check(np.ascontiguousarray(h[k]), st, K, at, (n, st, K, at, layout))
    return who, sid, starts, out


def _rows(who, names):
    return [k for k, n in enumerate(who) if n in names]


@pytest.mark.parametrize("name", ("s16", "t48"))
def test_gpu_mono_at_the_native_rate(shard, name):
    s, streams = shard
    _, _, _, tc = _read(s, streams, [name], 1, None, "tc")
    _, _, _, ct = _read(s, streams, [name], 1, None, "ct")
    assert torch.equal(tc, ct)                               # (K = 1: the two layouts are the same bytes)


def test_gpu_stereo_at_the_native_rate(shard):
    s, streams = shard
    for layout in ("tc", "ct"):
        who, sid, starts, out = _read(s, streams, ["m16", "s16"], 2, None, layout)
        k = _rows(who, ["s16"])
        plain, _ = s.read([sid[i] for i in k], [starts[i] for i in k], L)
        assert torch.equal(out[k], plain)


def test_gpu_mono_at_16k_from_three_rates_and_three_channel_counts(shard):
    s, streams = shard
    for layout in ("tc", "ct"):
        who, sid, starts, out = _read(s, streams, NAMES, 1, R, layout)
        k = _rows(who, ["m16"])
        plain, _ = s.read([sid[i] for i in k], [starts[i] for i in k], L)
        assert torch.equal(out[k], plain)


def test_gpu_stereo_at_16k(shard):
    s, streams = shard
    for layout in ("tc", "ct"):
        who, sid, starts, out = _read(s, streams, ["m44", "s44", "m16", "s16"], 2, R, layout)
        k = _rows(who, ["s44", "s16"])
        plain, _ = s.read([sid[i] for i in k], [starts[i] for i in k], L, sample_rate=R)
        assert torch.equal(out[k], plain)


def test_gpu_streams_that_have_k_channels_take_the_old_path(shard):
    s, streams = shard
    for names, K, at in ((["s44", "s16"], 2, R), (["s16"], 2, None), (["m44", "m16"], 1, R), (["t48"], 3, None)):
        who, sid, starts = _windows(streams, names, at)
        for layout in ("tc", "ct"):
            a, va = s.read(sid, starts, L, layout=layout, sample_rate=at)
            b, vb = s.read(sid, starts, L, layout=layout, sample_rate=at, channels=K)
            assert torch.equal(a, b) and torch.equal(va, vb)
    out, valid = s.read([], [], 16, layout="ct", channels=4)
    assert out.shape == (0, 4, 16) and valid.shape == (0,)
    out, valid = s.read([0, 1], [0, 5], 0, channels=1)
    assert out.shape == (2, 0, 1) and valid.tolist() == [0, 0]


def test_gpu_raw_mix_windows(ctx):
    """clx_mix_windows itself on a random device buffer, the output pre-filled with NaNs and a guard word behind it: spans at odd
    float offsets, 8 -> 1 and 1 -> 8, L = one tile and one output, a job without outputs, and out_t0 = 2^40 + 3 (at the native rate
    with src_t0 to match; resampled, moved by whole periods: q n outputs and q o source samples)."""
    rng = np.random.default_rng(31)
    Lr, T, fs, big = 1025, 3300, 44100, (1 << 40) + 3
    x8, x1 = (rng.uniform(-1, 1, size=(T, C)).astype(np.float32) for C in (8, 1))
    o, n, _ = sr.pair(fs, R)
    q, st_big = divmod(big, n)
    T_R = sr.length_at(T, fs, R)
    assert T_R - st_big >= Lr

    for x, K, base in ((x8, 1, 3), (x1, 8, 3 + x8.size)):
        Cs = x.shape[1]
        src = torch.from_numpy(np.concatenate([np.zeros(3, np.float32), x8.reshape(-1), x1.reshape(-1)])).to("cuda:0")
        jobs = []                                            # (rate, local start, valid, out_t0 shift, src_t0 shift)
        jobs.append((R, 5, Lr, 0, 0))
        jobs.append((fs, 40, Lr, 0, 0))
        jobs.append((fs, T_R + 9, 0, 0, 0))
        jobs.append((R, 7, Lr, big - 7, big - 7))
        jobs.append((fs, st_big, Lr, q * n, q * o))
        jobs.append((fs, T_R - 100, 100, 0, 0))
        first, t0, sn, o0, valid, rates = [], [], [], [], [], []
        for rate, st, v, d_out, d_src in jobs:
            lo, hi = (0, 0) if v == 0 else (st, st + v) if rate == R else sr.span(st, st + v - 1, T, rate, R)
            first.append(base + lo * Cs); t0.append(lo + d_src); sn.append(hi - lo); o0.append(st + d_out); valid.append(v); rates.append(rate)
        assert any(f % 2 for f in first)
        want = sm.mix(x, K)
        B, n_out = len(jobs), len(jobs) * Lr * K
        outs = []
        for layout in (cx.WINDOW_TC, cx.WINDOW_CT):
            fill = np.full(n_out + 1, 0x7fc0dead, dtype=np.uint32)                 # (a NaN pattern, and the guard word behind it)
            fill[n_out] = 0xffc0beef
            flat = torch.from_numpy(fill.view(np.float32)).to("cuda:0")
            out = flat[:n_out].view((B, Lr, K) if layout == cx.WINDOW_TC else (B, K, Lr))
            ctx.mix_windows(src, first, t0, sn, o0, valid, rates, [Cs] * B, R, Lr, K, layout, out)
            torch.cuda.synchronize()
            h = flat.cpu().numpy()
            assert h[n_out:].view(np.uint32)[0] == 0xffc0beef, "the word behind the output was written"
            got = h[:n_out].reshape(out.shape)
            got = got if layout == cx.WINDOW_TC else got.transpose(0, 2, 1)
            outs.append(np.ascontiguousarray(got))
            for k, (rate, st, v, _, _) in enumerate(jobs):
                what = (Cs, K, layout, k)
                assert np.all(got[k, v:].view(np.uint32) == 0), what
                if rate == R:
                    assert np.array_equal(got[k, :v].view(np.uint32), want[st:st + v].view(np.uint32)), what
                elif v:
                    sr.assert_close(got[k, :v], want, rate, R, np.arange(st, st + v), what)
                for c in range(1, K):
                    assert np.array_equal(got[k, :, c].view(np.uint32), got[k, :, 0].view(np.uint32)), what
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    for change, why in ((dict(K=0), "out_channels"), (dict(K=9), "out_channels"), (dict(Cs=0), "src_channels"), (dict(Cs=9), "src_channels"),
                        (dict(Cs=3, K=2), "no rule"), (dict(R=16001), "table"), (dict(layout=5), "layout")):
        a = dict(dict(Cs=1, K=8, R=R, layout=cx.WINDOW_TC), **change)
        with pytest.raises(cx.ClaxonError) as e:
            ctx.mix_windows(src, first, t0, sn, o0, valid, rates, [a["Cs"]] * B, a["R"], Lr, a["K"], a["layout"], out)
        assert e.value.status == cx.API_ERROR and why in e.value.message and e.value.message.startswith("clx_mix_windows")


def test_gpu_refusals(shard):
    s, streams = shard
    t48, m16, s16 = (streams[n].sid for n in ("t48", "m16", "s16"))
    for bad in (0, 9, 2.5, True, -1, "2"):
        with pytest.raises(ValueError) as e:
            s.read([s16], [0], 16, channels=bad)
        assert "channels" in str(e.value)
        with pytest.raises(ValueError):
            s.read([s16], [0], 16, sample_rate=R, channels=bad)
    with pytest.raises(ValueError) as e:
        s.read([m16, t48], [0, 0], 16, channels=2)
    assert "3 channels" in str(e.value) and "to 2" in str(e.value) and "window 1" in str(e.value)
    with pytest.raises(ValueError):
        s.read([t48], [0], 16, sample_rate=R, channels=2)
    with pytest.raises(ValueError) as e:
        s.read([m16, s16], [0, 0], 16)                       # (channels=None: today's refusal, today's text)
    assert "differ in their channel count" in str(e.value)
    with pytest.raises(ValueError) as e:
        s.read([m16, s16], [0, 0], 16, sample_rate=R, channels=None)
    assert "differ in their channel count" in str(e.value)
    out, valid = s.read([t48, s16, m16], [3, 3, 10 ** 9], 16, channels=1)     # (and the set reads on)
    assert out.shape == (3, 16, 1) and valid.tolist() == [16, 16, 0]
