"""Windows at a target sample rate on the GPU: StreamSet.read(..., sample_rate=R), StreamSet.lengths_at and clx_resample_windows.  The
reference is the resampler's definition evaluated in float64 with numpy (simlib_resample.reference) from cx.load()'s tensor of each
stream; per output |y - y64| <= gamma * sum_k |h_k x_k|, gamma = N u / (1 - N u), u = 2^-24, N = 2W + 2, and exactly 0 where no tap
lies inside the stream.  Windows of a stream that has the target rate already are torch.equal to read() without sample_rate."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import md5_cases as mc
import simlib_resample as sr
import synth

pytestmark = pytest.mark.gpu
R = 16000


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
    return synth.encode_frames("resample", frames, ch, bs, bps, fp, sample_rate=rate), pcm.T.reshape(-1)


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
        w, vals = synth.concat("resample", [w, w2]), np.concatenate([vals, v2])
    body = b"".join(w.arena[int(w.offs[i]):int(w.offs[i] + w.lens[i])].tobytes() for i in range(w.n))
    return (_streaminfo(bs, ch, bps, rate, vals.size // ch, mc.ref_md5(vals, bps)) + body,
            [bs * i for i in range(n + 1)] + ([bs * n + last] if last else []))


class Case:
    """A stream, its whole decode by load() (computed once, kept on the host as the reference's input) and its single-stream set;
    `at` is the rate its windows are read at."""

    def __init__(self, ctx, data, bounds, at=R):
        self.data, self.bounds, self.at, self.worst = data, bounds, at, 0.0
        ref, self.rate = cx.load(ctx, data)
        self.x = ref.cpu().numpy()
        self.T, self.C = self.x.shape
        assert self.T == bounds[-1]
        self.T_R = self.T if self.rate == at else sr.length_at(self.T, self.rate, at)
        self.set = cx.open_streams(ctx, [data])
        assert self.set.problems == [None] and self.set.sample_rates == [self.rate] and int(self.set.lengths[0]) == self.T

    def span(self, st, valid):
        return (st, st + valid) if self.rate == self.at else sr.span(st, st + valid - 1, self.T, self.rate, self.at)

    def frames_for(self, st, L):
        """The frames that cover the source span of outputs st .. st + L - 1, counted from the frame boundaries."""
        valid = min(max(self.T_R - st, 0), L)
        if valid == 0:
            return 0
        lo, hi = self.span(st, valid)
        return sum(1 for a, b in zip(self.bounds[:-1], self.bounds[1:]) if a < hi and b > lo)

    def check(self, got, st, L, what):
        """got [L, C] (a numpy array): window st of this stream at `at`.  Returns valid; .worst keeps the worst |error| / bound seen."""
        valid = min(max(self.T_R - st, 0), L)
        assert np.all(got[valid:].view(np.uint32) == 0), (what, "the window's tail is not zeros")
        if self.rate == self.at:
            assert np.array_equal(got[:valid], self.x[st:st + valid]), what
        elif valid:
            self.worst = max(self.worst, sr.assert_close(got[:valid], self.x, self.rate, self.at, np.arange(st, st + valid), what))
        return valid


SHAPES = dict(a44=(8, 2, 256, 16, 44100, 77), b48=(8, 2, 256, 16, 48000, 0), c16=(8, 2, 256, 16, 16000, 0), m44=(6, 1, 192, 24, 44100, 0))


@pytest.fixture(scope="module")
def cases(ctx):
    rng = np.random.default_rng(2025)
    return {name: Case(ctx, *_stream(rng, *shape)) for name, shape in SHAPES.items()}


def _starts(c, L):
    """0, round every frame boundary mapped to the output rate, across the stream's end, at it and behind it."""
    o, n, _ = cx.resample_pair(c.rate, c.at)
    st = {0, c.T_R - L // 2, c.T_R - 1, c.T_R, c.T_R + 5}
    for b in c.bounds:
        st |= {b * n // o + d for d in (-1, 0, 1)}
    return sorted(s for s in st if s >= 0)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gpu_windows_at_16k(cases, name):
    c = cases[name]
    assert c.set.lengths_at(R).tolist() == [-(-c.T * cx.resample_pair(c.rate, R)[1] // cx.resample_pair(c.rate, R)[0])] == [c.T_R]
    assert c.set.lengths_at(R).dtype == torch.int64
    for L in (100, c.T_R + 10):                              # (the second: one window over the whole stream and 10 zeros)
        starts = _starts(c, L) if L == 100 else [0]
        n0 = c.set.frames_decoded
        tc, v1 = c.set.read([0] * len(starts), starts, L, sample_rate=R)
        assert c.set.frames_decoded - n0 == sum(c.frames_for(s, L) for s in starts)
        ct, v2 = c.set.read([0] * len(starts), starts, L, layout="ct", sample_rate=R)
        assert tc.shape == (len(starts), L, c.C) and ct.shape == (len(starts), c.C, L) and tc.is_contiguous() and ct.is_contiguous()
        assert tc.dtype == ct.dtype == torch.float32 and tc.is_cuda and ct.is_cuda and v1.dtype == torch.int64
        want_valid = [min(max(c.T_R - s, 0), L) for s in starts]
        assert v1.tolist() == want_valid and v2.tolist() == want_valid
        tc_h, ct_h = tc.cpu().numpy(), ct.cpu().numpy()
        for k, s in enumerate(starts):
            c.check(tc_h[k], s, L, (name, "tc", s, L))
            c.check(np.ascontiguousarray(ct_h[k].T), s, L, (name, "ct", s, L))
    if L > 100:
        assert c.frames_for(0, L) == len(c.bounds) - 1


def test_gpu_the_target_rate_itself_is_read_as_ever(cases):
    c = cases["c16"]
    starts = _starts(c, 100)
    for layout in ("tc", "ct"):
        n0 = c.set.frames_decoded
        plain, v0 = c.set.read([0] * len(starts), starts, 100, layout=layout)
        n1 = c.set.frames_decoded
        got, v1 = c.set.read([0] * len(starts), starts, 100, layout=layout, sample_rate=R)
        assert torch.equal(got, plain) and torch.equal(v0, v1) and c.set.frames_decoded - n1 == n1 - n0


def test_gpu_one_call_three_rates(ctx, cases):
    """The three stereo streams in one set, windows of all of them in one call: one dense batch."""
    names = ("a44", "b48", "c16")
    s = cx.open_streams(ctx, [cases[n].data for n in names])
    assert s.sample_rates == [44100, 48000, 16000] and s.lengths_at(R).tolist() == [cases[n].T_R for n in names]
    rng = np.random.default_rng(12)
    sid = np.concatenate([np.arange(3), rng.integers(0, 3, size=21)])
    starts = np.array([int(rng.integers(0, cases[names[i]].T_R + 20)) for i in sid])
    starts[:3] = 0
    L = 150
    for layout in ("tc", "ct"):
        n0 = s.frames_decoded
        out, valid = s.read(sid, starts, L, layout=layout, sample_rate=R)
        assert out.shape == ((24, L, 2) if layout == "tc" else (24, 2, L)) and out.is_contiguous()
        assert s.frames_decoded - n0 == sum(cases[names[i]].frames_for(st, L) for i, st in zip(sid.tolist(), starts.tolist()))
        h = out.cpu().numpy()
        for k, (i, st) in enumerate(zip(sid.tolist(), starts.tolist())):
            got = h[k] if layout == "tc" else np.ascontiguousarray(h[k].T)
            assert int(valid[k]) == cases[names[i]].check(got, st, L, (layout, k, names[i], st))
    k16 = np.nonzero(sid == 2)[0]
    plain, _ = s.read(sid[k16], starts[k16], L)
    assert torch.equal(out.transpose(1, 2)[torch.from_numpy(k16).to(out.device)], plain)
    s.close()


def test_gpu_raw_resample_windows(ctx):
    """clx_resample_windows itself on a random device buffer: three rate pairs and a copy in one call, spans at odd float offsets,
    both layouts; then once more on a non-default torch stream."""
    rng = np.random.default_rng(21)
    C, L, T = 2, 1030, 3000                                  # (L: one tile of 1024 outputs and a few)
    rates = (44100, 48000, 8000, R)
    xs = [rng.uniform(-1, 1, size=(T, C)).astype(np.float32) for _ in rates]
    src = torch.from_numpy(np.concatenate([np.zeros(3, np.float32)] + [x.reshape(-1) for x in xs])).to("cuda:0")
    first, t0, sn, o0, valid, fs, which = [], [], [], [], [], [], []
    for i, (rate, x) in enumerate(zip(rates, xs)):
        T_R = T if rate == R else sr.length_at(T, rate, R)
        for st in (0, T_R // 3, T_R - 400, T_R):
            v = min(max(T_R - st, 0), L)
            lo, hi = (0, 0) if v == 0 else (st, st + v) if rate == R else sr.span(st, st + v - 1, T, rate, R)
            first.append(3 + i * T * C + lo * C); t0.append(lo); sn.append(hi - lo); o0.append(st); valid.append(v); fs.append(rate)
            which.append(i)
    B = len(first)

    def check(out, layout):
        h = out.cpu().numpy()
        for k in range(B):
            got = h[k] if layout == cx.WINDOW_TC else np.ascontiguousarray(h[k].T)
            assert np.all(got[valid[k]:].view(np.uint32) == 0)
            if fs[k] == R:
                assert np.array_equal(got[:valid[k]], xs[which[k]][o0[k]:o0[k] + valid[k]])
            elif valid[k]:
                sr.assert_close(got[:valid[k]], xs[which[k]], fs[k], R, np.arange(o0[k], o0[k] + valid[k]), (layout, k))

    torch.cuda.synchronize()
    for layout, shape in ((cx.WINDOW_TC, (B, L, C)), (cx.WINDOW_CT, (B, C, L))):
        out = torch.full(shape, float("nan"), device="cuda:0")
        ctx.resample_windows(src, first, t0, sn, o0, valid, fs, R, L, C, layout, out)
        torch.cuda.synchronize()
        check(out, layout)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        out = torch.full((B, C, L), float("nan"), device="cuda:0")
        ctx.resample_windows(src, first, t0, sn, o0, valid, fs, R, L, C, cx.WINDOW_CT, out)      # (queued on `side`, the current stream here)
        again = out.clone()
    side.synchronize()
    check(again, cx.WINDOW_CT)
    for change, why in ((dict(C=9), "channels"), (dict(R=16001), "table"), (dict(R=0), "rate"), (dict(layout=5), "layout")):
        a = dict(dict(C=C, R=R, layout=cx.WINDOW_TC), **change)
        with pytest.raises(cx.ClaxonError) as e:
            ctx.resample_windows(src, first, t0, sn, o0, valid, fs, a["R"], L, a["C"], a["layout"], out)
        assert e.value.status == cx.API_ERROR and why in e.value.message


def test_gpu_refusals(ctx, cases):
    a, m = cases["a44"], cases["m44"]
    s = cx.open_streams(ctx, [a.data, m.data, b"not a FLAC stream at all"])
    for bad in (0, -16000, 1 << 20, 1 << 40, 16000.5):
        with pytest.raises(ValueError):
            s.read([0], [0], 16, sample_rate=bad)
        with pytest.raises(ValueError):
            s.lengths_at(bad)
    with pytest.raises(ValueError) as e:
        s.read([0], [0], 16, sample_rate=16001)              # (a table of 16001 x 34 entries)
    assert "table" in str(e.value)
    with pytest.raises(ValueError):
        s.lengths_at(16001)
    # every refusal of read() without sample_rate stays
    with pytest.raises(ValueError):
        s.read([0, 1], [0, 0], 16, sample_rate=R)           # mixed channel counts
    with pytest.raises(ValueError):
        s.read([0], [-1], 16, sample_rate=R)
    with pytest.raises(ValueError):
        s.read([0], [0], -1, sample_rate=R)
    with pytest.raises(ValueError):
        s.read([0], [0], 16, layout="lc", sample_rate=R)
    with pytest.raises(ValueError):
        s.read([3], [0], 16, sample_rate=R)
    with pytest.raises(cx.ClaxonError) as e:
        s.read([2], [0], 16, sample_rate=R)
    assert e.value is s.problems[2]
    assert s.lengths_at(R).tolist() == [a.T_R, m.T_R, 0]
    out, valid = s.read([1], [10], 16, sample_rate=R)       # (the good streams of the set read as ever)
    assert valid.tolist() == [16]
    m.check(out[0].cpu().numpy(), 10, 16, "mono")
    out, valid = s.read([], [], 16, layout="ct", sample_rate=R)
    assert out.shape[0] == 0 and out.shape[2] == 16 and valid.shape == (0,)
    out, valid = s.read([0, 0], [0, 5], 0, sample_rate=R)
    assert out.shape == (2, 0, 2) and valid.tolist() == [0, 0]
    out, valid = s.read([0], [1 << 50], 8, sample_rate=R)   # (far behind the end: zeros, nothing decoded)
    assert valid.tolist() == [0] and not bool(out.any())
