"""Centred frames and range scaling on the GPU: Context.mel_windows with centred specs against the existing kernel on the batch padded
on the host, word for word; a ranged spec against float32 numpy on the unranged output of the same device, word for word; and
StreamSet.read_mel with MelSpec.whisper over test_gpu_mel's five synthetic streams (mono and stereo at 16, 44.1 and 48 kHz) plus
one that is no FLAC stream: bit-equal to read + mel_windows, and held end to end to the float64 Whisper formula by interval
arithmetic (simlib_mel.reference's bound, LOG_ULPS for the log, one ulp for each rounded operation behind it)."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_mel as sm
from gpu_guarded import device_out, written
from test_gpu_mel import NAMES, SHAPES, _native_batch
from test_gpu_mix import _stream

pytestmark = pytest.mark.gpu
R = 16000
T = 37
FLOOR = 1e-10
SPECS = ((400, 160, 80), (50, 7, 5), (51, 7, 5))
RANGES = ((8.0, 4.0, 0.25), (8.0, 0.0, 10.0))


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


@pytest.fixture(scope="module")
def shard(ctx):
    rng = np.random.default_rng(411)
    made = [_stream(rng, *SHAPES[name]) for name in NAMES]
    s = cx.open_streams(ctx, [m[0] for m in made] + [b"not a FLAC stream at all"])
    assert s.problems[:5] == [None] * 5 and isinstance(s.problems[5], cx.ClaxonError)
    x, rate = cx.load(ctx, made[0][0])                      # the 16 kHz mono stream, whole: [T, 1]
    assert rate == R and x.shape == (64 * 256, 1)
    return s, x[:, 0].contiguous()


def _btm(out, layout):
    o = out.cpu().numpy()
    return o.transpose(0, 2, 1) if layout == "ct" else o


def _mel(ctx, spec, a, valid, layout):
    """mel_windows into a guarded slice: [B, T, n_mels] on the host, after the guards' and the fill's checks."""
    B, n = int(a.shape[0]), int(a.shape[0]) * spec.n_mels * T
    flat, out = device_out(n, offset_words=1)
    torch.cuda.synchronize()                                 # (the fill first: on torch's default stream the launch goes to the context's own)
    ctx.mel_windows(spec, a, valid, T, cx._LAYOUTS[layout], out.view((B, spec.n_mels, T) if layout == "ct" else (B, T, spec.n_mels)))
    torch.cuda.synchronize()
    o = written(flat, n, (spec.n_fft, spec.hop, spec.n_mels, layout), offset_words=1).view(np.float32)
    return o.reshape(B, spec.n_mels, T).transpose(0, 2, 1) if layout == "ct" else o.reshape(B, T, spec.n_mels)


@pytest.mark.parametrize("pad_mode", ("reflect", "zeros"))
@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("N,H,n_mels", SPECS)
def test_centred_is_the_existing_kernel_on_the_padded_batch(ctx, shard, N, H, n_mels, layout, pad_mode):
    """Five windows of load()'s audio, L = T * H: from the start, inside, ending on the last sample, across the end, behind it."""
    P = N // 2
    a, valid = _native_batch(shard[1], T * H)
    ap = np.pad(a.cpu().numpy(), ((0, 0), (P, P)), mode="reflect" if pad_mode == "reflect" else "constant")
    vp = np.where(valid > 0, valid + P, 0).astype(np.uint32)
    for mode in ("power", "ln"):
        plain = cx.MelSpec(ctx, R, n_fft=N, hop=H, n_mels=n_mels, mode=mode, floor=FLOOR)
        centred = cx.MelSpec(ctx, R, n_fft=N, hop=H, n_mels=n_mels, mode=mode, floor=FLOOR, center=True, pad_mode=pad_mode)
        vf = centred.valid_frames(valid, T)
        assert vf.tolist() == plain.valid_frames(vp, T).tolist() and vf[2] == T and 0 < vf[3] < T and vf[4] == 0
        want = _mel(ctx, plain, torch.from_numpy(ap).to(a.device), vp, layout)
        got = _mel(ctx, centred, a, valid, layout)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, layout, pad_mode, mode)
        for k in range(5):
            assert np.all(got[k, vf[k]:].view(np.uint32) == 0) and np.all(np.isfinite(got[k]))
        plain.close()
        centred.close()


@pytest.mark.parametrize("mode", ("ln", "log10"))
@pytest.mark.parametrize("N,H,n_mels", SPECS[:2])
def test_ranged_is_float32_numpy_on_the_unranged_output(ctx, shard, N, H, n_mels, mode):
    """The five windows and a sixth of zeros that is live to its end (its cells are the device's finish(0): the silence value)."""
    a5, v5 = _native_batch(shard[1], T * H)
    a = torch.cat([a5, torch.zeros_like(a5[:1])])
    valid = np.concatenate([v5, [T * H]]).astype(np.uint32)
    kw = dict(n_fft=N, hop=H, n_mels=n_mels, mode=mode, floor=FLOOR, center=True)
    plain = cx.MelSpec(ctx, R, **kw)
    vf = plain.valid_frames(valid, T)
    for layout in ("ct", "tc"):
        u = _mel(ctx, plain, a, valid, layout).copy()
        y0 = u[5, 0, 0]
        assert np.all(u[5].view(np.uint32) == y0.view(np.uint32)) and abs(float(y0) - (np.log(FLOOR) if mode == "ln" else -10.0)) < 1e-4
        for k in range(6):
            u[k, vf[k]:] = y0
        mx = u.reshape(6, -1).max(axis=1)
        for D, shift, scale in RANGES:
            lo = (mx - np.float32(D)).astype(np.float32)
            want = ((np.maximum(u, lo[:, None, None]) + np.float32(shift)).astype(np.float32) * np.float32(scale)).astype(np.float32)
            ranged = cx.MelSpec(ctx, R, top=D, shift=shift, scale=scale, **kw)
            got = _mel(ctx, ranged, a, valid, layout)
            ranged.close()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, mode, layout, D, shift, scale)
            silence = np.float32(np.float32(np.maximum(y0, lo[3]) + np.float32(shift)) * np.float32(scale))
            assert 0 < vf[3] < T and np.all(got[3, vf[3]:].view(np.uint32) == silence.view(np.uint32)), "a dead frame is not the scaled silence value"
            assert vf[4] == 0 and np.all(got[4].view(np.uint32) == got[4, 0, 0].view(np.uint32)), "the window behind its stream is not uniform"
    plain.close()


def _calls(s, L):
    """(stream ids, starts at 16 kHz): every stream from near its start and across its end, and one window wholly behind its stream."""
    len16 = s.lengths_at(R).tolist()
    sid = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 2]
    st = [0, 3, 1000, 77, 5000] + [len16[i] - L + 500 + 300 * i for i in range(5)] + [len16[2] + 4]
    return sid, st


def _ulp(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _whisper_intervals(audio, valid, spec):
    """[lo, hi] per cell ([B, T, n_mels], float64) of the Whisper formula on `audio` [B, L] (float32): the float64 band sums +- the
    bound, log10 (monotone) widened by LOG_ULPS ulps, the window's maximum, - 8, the clamp, + 4, * 0.25 -- all monotone, each
    rounded operation widened by one ulp of the larger end."""
    N, H, P = spec.n_fft, spec.hop, spec.n_fft // 2
    M64, dM = sm.reference(np.pad(audio, ((0, 0), (P, P)), mode="reflect"), spec.window, spec.fbank, N, H, T)
    lo, hi = np.log10(np.maximum(M64 - dM, spec.floor)), np.log10(np.maximum(M64 + dM, spec.floor))
    vf = spec.valid_frames(valid, T)
    for k in range(audio.shape[0]):
        lo[k, vf[k]:] = hi[k, vf[k]:] = np.log10(spec.floor)
    lo, hi = lo - sm.LOG_ULPS * _ulp(lo), hi + sm.LOG_ULPS * _ulp(hi)

    def widen(a, b):
        u = np.maximum(_ulp(a), _ulp(b))
        return a - u, b + u

    mlo, mhi = lo.reshape(lo.shape[0], -1).max(axis=1), hi.reshape(hi.shape[0], -1).max(axis=1)
    clo, chi = widen(mlo - spec.top, mhi - spec.top)
    lo, hi = np.maximum(lo, clo[:, None, None]), np.maximum(hi, chi[:, None, None])
    lo, hi = widen(lo + spec.shift, hi + spec.shift)
    return widen(lo * spec.scale, hi * spec.scale)


@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_read_mel_with_the_whisper_spec(ctx, shard, layout):
    s = shard[0]
    spec = cx.MelSpec.whisper(ctx)
    assert (spec.n_fft, spec.hop, spec.n_mels, spec.mode, spec.center, spec.top, spec.shift, spec.scale) == (400, 160, 80, "log10", True, 8.0, 4.0, 0.25)
    assert np.array_equal(spec.fbank, sm.triangles(R, 400, 80, 0.0, 8000.0, "slaney", True)) and spec.window_len(3000) == 480000
    L = spec.window_len(T)
    assert L == T * 160
    sid, st = _calls(s, L)
    n0 = s.frames_decoded
    audio, valid = s.read(sid, st, L, "ct", sample_rate=R, channels=1)
    n1 = s.frames_decoded
    want = torch.empty((len(sid), 80, T) if layout == "ct" else (len(sid), T, 80), dtype=torch.float32, device=audio.device)
    ctx.mel_windows(spec, audio.view(len(sid), L), valid.numpy(), T, cx._LAYOUTS[layout], want)
    got, vf = s.read_mel(sid, st, T, spec, layout=layout)
    torch.cuda.synchronize()
    assert s.frames_decoded - n1 == n1 - n0 > 0
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got.view(torch.int32), want.view(torch.int32))
    v = valid.numpy().astype(np.int64)
    rule = np.where(v == 0, 0, np.minimum((v + 200 + 159) // 160, T))
    assert vf.dtype == torch.int64 and vf.tolist() == rule.tolist() and 0 < vf[5] < T and vf[-1] == 0 and vf[0] == T
    got2, vf2 = s.read_mel(sid, st, T, spec, layout=layout, length=L)                       # the default length, spelled out
    longer, vfl = s.read_mel(sid, st, T, spec, layout=layout, length=L + 123)               # a longer crop: other reflections, same shape
    torch.cuda.synchronize()                                 # (on torch's default stream the launches go to the context's own)
    assert torch.equal(got2.view(torch.int32), got.view(torch.int32)) and torch.equal(vf2, vf)
    assert longer.shape == got.shape and vfl[0] == T
    # end to end against the float64 formula
    lo, hi = _whisper_intervals(audio.view(len(sid), L).cpu().numpy(), v, spec)
    g = _btm(got, layout).astype(np.float64)
    bad = np.argwhere(~((lo <= g) & (g <= hi)))
    assert bad.size == 0, (bad[:4], g[tuple(bad[0])], lo[tuple(bad[0])], hi[tuple(bad[0])])
    print("whisper intervals: widest %.3g, median %.3g" % (float((hi - lo).max()), float(np.median(hi - lo))))
    assert np.all(g[-1] == g[-1, 0, 0]) and np.all(g.max(axis=(1, 2)) - g.min(axis=(1, 2)) <= 2.0 + 1e-6)      # (8 / 4: the range's width)
    # read()'s refusals, and the new ones of `length`
    with pytest.raises(cx.ClaxonError) as e:
        s.read_mel([0, 5], [0, 0], T, spec, layout=layout)
    assert e.value is s.problems[5]
    for bad in (dict(stream_ids=[0], starts=[-1]), dict(stream_ids=[6], starts=[0]), dict(stream_ids=[0, 1], starts=[0])):
        with pytest.raises(ValueError):
            s.read_mel(n_frames=T, spec=spec, layout=layout, **bad)
    with pytest.raises(ValueError, match="greater than n_fft // 2"):
        s.read_mel([0], [0], 1, spec, length=200)
    with pytest.raises(ValueError, match="centred frames"):
        s.read_mel([0], [0], T, spec, length=(T - 1) * 160 - 1)
    with pytest.raises(ValueError, match="length must be a whole number"):
        s.read_mel([0], [0], T, spec, length=-5)
    one, vf1 = s.read_mel([0], [0], 1, spec, length=201)                                    # P + 1: the shortest crop
    torch.cuda.synchronize()
    assert one.shape == (1, 80, 1) and vf1.tolist() == [1]
    plain = cx.MelSpec(ctx, R, mode="ln")
    with pytest.raises(ValueError, match="not centred"):
        s.read_mel([0], [0], T, plain, length=T * 160)
    a, _ = s.read_mel([0], [0], T, plain, length=plain.window_len(T))
    b, _ = s.read_mel([0], [0], T, plain)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    empty, vf0 = s.read_mel([], [], T, spec, layout=layout)
    assert empty.numel() == 0 and vf0.numel() == 0
    none, vf0 = s.read_mel([0, 1], [0, 0], 0, spec, layout=layout)
    assert none.numel() == 0 and vf0.tolist() == [0, 0]
    plain.close()
    spec.close()
    with pytest.raises(ValueError):
        s.read_mel(sid, st, T, spec)


def test_a_centred_ranged_spec_beside_a_plain_one(ctx, shard):
    """Calls interleaved on one context, then each on a torch stream of its own: each spec gives what it gives alone (the shared
    table -- valid_frames, the load limits, the maxima -- and its two events hold)."""
    s = shard[0]
    sid, st = [0, 1, 4, 2], [100, 2000, 9000, 16000]

    def alone(make):
        spec = make()
        out = s.read_mel(sid, st, T, spec)[0]
        torch.cuda.synchronize()
        spec.close()
        return out

    make_a, make_b = (lambda: cx.MelSpec.whisper(ctx)), (lambda: cx.MelSpec(ctx, R, n_fft=64, hop=24, n_mels=13, mode="log10"))
    want_a, want_b = alone(make_a), alone(make_b)
    assert not torch.equal(want_a, alone(lambda: cx.MelSpec(ctx, R, n_fft=400, hop=160, n_mels=80, f_max=8000.0, mel_scale="slaney", norm="slaney",
                                                              mode="log10", center=True)))
    a, b = make_a(), make_b()
    for _ in range(2):
        ga, gb = s.read_mel(sid, st, T, a)[0], s.read_mel(sid, st, T, b)[0]
        torch.cuda.synchronize()
        assert torch.equal(ga.view(torch.int32), want_a.view(torch.int32)) and torch.equal(gb.view(torch.int32), want_b.view(torch.int32))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):
        with torch.cuda.stream(s1):
            ga = s.read_mel(sid, st, T, a)[0]
        with torch.cuda.stream(s2):
            gb = s.read_mel(sid, st, T, b)[0]
        with torch.cuda.stream(s1):
            ga2 = s.read_mel(sid, st, T, a)[0]
        torch.cuda.synchronize()
        for g, w in ((ga, want_a), (gb, want_b), (ga2, want_a)):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    a.close()
    b.close()
