"""Mel features on the GPU: Context.mel_windows on audio from load(), and StreamSet.read_mel over five synthetic streams (mono and
stereo at 16, 44.1 and 48 kHz, 1 to 1.1 s long) plus one that is no FLAC stream.  Power mode is held to the definition in float64
under the derived bound (simlib_mel.reference: |M - M64| <= dM per cell, any summation order); a log mode to float64
log(max(float64(M), floor)) of the power output of the same call shape within LOG_ULPS -- the modes share M bitwise; read_mel to
mel_windows on what read() gives, bit for bit."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_mel as sm
from test_gpu_mix import _stream

pytestmark = pytest.mark.gpu
R = 16000
T = 37
FLOOR = 1e-10
# name: (frames, channels, block size, bits, rate, samples of a last short frame)
SHAPES = dict(m16=(64, 1, 256, 16, 16000, 0), s16=(18, 2, 1024, 16, 16000, 0), m44=(44, 1, 1024, 24, 44100, 0),
              s48=(48, 2, 1024, 16, 48000, 0), s44=(46, 2, 1024, 16, 44100, 77))
NAMES = tuple(SHAPES)
SPECS = ((400, 160, 80), (50, 7, 5))


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


@pytest.fixture(scope="module")
def shard(ctx):
    rng = np.random.default_rng(410)
    made = [_stream(rng, *SHAPES[name]) for name in NAMES]
    s = cx.open_streams(ctx, [m[0] for m in made] + [b"not a FLAC stream at all"])
    assert s.problems[:5] == [None] * 5 and isinstance(s.problems[5], cx.ClaxonError)
    assert s.channels[:5] == [1, 2, 1, 2, 2] and s.sample_rates[:5] == [16000, 16000, 44100, 48000, 44100]
    x, rate = cx.load(ctx, made[0][0])                      # the 16 kHz mono stream, whole: [T, 1]
    assert rate == R and x.shape == (64 * 256, 1)
    return s, x[:, 0].contiguous()


def _native_batch(x, L):
    """Five windows of x cut by hand: from its start, inside, ending on its last sample, across its end and behind it."""
    n = x.numel()
    starts = [0, 5000, n - L, n - L + L // 3, n + 9]
    a = torch.zeros((5, L), dtype=torch.float32, device=x.device)
    valid = []
    for k, st in enumerate(starts):
        v = min(max(n - st, 0), L)
        a[k, :v] = x[st:st + v]
        valid.append(v)
    assert valid[2] == L and 0 < valid[3] < L and valid[4] == 0
    return a, np.array(valid, dtype=np.uint32)


@pytest.fixture(scope="module")
def native(shard):
    """Per spec shape: the batch, its valid and the float64 reference (computed once, shared by the layouts and modes)."""
    out = {}
    for N, H, n_mels in SPECS:
        a, valid = _native_batch(shard[1], (T - 1) * H + N)
        w, fb = sm.hann(N), sm.triangles(R, N, n_mels)
        out[N] = (a, valid, sm.reference(a.cpu().numpy(), w, fb, N, H, T))
    return out


def _as_btm(out, layout):
    o = out.cpu().numpy()
    return o.transpose(0, 2, 1) if layout == "ct" else o


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("N,H,n_mels", SPECS)
def test_mel_windows_on_native_audio(ctx, native, N, H, n_mels, layout):
    a, valid, (M64, dM) = native[N]
    vf = sm.valid_frames(valid, H, T)
    assert vf[2] == T and 0 < vf[3] < T and vf[4] == 0
    shape = (5, n_mels, T) if layout == "ct" else (5, T, n_mels)
    got = {}
    for mode in ("power", "ln", "log10"):
        spec = cx.MelSpec(ctx, R, n_fft=N, hop=H, n_mels=n_mels, mode=mode, floor=FLOOR)
        assert np.array_equal(spec.fbank, sm.triangles(R, N, n_mels)) and np.array_equal(spec.window, sm.hann(N))
        out = torch.full(shape, float("nan"), dtype=torch.float32, device=a.device)
        torch.cuda.synchronize()                             # (the fill first: on torch's default stream the launch goes to the context's own)
        ctx.mel_windows(spec, a, valid, T, cx._LAYOUTS[layout], out)
        torch.cuda.synchronize()
        got[mode] = _as_btm(out, layout)
        spec.close()
    worst = 0.0
    for k in range(5):
        for mode in got:
            assert np.all(got[mode][k, vf[k]:].view(np.uint32) == 0), (mode, k, "a frame past valid_frames is not the word 0")
        live = got["power"][k, :vf[k]].astype(np.float64)
        err = np.abs(live - M64[k, :vf[k]])
        assert np.all(err <= dM[k, :vf[k]]), (N, layout, k, float(np.max(err / np.where(dM[k, :vf[k]] > 0, dM[k, :vf[k]], 1.0))))
        if vf[k]:
            worst = max(worst, float(np.max(err / np.where(dM[k, :vf[k]] > 0, dM[k, :vf[k]], 1.0))))
    print("n_fft %d, layout %s: worst |error| / bound %.4f" % (N, layout, worst))
    for mode in ("ln", "log10"):
        ulps = np.concatenate([sm.log_ulps(got[mode][k, :vf[k]], got["power"][k, :vf[k]], sm.MODES[mode], FLOOR).reshape(-1) for k in range(5)])
        print("n_fft %d, layout %s, %s: worst error %.3f ulp" % (N, layout, mode, float(ulps.max())))
        assert np.all(ulps <= sm.LOG_ULPS), (N, layout, mode, float(ulps.max()))


def test_an_all_zero_window_and_the_empty_calls(ctx):
    N, H, n_mels = 64, 24, 13
    a = torch.zeros((2, 4 * H + N), dtype=torch.float32, device="cuda:0")
    valid = [a.shape[1], a.shape[1]]
    for mode in ("power", "ln", "log10"):
        spec = cx.MelSpec(ctx, R, n_fft=N, hop=H, n_mels=n_mels, mode=mode, floor=FLOOR)
        out = torch.full((2, 5, n_mels), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()                             # (the fill first, as above)
        ctx.mel_windows(spec, a, valid, 5, cx.WINDOW_TC, out)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        if mode == "power":
            assert np.all(o.view(np.uint32) == 0)
        else:
            assert np.all(sm.log_ulps(o, np.zeros_like(o), sm.MODES[mode], FLOOR) <= sm.LOG_ULPS)
        out.fill_(7.0)
        torch.cuda.synchronize()
        ctx.mel_windows(spec, a, valid, 0, cx.WINDOW_TC, out)                           # no frame, no window: nothing is written
        ctx.mel_windows(spec, a[:0], [], 5, cx.WINDOW_TC, out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
        with pytest.raises(cx.ClaxonError) as e:
            ctx.mel_windows(spec, a, valid, 6, cx.WINDOW_TC, out)
        assert "window_len" in e.value.message
        with pytest.raises(cx.ClaxonError) as e:
            ctx.mel_windows(spec, a, [a.shape[1] + 1, 0], 5, cx.WINDOW_TC, out)
        assert "valid" in e.value.message
        spec.close()
        with pytest.raises(ValueError):
            ctx.mel_windows(spec, a, valid, 5, cx.WINDOW_TC, out)                        # (a closed spec)


def _calls(shard):
    """(stream ids, starts at 16 kHz): every stream from its start and across its end (the stream ends 500 or more samples before
    the window does, inside its last frames: valid_frames < n_frames), and one window wholly behind its stream."""
    s = shard[0]
    len16 = s.lengths_at(R).tolist()
    L = (T - 1) * 160 + 400
    sid = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 2]
    st = [0, 3, 1000, 77, 5000] + [len16[i] - L + 500 + 300 * i for i in range(5)] + [len16[2] + 4]
    return sid, st


@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_read_mel_is_read_then_mel_windows(ctx, shard, layout):
    s = shard[0]
    spec = cx.MelSpec(ctx, R, mode="ln", floor=FLOOR)        # 400 / 160 / 80
    sid, st = _calls(shard)
    L = spec.window_len(T)
    n0 = s.frames_decoded
    audio, valid = s.read(sid, st, L, "ct", sample_rate=R, channels=1)
    n1 = s.frames_decoded
    want = torch.empty((len(sid), 80, T) if layout == "ct" else (len(sid), T, 80), dtype=torch.float32, device=audio.device)
    ctx.mel_windows(spec, audio.view(len(sid), L), valid.numpy(), T, cx._LAYOUTS[layout], want)
    got, vf = s.read_mel(sid, st, T, spec, layout=layout)
    torch.cuda.synchronize()
    assert s.frames_decoded - n1 == n1 - n0 > 0
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert vf.dtype == torch.int64 and vf.tolist() == sm.valid_frames(valid.numpy(), 160, T).tolist()
    assert 0 < vf[5] < T and vf[-1] == 0 and vf[0] == T
    g = got if layout == "tc" else got.transpose(1, 2)
    for k in range(len(sid)):
        assert bool((g[k, int(vf[k]):].view(torch.int32) == 0).all()) and bool(torch.isfinite(g[k]).all())
    # the same refusals as read(): a problem stream, a negative start, an unknown stream, a bad layout -- and its own
    with pytest.raises(cx.ClaxonError) as e:
        s.read_mel([0, 5], [0, 0], T, spec, layout=layout)
    assert e.value is s.problems[5]
    for bad in (dict(stream_ids=[0], starts=[-1]), dict(stream_ids=[6], starts=[0]), dict(stream_ids=[0, 1], starts=[0])):
        with pytest.raises(ValueError):
            s.read_mel(n_frames=T, spec=spec, layout=layout, **bad)
    with pytest.raises(ValueError):
        s.read_mel([0], [0], T, spec, layout="lc")
    with pytest.raises(ValueError):
        s.read_mel([0], [0], -1, spec)
    empty, vf0 = s.read_mel([], [], T, spec, layout=layout)
    assert empty.numel() == 0 and vf0.numel() == 0
    none, vf0 = s.read_mel([0, 1], [0, 0], 0, spec, layout=layout)
    assert none.numel() == 0 and vf0.tolist() == [0, 0]
    spec.close()
    with pytest.raises(ValueError):
        s.read_mel(sid, st, T, spec)


def test_a_second_spec_on_the_same_context(ctx, shard):
    """n_fft 64 beside n_fft 400, calls interleaved: each gives what it gives alone (the tables are the spec's, not the context's)."""
    s = shard[0]
    sid, st = [0, 1, 4], [100, 2000, 9000]

    def alone(**kw):
        spec = cx.MelSpec(ctx, R, **kw)
        out = s.read_mel(sid, st, T, spec)[0]
        torch.cuda.synchronize()
        spec.close()
        return out

    kw_a, kw_b = dict(mode="ln"), dict(n_fft=64, hop=24, n_mels=13, mode="log10")
    want_a, want_b = alone(**kw_a), alone(**kw_b)
    a, b = cx.MelSpec(ctx, R, **kw_a), cx.MelSpec(ctx, R, **kw_b)
    def both():
        ga, gb = s.read_mel(sid, st, T, a)[0], s.read_mel(sid, st, T, b)[0]
        torch.cuda.synchronize()
        return ga, gb

    for _ in range(2):
        ga, gb = both()
        assert torch.equal(ga, want_a) and torch.equal(gb, want_b)
    b.close()
    ga = s.read_mel(sid, st, T, a)[0]
    torch.cuda.synchronize()
    assert torch.equal(ga, want_a)
    a.close()
    assert want_a.shape == (3, 80, T) and want_b.shape == (3, 13, T)
