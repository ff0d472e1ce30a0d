"""Framed mel specs -- Kaldi's fbank -- on the GPU: the three plain equalities and the conditioning equality of test_melk_sim.py on
load()'s 16-bit audio, word for word; the conditioned kernel on a 24-bit stream under the derived bound of the float64 reference
(simlib_melk.reference); StreamSet.read_mel with MelSpec.kaldi over test_gpu_mel's five synthetic streams, bit-equal to read +
mel_windows, with valid_frames by the whole-frame rule and inside the float64 intervals; and a Kaldi, a Whisper and a plain spec side
by side on one context."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_mel as sm
import simlib_melk as sk
from gpu_guarded import device_out, written
from test_gpu_mel import NAMES, SHAPES, _native_batch
from test_gpu_melc import _calls
from test_gpu_mix import _stream

pytestmark = pytest.mark.gpu
R = 16000
T = 37
FLOOR = 1e-10
SPECS = ((400, 512, 160, 80, 256), (25, 32, 10, 5, 16))     # (Nw, N, H, n_mels, n_bins)
CONDS = ((True, 0.0), (False, 0.97), (True, 0.97))


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


@pytest.fixture(scope="module")
def shard(ctx):
    rng = np.random.default_rng(412)
    made = [_stream(rng, *SHAPES[name]) for name in NAMES]
    s = cx.open_streams(ctx, [m[0] for m in made] + [b"not a FLAC stream at all"])
    assert s.problems[:5] == [None] * 5 and isinstance(s.problems[5], cx.ClaxonError)
    x, rate = cx.load(ctx, made[0][0])                      # the 16 kHz mono 16-bit stream, whole: [T, 1]
    assert rate == R and x.shape == (64 * 256, 1)
    y, rate = cx.load(ctx, made[2][0])                      # the 44.1 kHz mono 24-bit stream
    assert rate == 44100 and y.shape[1] == 1 and SHAPES["m44"][3] == 24
    return s, x[:, 0].contiguous(), y[:, 0].contiguous()


def _btm(out, layout):
    o = out.cpu().numpy()
    return o.transpose(0, 2, 1) if layout == "ct" else o


def _mel(ctx, spec, a, valid, layout, n_frames=T):
    """mel_windows into a guarded slice: [B, n_frames, n_mels] on the host, after the guards' and the fill's checks."""
    B, n = int(a.shape[0]), int(a.shape[0]) * spec.n_mels * n_frames
    flat, out = device_out(n, offset_words=1)
    torch.cuda.synchronize()                                 # (the fill first: on torch's default stream the launch goes to the context's own)
    ctx.mel_windows(spec, a, valid, n_frames, cx._LAYOUTS[layout], out.view((B, spec.n_mels, n_frames) if layout == "ct" else (B, n_frames, spec.n_mels)))
    torch.cuda.synchronize()
    o = written(flat, n, (spec.win_length, spec.n_fft, spec.hop, spec.n_mels, layout), offset_words=1).view(np.float32)
    return o.reshape(B, spec.n_mels, n_frames).transpose(0, 2, 1) if layout == "ct" else o.reshape(B, n_frames, spec.n_mels)


def _tables(Nw, N, n_mels, n_bins):
    w = cx.mel_window_kaldi("povey", Nw, 32768.0)
    fb = cx.mel_fbank_kaldi(R, N, n_mels)
    assert fb.shape == (n_mels, n_bins) and np.array_equal(w, (sk.kaldi_window("povey", Nw) * 32768.0).astype(np.float32))
    return w, fb


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins", SPECS)
def test_plain_equalities(ctx, shard, Nw, N, H, n_mels, n_bins, layout):
    """(i) zero options, Nw == N, all bins: MelSpec's words.  (ii) Nw < N: the window zero-padded to N, power mode.  (iii) a bank over
    n_bins bins: the bank with zero columns from there on.  The padded counterparts of (ii) and (iii) are framed specs of the shape
    that (i) ties to clx_mel_create's."""
    J = N // 2 + 1
    a, valid = _native_batch(shard[1], (T - 1) * H + N)
    w, fb = _tables(Nw, N, n_mels, n_bins)
    wpad = np.concatenate([w, np.zeros(N - Nw, np.float32)])
    fbz = np.concatenate([fb, np.zeros((n_mels, J - n_bins), np.float32)], axis=1)
    for mode in ("power", "ln", "log10"):
        plain = cx.MelSpec(ctx, R, n_fft=N, hop=H, n_mels=n_mels, mode=mode, floor=FLOOR)
        pairs = [(plain, cx.MelSpec.framed(ctx, R, N, N, H, plain.window, plain.fbank, mode=mode, floor=FLOOR)),
                 (cx.MelSpec.framed(ctx, R, N, N, H, plain.window, fbz, mode=mode, floor=FLOOR),
                  cx.MelSpec.framed(ctx, R, N, N, H, plain.window, fb, mode=mode, floor=FLOOR))]
        if mode == "power":
            pairs.append((cx.MelSpec.framed(ctx, R, N, N, H, wpad, plain.fbank, mode=mode), cx.MelSpec.framed(ctx, R, N, Nw, H, w, plain.fbank, mode=mode)))
        for i, (p, f) in enumerate(pairs):
            vf = f.valid_frames(valid, T)
            assert vf.tolist() == sm.valid_frames(valid, H, T).tolist() and 0 < vf[3] < T and vf[4] == 0
            got = _mel(ctx, f, a, valid, layout)
            assert _same(got, _mel(ctx, p, a, valid, layout)), (i, mode, layout)
            assert np.all(np.isfinite(got)) and np.any(got[0] != 0)
            p.close()
            f.close()


@pytest.mark.parametrize("dc,c", CONDS)
@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins", SPECS)
def test_conditioning_is_float32_numpy_in_front_of_the_unconditioned_spec(ctx, shard, Nw, N, H, n_mels, n_bins, dc, c):
    """load()'s 16-bit audio lies on the 2^-15 grid, so a frame's sum is exact in any order: the conditioned spec on the batch gives
    the words of the unconditioned framed spec on single frames that numpy conditioned in float32.  Three modes, both layouts."""
    L = (T - 1) * H + Nw
    a, valid = _native_batch(shard[1], L)
    w, fb = _tables(Nw, N, n_mels, n_bins)
    X = sk.frames_of(a.cpu().numpy(), Nw, H, T)              # [5, T, Nw]
    assert np.array_equal(X * 32768.0, np.round(X * 32768.0))
    Y = torch.from_numpy(sk.condition32(X, dc, np.float32(c)).reshape(5 * T, Nw)).to(a.device)
    for mode in ("power", "ln", "log10"):
        h0 = cx.MelSpec.framed(ctx, R, N, Nw, H, w, fb, mode=mode, floor=FLOOR)
        hf = cx.MelSpec.framed(ctx, R, N, Nw, H, w, fb, mode=mode, floor=FLOOR, remove_dc=dc, preemph=c, whole_frames=True)
        vf = hf.valid_frames(valid, T)
        assert vf.tolist() == sk.valid_frames(valid, Nw, H, T, True).tolist() and vf[2] == T and 0 < vf[3] < T and vf[4] == 0
        want = _mel(ctx, h0, Y, np.full(5 * T, Nw, np.uint32), "tc", n_frames=1).reshape(5, T, n_mels).copy()
        for k in range(5):
            want[k, vf[k]:] = 0.0
        for layout in ("ct", "tc"):
            assert _same(_mel(ctx, hf, a, valid, layout), want), (dc, c, mode, layout)
        h0.close()
        hf.close()


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins", SPECS)
def test_a_24_bit_stream_is_within_the_bound(ctx, shard, Nw, N, H, n_mels, n_bins):
    """24-bit samples do not sum exactly: |M - M64| <= dM per live cell for every conditioning, and the log modes within LOG_ULPS of
    the logarithm of the power mode's words."""
    L = (T - 1) * H + Nw
    a, valid = _native_batch(shard[2], L)
    x = a.cpu().numpy()
    assert not np.array_equal(x * 32768.0, np.round(x * 32768.0))
    w, fb = _tables(Nw, N, n_mels, n_bins)
    vf = sk.valid_frames(valid, Nw, H, T, True)
    for dc, c in CONDS:
        M64, dM = sk.reference(x, w, fb, N, H, T, dc, c)
        got = {}
        for mode in ("power", "ln", "log10"):
            spec = cx.MelSpec.framed(ctx, R, N, Nw, H, w, fb, mode=mode, floor=FLOOR, remove_dc=dc, preemph=c, whole_frames=True)
            got[mode] = _mel(ctx, spec, a, valid, "ct")
            spec.close()
        worst = 0.0
        for k in range(5):
            for mode in got:
                assert np.all(got[mode][k, vf[k]:].view(np.uint32) == 0), (mode, k)
            err = np.abs(got["power"][k, :vf[k]].astype(np.float64) - M64[k, :vf[k]])
            assert np.all(err <= dM[k, :vf[k]]), (Nw, dc, c, k)
            if vf[k]:
                worst = max(worst, float(np.max(err / np.where(dM[k, :vf[k]] > 0, dM[k, :vf[k]], 1.0))))
        print("win %d dc %d c %.2f: worst |error| / bound %.4f" % (Nw, dc, c, worst))
        for mode in ("ln", "log10"):
            ulps = np.concatenate([sm.log_ulps(got[mode][k, :vf[k]], got["power"][k, :vf[k]], sm.MODES[mode], FLOOR).reshape(-1) for k in range(5)])
            assert np.all(ulps <= sm.LOG_ULPS), (Nw, dc, c, mode, float(ulps.max()))


@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_read_mel_with_the_kaldi_spec(ctx, shard, layout):
    s = shard[0]
    spec = cx.MelSpec.kaldi(ctx)
    assert (spec.n_fft, spec.win_length, spec.hop, spec.n_mels, spec.n_bins, spec.mode) == (512, 400, 160, 80, 256, "ln")
    assert np.array_equal(spec.fbank, sk.kaldi_fbank(R, 512, 80).astype(np.float32))
    L = spec.window_len(T)
    assert L == 36 * 160 + 400
    sid, st = _calls(s, L)
    len16 = s.lengths_at(R).tolist()
    sid, st = sid + [0, 1], st + [len16[0] - 399, len16[1] - 400]                           # shorter than one frame; exactly one frame
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
    rule = np.where(v < 400, 0, np.minimum(1 + np.maximum(v - 400, 0) // 160, T))
    assert vf.dtype == torch.int64 and vf.tolist() == rule.tolist()
    assert v[-2] == 399 and vf[-2] == 0 and v[-1] == 400 and vf[-1] == 1 and vf[0] == T and 0 < vf[5] < T and vf[10] == 0
    # end to end against the float64 definition: ln is monotone, so the band sums' bound gives an interval
    M64, dM = sk.reference(audio.view(len(sid), L).cpu().numpy(), spec.window, spec.fbank, 512, 160, T, True, spec.preemph)
    lo, hi = np.log(np.maximum(M64 - dM, spec.floor)), np.log(np.maximum(M64 + dM, spec.floor))
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    lo, hi = lo - sm.LOG_ULPS * ulp(lo), hi + sm.LOG_ULPS * ulp(hi)
    g = _btm(got, layout).astype(np.float64)
    for k in range(len(sid)):
        assert np.all(g[k, vf[k]:] == 0) and np.all((lo[k, :vf[k]] <= g[k, :vf[k]]) & (g[k, :vf[k]] <= hi[k, :vf[k]])), k
    print("kaldi intervals: widest %.3g, median %.3g" % (float((hi - lo).max()), float(np.median(hi - lo))))
    # read()'s refusals, and the length rule of a spec that is not centred
    with pytest.raises(cx.ClaxonError) as e:
        s.read_mel([0, 5], [0, 0], T, spec, layout=layout)
    assert e.value is s.problems[5]
    with pytest.raises(ValueError, match="not centred"):
        s.read_mel([0], [0], T, spec, length=L + 1)
    same, _ = s.read_mel(sid, st, T, spec, layout=layout, length=L)
    empty, vf0 = s.read_mel([], [], T, spec, layout=layout)
    none, vf1 = s.read_mel([0, 1], [0, 0], 0, spec, layout=layout)
    torch.cuda.synchronize()
    assert torch.equal(same.view(torch.int32), got.view(torch.int32))
    assert empty.numel() == 0 and vf0.numel() == 0 and none.numel() == 0 and vf1.tolist() == [0, 0]
    spec.close()
    with pytest.raises(ValueError):
        s.read_mel(sid, st, T, spec)


def test_a_kaldi_a_whisper_and_a_plain_spec_side_by_side(ctx, shard):
    """Calls interleaved on one context: each spec gives what it gives alone (the shared table and its two events hold)."""
    s = shard[0]
    sid, st = [0, 1, 4, 2], [100, 2000, 9000, 16000]
    makers = (lambda: cx.MelSpec.kaldi(ctx), lambda: cx.MelSpec.whisper(ctx), lambda: cx.MelSpec(ctx, R, n_fft=64, hop=24, n_mels=13, mode="log10"))

    def alone(make):
        spec = make()
        out = s.read_mel(sid, st, T, spec)[0]
        torch.cuda.synchronize()
        spec.close()
        return out

    want = [alone(m) for m in makers]
    assert not torch.equal(want[0], alone(lambda: cx.MelSpec.kaldi(ctx, remove_dc_offset=False)))
    specs = [m() for m in makers]
    for _ in range(2):
        got = [s.read_mel(sid, st, T, spec)[0] for spec in specs]
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    for spec in specs:
        spec.close()
