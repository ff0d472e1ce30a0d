"""Cepstral mel specs -- Kaldi's MFCC -- on the GPU: the cepstrum equality of test_melq_sim.py on load()'s 16-bit audio, word for
word against the chain of the host libm's fmaf over the GPU's own framed-spec output (so that the device's logf cancels); the energy
row within LOG_ULPS of the logarithm of the energy emulated in the stated lane order, and of the exact integer energy where every
sum is exact; StreamSet.read_mel with MelSpec.mfcc, with and without use_energy, over test_gpu_mel's five synthetic streams, bit-equal
to read + mel_windows with valid_frames by the whole-frame rule; every live cell of broadband noise inside the float64 interval of
the MFCC formula (simlib_melq.reference), which is held to be narrow; and an MFCC, a Kaldi fbank and a Whisper spec side by side on
one context.  The outputs of mel_windows are guarded slices (gpu_guarded.py)."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_mel as sm
import simlib_melk as sk
import simlib_melq as sq
from gpu_guarded import device_out, written
from test_gpu_mel import NAMES, SHAPES, _native_batch
from test_gpu_melc import _calls
from test_gpu_mix import _stream
from test_melq_sim import SHAPES as SPECS, _bank, _tables, _window

pytestmark = pytest.mark.gpu
R = 16000
T = 37
EPS = float(np.finfo(np.float32).eps)
PRE = float(np.float32(0.97))
# The width of the MFCC interval that 99 % of the cells must stay within in test_noise_is_inside_the_float64_interval: chosen from
# simlib_melq.reference alone, on the CPU: for the test's three windows the intervals' widths are 0.56 at the median, 1.18 at the 99th
# percentile and 1.42 at most (rows 0..12 at most 0.12, 0.39, 0.60, .. 1.42: the lifter grows to 12.0), where C0 is about 122 and
# the median |C| is 6.6.
WIDTH = 1.5


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


@pytest.fixture(scope="module")
def shard(ctx):
    rng = np.random.default_rng(413)
    made = [_stream(rng, *SHAPES[name]) for name in NAMES]
    s = cx.open_streams(ctx, [m[0] for m in made] + [b"not a FLAC stream at all"])
    assert s.problems[:5] == [None] * 5 and isinstance(s.problems[5], cx.ClaxonError)
    x, rate = cx.load(ctx, made[0][0])                      # the 16 kHz mono 16-bit stream, whole: [T, 1]
    assert rate == R and x.shape == (64 * 256, 1)
    return s, x[:, 0].contiguous()


def _btm(o, layout, B, rows, n_frames):
    o = o.view(np.float32)
    return o.reshape(B, rows, n_frames).transpose(0, 2, 1) if layout == "ct" else o.reshape(B, n_frames, rows)


def _mel(ctx, spec, a, valid, layout, n_frames=T):
    """mel_windows into a guarded slice: [B, n_frames, n_out] on the host, after the guards' and the fill's checks."""
    B, n = int(a.shape[0]), int(a.shape[0]) * spec.n_out * n_frames
    flat, out = device_out(n, offset_words=1)
    torch.cuda.synchronize()                                 # (the fill first: on torch's default stream the launch goes to the context's own)
    ctx.mel_windows(spec, a, valid, n_frames, cx._LAYOUTS[layout], out.view((B, spec.n_out, n_frames) if layout == "ct" else (B, n_frames, spec.n_out)))
    torch.cuda.synchronize()
    return _btm(written(flat, n, (spec.n_out, layout), offset_words=1), layout, B, spec.n_out, n_frames)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _framed(ctx, Nw, N, H, w, fb, mode, **kw):
    return cx.MelSpec.framed(ctx, R, N, Nw, H, w, fb, mode=mode, floor=EPS, remove_dc=True, preemph=PRE, whole_frames=True, **kw)


_WANT = {}


def _want(ctx, shard, shape, mode):
    """Per shape and mode, once: the batch, valid, valid_frames and the libm fmaf chain over the GPU's framed-spec output."""
    if (shape, mode) not in _WANT:
        Nw, N, H, n_mels, n_bins, n_ceps = shape
        a, valid = _native_batch(shard[1], (T - 1) * H + Nw)
        w, fb = _window(Nw), _bank(N, n_mels, n_bins)
        D, lift = _tables(n_ceps, n_mels)
        hf = _framed(ctx, Nw, N, H, w, fb, mode)
        vf = hf.valid_frames(valid, T)
        assert vf.tolist() == sk.valid_frames(valid, Nw, H, T, True).tolist() and vf[2] == T and 0 < vf[3] < T and vf[4] == 0
        Y = _mel(ctx, hf, a, valid, "tc")
        hf.close()
        assert np.all(np.isfinite(Y)) and np.any(Y[0] != 0)
        want = sq.chain(D, Y, lift)
        for k in range(5):
            want[k, vf[k]:] = 0.0
        _WANT[(shape, mode)] = (a, valid, vf, want)
    return _WANT[(shape, mode)]


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("shape", SPECS)
def test_the_cepstrum_is_the_fmaf_chain_over_the_gpus_framed_output(ctx, shard, shape, layout):
    """Word for word, dead frames +0.0 in every row.  ln for every shape, power as well where the chain is short."""
    Nw, N, H, n_mels, n_bins, n_ceps = shape
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    D, lift = _tables(n_ceps, n_mels)
    for mode in ("ln", "power") if n_mels * n_ceps < 1000 else ("ln",):
        a, valid, vf, want = _want(ctx, shard, shape, mode)
        hq = _framed(ctx, Nw, N, H, w, fb, mode, dct=D, lifter=lift)
        assert hq.n_out == n_ceps and hq.valid_frames(valid, T).tolist() == vf.tolist()
        got = _mel(ctx, hq, a, valid, layout)
        hq.close()
        assert _same(got, want), (shape, mode, layout, float(np.max(np.abs(got - want))))


@pytest.mark.parametrize("shape", SPECS)
def test_the_energy_row(ctx, shard, shape):
    """load()'s 16-bit audio with the mean removed: row 0 within LOG_ULPS of the logarithm (float64) of E emulated in the stated lane
    order, rows 1.. the words of the spec without energy.  Integers |k| <= 127 over 32768 with the mean left in and energy_scale
    2^30: E is the exact integer energy, row 0 within LOG_ULPS of its logarithm; under a floor nothing is below logf(floor)."""
    Nw, N, H, n_mels, n_bins, n_ceps = shape
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    D, lift = _tables(n_ceps, n_mels)
    a, valid, vf, want = _want(ctx, shard, shape, "ln")
    le64 = sq.log_energy64(sq.energy32(sk.frames_of(a.cpu().numpy(), Nw, H, T), True, 2.0 ** 30))
    he = _framed(ctx, Nw, N, H, w, fb, "ln", dct=D, lifter=lift, energy=True, energy_scale=2.0 ** 30)
    worst = 0.0
    for layout in ("ct", "tc"):
        got = _mel(ctx, he, a, valid, layout)
        assert _same(got[:, :, 1:], want[:, :, 1:]), (shape, layout)
        for k in range(5):
            assert np.all(got[k, vf[k]:, 0].view(np.uint32) == 0)
            if vf[k]:
                ulps = sq.ulps_of(got[k, :vf[k], 0], le64[k, :vf[k]])
                worst = max(worst, float(ulps.max()))
                assert np.all(ulps <= sm.LOG_ULPS), (shape, layout, k, float(ulps.max()))
    he.close()
    L = (T - 1) * H + Nw
    small = (np.random.default_rng(Nw).integers(-127, 128, size=(2, L)).astype(np.float64) / 32768.0).astype(np.float32)
    small[1, :Nw] = np.float32(1.0 / 32768.0)
    X = sk.frames_of(small, Nw, H, T).astype(np.float64) * 32768.0
    exact = (X * X).sum(axis=-1)
    assert exact.max() < 2 ** 24 and exact[1, 0] == Nw
    dev = torch.from_numpy(small).to(a.device)
    for fl in (0.0, 1000.0):
        hs = cx.MelSpec.framed(ctx, R, N, Nw, H, w, fb, mode="ln", floor=EPS, preemph=PRE, whole_frames=True, dct=D, lifter=lift, energy=True,
                               energy_scale=2.0 ** 30, energy_floor=fl)
        got = _mel(ctx, hs, dev, [L, L], "ct")[:, :, 0]
        hs.close()
        ulps = sq.ulps_of(got, sq.log_energy64(exact, fl))
        worst = max(worst, float(ulps.max()))
        assert np.all(ulps <= sm.LOG_ULPS), (shape, fl, float(ulps.max()))
        if fl:
            assert got[1, 0] == got.min() and sq.ulps_of(got[1, 0], np.log(fl)) <= sm.LOG_ULPS
    print("energy rows of %r: worst %.2f ulps" % (shape, worst))


@pytest.mark.parametrize("use_energy", (False, True))
@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_read_mel_with_the_mfcc_spec(ctx, shard, layout, use_energy):
    s = shard[0]
    spec = cx.MelSpec.mfcc(ctx, use_energy=use_energy)
    assert (spec.n_fft, spec.win_length, spec.hop, spec.n_mels, spec.n_bins, spec.n_ceps, spec.n_out, spec.mode) == (512, 400, 160, 23, 256, 13, 13, "ln")
    assert np.array_equal(spec.fbank, sk.kaldi_fbank(R, 512, 23).astype(np.float32))
    assert np.array_equal(spec.dct, sq.dct_kaldi(13, 23).astype(np.float32)) and np.array_equal(spec.lifter, sq.lifter_kaldi(13).astype(np.float32))
    L = spec.window_len(T)
    assert L == 36 * 160 + 400
    sid, st = _calls(s, L)
    len16 = s.lengths_at(R).tolist()
    sid, st = sid + [0, 1], st + [len16[0] - 399, len16[1] - 400]                           # shorter than one frame; exactly one frame
    n0 = s.frames_decoded
    audio, valid = s.read(sid, st, L, "ct", sample_rate=R, channels=1)
    n1 = s.frames_decoded
    want = torch.empty((len(sid), 13, T) if layout == "ct" else (len(sid), T, 13), dtype=torch.float32, device=audio.device)
    ctx.mel_windows(spec, audio.view(len(sid), L), valid.numpy(), T, cx._LAYOUTS[layout], want)
    got, vf = s.read_mel(sid, st, T, spec, layout=layout)
    torch.cuda.synchronize()
    assert s.frames_decoded - n1 == n1 - n0 > 0
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got.view(torch.int32), want.view(torch.int32))
    v = valid.numpy().astype(np.int64)
    rule = np.where(v < 400, 0, np.minimum(1 + np.maximum(v - 400, 0) // 160, T))
    assert vf.dtype == torch.int64 and vf.tolist() == rule.tolist()
    assert v[-2] == 399 and vf[-2] == 0 and v[-1] == 400 and vf[-1] == 1 and vf[0] == T and 0 < vf[5] < T and vf[10] == 0
    # end to end against the float64 definition (these streams are a tone over faint noise: the intervals hold, but they are wide)
    x = audio.view(len(sid), L).cpu().numpy()
    C64, dC = sq.reference(x, spec.window, spec.fbank, 512, 160, T, True, spec.preemph, spec.floor, spec.dct, spec.lifter)
    g = (got.cpu().numpy().transpose(0, 2, 1) if layout == "ct" else got.cpu().numpy()).astype(np.float64)
    first = 1 if use_energy else 0
    for k in range(len(sid)):
        assert np.all(g[k, vf[k]:] == 0) and np.all(np.isfinite(g[k])), k
        assert np.all(np.abs(g[k, :vf[k], first:] - C64[k, :vf[k], first:]) <= dC[k, :vf[k], first:]), k
    if use_energy:                                                                            # row 0: the frame's log energy
        X = sk.frames_of(x.astype(np.float64), 400, 160, T)
        d = X - X.mean(axis=-1, keepdims=True)
        le = sq.log_energy64((d * d).sum(axis=-1) * 2.0 ** 30)
        plain = cx.MelSpec.mfcc(ctx)
        rest = s.read_mel(sid, st, T, plain, layout=layout)[0]
        torch.cuda.synchronize()
        plain.close()
        r = rest.cpu().numpy().transpose(0, 2, 1) if layout == "ct" else rest.cpu().numpy()
        assert _same(r[:, :, 1:], g[:, :, 1:].astype(np.float32))
        for k in range(len(sid)):
            assert np.all(np.abs(g[k, :vf[k], 0] - le[k, :vf[k]]) <= 1e-3), (k, float(np.max(np.abs(g[k, :vf[k], 0] - le[k, :vf[k]]))))
    with pytest.raises(cx.ClaxonError) as e:
        s.read_mel([0, 5], [0, 0], T, spec, layout=layout)
    assert e.value is s.problems[5]
    with pytest.raises(ValueError, match="not centred"):
        s.read_mel([0], [0], T, spec, length=L + 1)
    empty, vf0 = s.read_mel([], [], T, spec, layout=layout)
    none, vf1 = s.read_mel([0, 1], [0, 0], 0, spec, layout=layout)
    torch.cuda.synchronize()
    assert empty.numel() == 0 and vf0.numel() == 0 and none.numel() == 0 and vf1.tolist() == [0, 0]
    spec.close()
    with pytest.raises(ValueError):
        s.read_mel(sid, st, T, spec)


def test_noise_is_inside_the_float64_interval(ctx):
    """Uniform noise in [-1, 1), the same kind times 0.1 plus 0.05 (a large mean) and a window that stops half way, MelSpec.mfcc's
    tables: every live cell within dC of C64 (simlib_melq.reference: 4.12's dM through the logarithm, the DCT's sum in any order,
    one rounding for the lifter), both layouts.  So that this cannot go vacuous, 99 % of the intervals are no wider than WIDTH, which
    was chosen from the reference alone.  Measured on an MI355X: the kernel's worst error is 0.0007 of the bound."""
    spec = cx.MelSpec.mfcc(ctx)
    L = spec.window_len(T)
    a = np.random.default_rng(414).uniform(-1.0, 1.0, size=(3, L)).astype(np.float32)
    a[1] = a[1] * np.float32(0.1) + np.float32(0.05)
    valid = np.array([L, L, L // 2], dtype=np.uint32)
    a[2, valid[2]:] = 0.0
    vf = spec.valid_frames(valid, T)
    assert vf.tolist() == [T, T, 1 + (L // 2 - 400) // 160]
    C64, dC = sq.reference(a, spec.window, spec.fbank, 512, 160, T, True, spec.preemph, spec.floor, spec.dct, spec.lifter)
    width = np.concatenate([2.0 * dC[k, :vf[k]].reshape(-1) for k in range(3)])
    print("mfcc intervals: median width %.3g, 99th percentile %.3g, widest %.3g" % (float(np.median(width)), float(np.percentile(width, 99)), float(width.max())))
    assert np.mean(width <= WIDTH) >= 0.99
    dev = torch.from_numpy(a).to("cuda:0")
    worst = 0.0
    for layout in ("ct", "tc"):
        got = _mel(ctx, spec, dev, valid, layout).astype(np.float64)
        for k in range(3):
            assert np.all(got[k, vf[k]:] == 0)
            err = np.abs(got[k, :vf[k]] - C64[k, :vf[k]])
            worst = max(worst, float(np.max(err / dC[k, :vf[k]])))
            assert np.all(err <= dC[k, :vf[k]]), (layout, k, float(np.max(err / dC[k, :vf[k]])))
    print("mfcc: worst |error| / bound %.4f" % worst)
    spec.close()


def test_an_mfcc_a_kaldi_and_a_whisper_spec_side_by_side(ctx, shard):
    """Calls interleaved on one context: each spec gives what it gives alone (the shared table and its two events hold)."""
    s = shard[0]
    sid, st = [0, 1, 4, 2], [100, 2000, 9000, 16000]
    makers = (lambda: cx.MelSpec.mfcc(ctx, use_energy=True), lambda: cx.MelSpec.kaldi(ctx), lambda: cx.MelSpec.whisper(ctx))

    def alone(make):
        spec = make()
        out = s.read_mel(sid, st, T, spec)[0]
        torch.cuda.synchronize()
        spec.close()
        return out

    want = [alone(m) for m in makers]
    assert want[0].shape == (4, 13, T) and want[1].shape == (4, 80, T) and want[2].shape == (4, 80, T)
    assert not torch.equal(want[0], alone(lambda: cx.MelSpec.mfcc(ctx)))
    specs = [m() for m in makers]
    for _ in range(2):
        got = [s.read_mel(sid, st, T, spec)[0] for spec in specs]
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    for spec in specs:
        spec.close()
