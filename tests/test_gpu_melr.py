"""Reflected mel specs -- Kaldi's snip_edges=false -- on the GPU: the equality of test_melr_sim.py (the reflected spec's live cells
are, word for word, the whole-frame spec's cells on the explicitly reflected samples, built with Kaldi's loop on the host) for three
shapes, both layouts, fbank and cepstral with the energy row; one fbank and one cepstral case word for word against the wave
simulator's output (power mode, where nothing but fmaf chains and single roundings are computed); StreamSet.read_mel with
MelSpec.kaldi_reflected and MelSpec.mfcc_reflected(use_energy=True) over test_gpu_mel's five synthetic streams bit-equal to
read + mel_windows, with valid_frames by the count rule, length=None and a longer length; Norm.cmvn() on top equal to norm_windows by
hand; and a reflected, a snipped and a Whisper spec side by side on one context.  The outputs of mel_windows are guarded slices
(gpu_guarded.py)."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_mel as sm
import simlib_melr as sr
from test_gpu_mel import NAMES, SHAPES as STREAMS
from test_gpu_melq import _mel, _same
from test_gpu_mix import _stream
from test_melq_sim import _tables
from test_melr_sim import CEPS, COND, SCALE, SHAPES, _fb, _run, _window, batch

pytestmark = pytest.mark.gpu
R = 16000
EPS = float(np.finfo(np.float32).eps)
PRE = float(np.float32(0.97))
GPU_SHAPES = (SHAPES[0], SHAPES[2], SHAPES[3])              # Kaldi's defaults; odd numbers; H > Nw


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


@pytest.fixture(scope="module")
def shard(ctx):
    rng = np.random.default_rng(416)
    made = [_stream(rng, *STREAMS[name]) for name in NAMES]
    s = cx.open_streams(ctx, [m[0] for m in made] + [b"not a FLAC stream at all"])
    assert s.problems[:5] == [None] * 5 and isinstance(s.problems[5], cx.ClaxonError)
    return s


def _specs(ctx, shape, mode, cond, cep):
    """(the reflected spec, its whole-frame sibling with the same tables)."""
    Nw, N, H, n_mels, n_bins = shape[:5]
    kw = dict(mode=mode, floor=EPS, remove_dc=cond, preemph=PRE if cond else 0.0)
    if cep:
        D, lift = _tables(shape[5], n_mels)
        kw.update(dct=D, lifter=lift, energy=True, energy_scale=SCALE)
    w, fb = _window(Nw), _fb(N, n_mels, n_bins)
    return (cx.MelSpec.framed(ctx, R, N, Nw, H, w, fb, reflect_edges=True, **kw), cx.MelSpec.framed(ctx, R, N, Nw, H, w, fb, whole_frames=True, **kw))


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("shape", GPU_SHAPES + (CEPS[0],))
def test_the_reflected_spec_is_the_whole_frame_spec_on_the_reflected_samples(ctx, shape, layout):
    """16 windows of 0 .. 37 frames and more (test_melr_sim.valids), NaN from valid[k] on; ln and power, conditioned and not."""
    Nw, N, H = shape[:3]
    cep = len(shape) == 6
    a, V = batch(Nw, H, seed=17 + Nw)
    T = int(sr.count(V, H, 1 << 30).max()) + 3
    p, vp, Tk = sr.reflected_batch(a, V, Nw, H, T)
    da, dp = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(p).to("cuda:0")
    for mode in ("ln", "power"):
        for cond in (True, False):
            hr, hs = _specs(ctx, shape, mode, cond, cep)
            assert hr.reflect_edges and hr.valid_frames(V, T).tolist() == Tk.tolist() == hs.valid_frames(vp, T).tolist()
            want = _mel(ctx, hs, dp, vp, "tc", T)
            got = _mel(ctx, hr, da, V, layout, T)
            hr.close()
            hs.close()
            assert np.all(np.isfinite(want)) and np.any(want != 0)
            for k in range(len(V)):
                assert np.all(got[k, Tk[k]:].view(np.uint32) == 0), (mode, cond, k)
            assert _same(got, want), (shape, mode, cond, layout, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:3])


@pytest.mark.parametrize("shape", (SHAPES[0], CEPS[0]))
def test_the_gpus_words_are_the_simulators(ctx, shape):
    """Power mode, conditioned, both layouts (a cepstral spec without the energy row, whose last step is the device's logf): every
    sum is a chain of explicit fmaf in a fixed order, so the two builds of the source have nothing to differ in."""
    Nw, N, H, n_mels, n_bins = shape[:5]
    a, V = batch(Nw, H, seed=23)
    T = 37
    w, fb = _window(Nw), _fb(N, n_mels, n_bins)
    kw, cep = {}, None
    if len(shape) == 6:
        D, lift = _tables(shape[5], n_mels)
        kw, cep = dict(dct=D, lifter=lift), dict(n_ceps=shape[5], dct=D, lifter=lift)
    hr = cx.MelSpec.framed(ctx, R, N, Nw, H, w, fb, mode="power", remove_dc=True, preemph=PRE, reflect_edges=True, **kw)
    hsim = sr.create(N, Nw, H, w, fb, n_bins, n_mels, sm.POWER, EPS, COND, cep)
    da = torch.from_numpy(a).to("cuda:0")
    for layout in ("ct", "tc"):
        want = _run(hsim, a, V, T, cx._LAYOUTS[layout])
        got = _mel(ctx, hr, da, V, layout, T)
        assert np.any(want != 0) and _same(got, want), (shape, layout, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:3])
    sr.destroy(hsim)
    hr.close()


def _calls(s, L):
    """(stream ids, starts at 16 kHz): every stream from its start (Kaldi's whole-utterance placement), from mid-stream, and across
    its end; one window wholly behind its stream."""
    len16 = s.lengths_at(R).tolist()
    sid = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 2]
    st = [0] * 5 + [3, 1000, 77, 5000, 4321] + [len16[i] - L + 500 + 300 * i for i in range(5)] + [len16[2] + 4]
    return sid, st


@pytest.mark.parametrize("kind", ("fbank", "mfcc"))
@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_read_mel_with_the_reflected_specs(ctx, shard, layout, kind):
    s = shard
    spec = cx.MelSpec.kaldi_reflected(ctx) if kind == "fbank" else cx.MelSpec.mfcc_reflected(ctx, use_energy=True)
    rows = 80 if kind == "fbank" else 13
    assert (spec.n_fft, spec.win_length, spec.hop, spec.n_bins, spec.n_out, spec.mode, spec.reflect_edges, spec.whole_frames) == (512, 400, 160, 256, rows, "ln", True, False)
    T = 37
    assert spec.window_len(T) == T * 160
    for length in (None, T * 160 + 123):
        L = T * 160 if length is None else length
        sid, st = _calls(s, L)
        n0 = s.frames_decoded
        audio, valid = s.read(sid, st, L, "ct", sample_rate=R, channels=1)
        n1 = s.frames_decoded
        want = torch.empty((len(sid), rows, T) if layout == "ct" else (len(sid), T, rows), dtype=torch.float32, device=audio.device)
        ctx.mel_windows(spec, audio.view(len(sid), L), valid.numpy(), T, cx._LAYOUTS[layout], want)
        got, vf = s.read_mel(sid, st, T, spec, layout=layout, length=length)
        torch.cuda.synchronize()
        assert s.frames_decoded - n1 == n1 - n0 > 0
        assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got.view(torch.int32), want.view(torch.int32))
        v = valid.numpy().astype(np.int64)
        rule = np.minimum((v + 80) // 160, T)
        assert vf.dtype == torch.int64 and vf.tolist() == rule.tolist()
        assert vf[0] == T and 0 < vf[10] < T and vf[15] == 0 and v[15] == 0
        g = got.cpu().numpy().transpose(0, 2, 1) if layout == "ct" else got.cpu().numpy()
        for k in range(len(sid)):
            assert np.all(g[k, vf[k]:].view(np.uint32) == 0) and np.all(np.isfinite(g[k])), k
            assert vf[k] == 0 or np.any(g[k, :vf[k]] != 0), k
    # the whole of a stream, as Kaldi frames an utterance: start 0, length >= its samples, (samples + 80) // 160 frames
    n = int(s.lengths_at(R)[0])
    frames = (n + 80) // 160
    whole, vfw = s.read_mel([0], [0], frames + 2, spec, layout=layout, length=n + 7)
    torch.cuda.synchronize()
    assert vfw.tolist() == [frames]
    with pytest.raises(cx.ClaxonError) as e:
        s.read_mel([0, 5], [0, 0], T, spec, layout=layout)
    assert e.value is s.problems[5]
    with pytest.raises(ValueError, match="length must be a whole number"):
        s.read_mel([0], [0], T, spec, length=-1)
    empty, vf0 = s.read_mel([], [], T, spec, layout=layout)
    none, vf1 = s.read_mel([0, 1], [0, 0], 0, spec, layout=layout)
    short, vf2 = s.read_mel([0, 1], [0, 0], 3, spec, layout=layout, length=1)   # (one sample: fewer than hop - hop // 2, no frame)
    torch.cuda.synchronize()
    assert empty.numel() == 0 and vf0.numel() == 0 and none.numel() == 0 and vf1.tolist() == [0, 0]
    assert vf2.tolist() == [0, 0] and short.shape[0] == 2 and not short.cpu().numpy().view(np.uint32).any()
    spec.close()
    with pytest.raises(ValueError):
        s.read_mel(sid, st, T, spec)


@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_cmvn_on_top_is_norm_windows_by_hand(ctx, shard, layout):
    s = shard
    spec = cx.MelSpec.kaldi_reflected(ctx)
    T, N = 12, cx.Norm.cmvn()
    sid, st = _calls(s, T * 160)
    got, vf = s.read_mel(sid, st, T, spec, layout=layout, normalize=N)
    plain, vf2 = s.read_mel(sid, st, T, spec, layout=layout)
    torch.cuda.synchronize()
    assert vf.tolist() == vf2.tolist() and 0 in vf.tolist() and T in vf.tolist()
    two = ctx.norm_windows(plain, vf.numpy(), cx._LAYOUTS[layout], N)
    torch.cuda.synchronize()
    spec.close()
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))


def test_a_reflected_a_snipped_and_a_whisper_spec_side_by_side(ctx, shard):
    """Calls interleaved on one context: each spec gives what it gives alone (the shared table -- one, two or three words a window --
    and its two events hold)."""
    s = shard
    T = 37
    sid, st = [0, 1, 4, 2], [100, 2000, 9000, 16000]
    makers = (lambda: cx.MelSpec.kaldi_reflected(ctx), lambda: cx.MelSpec.mfcc_reflected(ctx, use_energy=True), lambda: cx.MelSpec.kaldi(ctx),
              lambda: cx.MelSpec.whisper(ctx))

    def alone(make):
        spec = make()
        out = s.read_mel(sid, st, T, spec)[0]
        torch.cuda.synchronize()
        spec.close()
        return out

    want = [alone(m) for m in makers]
    assert [tuple(w.shape) for w in want] == [(4, 80, T), (4, 13, T), (4, 80, T), (4, 80, T)]
    assert not torch.equal(want[0], want[2])
    specs = [m() for m in makers]
    for _ in range(2):
        got = [s.read_mel(sid, st, T, spec)[0] for spec in specs]
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    for spec in specs:
        spec.close()
