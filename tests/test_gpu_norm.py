"""clx_norm_windows on the GPU: over the edge matrix of norm_cases.py the device's cells, stats and guard bands equal the wave
simulator's word for word in both layouts; calls queued back to back on one stream without a sync (tables growing and reused)
give what they give alone; read(..., normalize=) and read_mel(..., normalize=) from FLAC bytes -- mono and stereo streams, one of
them resampled -- equal read / read_mel followed by Context.norm_windows bit for bit, and the simulator on the same batch;
normalize=None is the call without the argument; and the recorded outside answers (tests/golden/features/norm_*.npz) hold from
FLAC bytes, inside the intervals of DESIGN.md 4.15."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import norm_cases as nc
import simlib_norm as sn
from gpu_guarded import device_out, written
from test_gpu_outside_features import _flac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _norm(o):
    return cx.Norm(bool(o["mean"]), bool(o["var"]), o["ddof"], o["eps"], o["pad"])


def _launch(ctx, c, layout, stream=None):
    """The case queued on the device: (flat, sflat or None) to be read back with _collect."""
    x = nc.data(c)
    B, rows, T = x.shape
    flat, body = device_out(x.size, offset_words=c["offset"])
    body.copy_(torch.from_numpy(nc.as_layout(x, layout).reshape(-1)))
    sflat, sbody = device_out(B * rows * 2, offset_words=1) if c["stats"] else (None, None)
    torch.cuda.synchronize()                                 # (the fills first: the launches may go to another stream)
    ctx.norm_windows((body.data_ptr(), B, rows, T), c["valid"], layout, _norm(c["o"]), stats=sbody.data_ptr() if c["stats"] else None,
                     stream=stream)
    return flat, sflat


def _collect(c, layout, flat, sflat):
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    cells = written(flat, B * rows * T, (c["name"], layout), offset_words=c["offset"]).view(np.float32)
    cells = nc.from_layout(cells.reshape((B, T, rows) if layout == sn.TC else (B, rows, T)), layout)
    stats = written(sflat, B * rows * 2, (c["name"], layout, "stats"), offset_words=1).view(np.float32).reshape(B, rows, 2) if c["stats"] else None
    return cells, stats


def _same_as_simulator(c, layout, cells, stats):
    want, wstats = nc.simulated(c["name"], layout)
    assert nc.same_words(cells, want), (c["name"], layout, "cells", int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))
    if c["stats"]:
        assert nc.same_words(stats, wstats), (c["name"], layout, "stats")


@pytest.mark.parametrize("layout", (sn.CT, sn.TC))
@pytest.mark.parametrize("name", nc.NAMES)
def test_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = nc.case(name)
    flat, sflat = _launch(ctx, c, layout)
    torch.cuda.synchronize()
    _same_as_simulator(c, layout, *_collect(c, layout, flat, sflat))


def test_calls_queued_back_to_back_on_one_stream(ctx):
    """Small, large (both tables grow), small again (both are reused), TC and CT in turn, nothing waited for in between."""
    st = torch.cuda.Stream(device=DEV)
    order = [("opts_mv", sn.CT), ("rows256", sn.TC), ("opts_mv1", sn.TC), ("T8195_rows3", sn.CT), ("opts_v", sn.CT)]
    bufs = []
    for name, layout in order:
        c = nc.case(name)
        x = nc.data(c)
        flat, body = device_out(x.size, offset_words=c["offset"])
        body.copy_(torch.from_numpy(nc.as_layout(x, layout).reshape(-1)))
        sflat, sbody = device_out(x.shape[0] * x.shape[1] * 2, offset_words=1) if c["stats"] else (None, None)
        bufs.append((c, layout, flat, body, sflat, sbody))
    torch.cuda.synchronize()
    for c, layout, flat, body, sflat, sbody in bufs:
        ctx.norm_windows((body.data_ptr(), len(c["valid"]), c["rows"], c["T"]), c["valid"], layout, _norm(c["o"]),
                         stats=sbody.data_ptr() if c["stats"] else None, stream=st)
    st.synchronize()
    for c, layout, flat, body, sflat, sbody in bufs:
        _same_as_simulator(c, layout, *_collect(c, layout, flat, sflat))


def _pcm(T, ch, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    return np.clip(np.rint(500.0 * (np.arange(ch)[None, :] + 1) + 5000.0 * np.sin(2 * np.pi * 300.0 * t / 16000.0 + np.arange(ch)[None, :])
                           + rng.normal(0, 700, (T, ch))), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def streams(ctx):
    """A mono stream at 16 kHz and a stereo one at 8 kHz (resampled when read at 16 kHz)."""
    s = cx.open_streams(ctx, [_flac(_pcm(5000, 1, 11), 16000), _flac(_pcm(3000, 2, 12), 8000)])
    assert s.problems == [None, None]
    return s


SID, STARTS = [0, 1, 0, 1, 0], [0, 100, 3500, 5000, 6000]    # whole windows, windows that run off their streams, one behind its stream


@pytest.mark.parametrize("layout", ("tc", "ct"))
@pytest.mark.parametrize("channels", (1, 2))
def test_read_normalize_is_read_then_norm_windows(ctx, streams, layout, channels):
    N = cx.Norm.wav2vec2()
    L = 2500
    got, v = streams.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels, normalize=N)
    plain, v2 = streams.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels)
    none, v3 = streams.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels, normalize=None)
    torch.cuda.synchronize()
    assert v.tolist() == v2.tolist() == v3.tolist() and 0 in v.tolist() and L in v.tolist() and any(0 < n < L for n in v.tolist())
    assert got.shape == plain.shape and torch.equal(plain.view(torch.int32), none.view(torch.int32))
    host = plain.cpu().numpy().copy()
    two = ctx.norm_windows(plain, v.numpy(), cx._LAYOUTS[layout], N)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    sim = sn.norm_windows(host, v.numpy(), cx._LAYOUTS[layout], sn.of_norm(N))
    assert nc.same_words(got.cpu().numpy(), sim)
    live = got.cpu().numpy()
    live = live if layout == "ct" else live.transpose(0, 2, 1)
    assert abs(float(live[0].mean())) < 1e-6 and abs(float(live[0].std()) - 1) < 1e-3 and np.all(live[4] == 0)


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("kind", ("kaldi", "whisper"))
def test_read_mel_normalize_is_read_mel_then_norm_windows(ctx, streams, kind, layout):
    spec = cx.MelSpec.kaldi(ctx) if kind == "kaldi" else cx.MelSpec.whisper(ctx)
    N = cx.Norm.cmvn() if kind == "kaldi" else cx.Norm(ddof=1, eps=1e-7, pad=-1.0)
    F = 12
    got, vf = streams.read_mel(SID, STARTS, F, spec, layout=layout, normalize=N)
    plain, vf2 = streams.read_mel(SID, STARTS, F, spec, layout=layout)
    none, vf3 = streams.read_mel(SID, STARTS, F, spec, layout=layout, normalize=None)
    torch.cuda.synchronize()
    assert vf.tolist() == vf2.tolist() == vf3.tolist() and 0 in vf.tolist() and F in vf.tolist()
    assert torch.equal(plain.view(torch.int32), none.view(torch.int32))
    host = plain.cpu().numpy().copy()
    two = ctx.norm_windows(plain, vf.numpy(), cx._LAYOUTS[layout], N)
    torch.cuda.synchronize()
    spec.close()
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    sim = sn.norm_windows(host, vf.numpy(), cx._LAYOUTS[layout], sn.of_norm(N))
    g = got.cpu().numpy()
    assert nc.same_words(g, sim)
    g = g if layout == "ct" else g.transpose(0, 2, 1)
    for k, n in enumerate(vf.tolist()):                      # dead frames are pad
        assert np.all(g[k, :, n:] == np.float32(N.pad))


def test_the_outside_wav2vec2_answer_from_flac_bytes(ctx):
    c = nc.outside("wav2vec2")
    s = cx.open_streams(ctx, [_flac(c.pcm[:, None], 16000)])
    for layout in ("ct", "tc"):
        got, v = s.read([0], [0], c.T, layout, normalize=cx.Norm.wav2vec2())
        torch.cuda.synchronize()
        assert v.tolist() == c.valid
        g = got.cpu().numpy()
        c.check(g if layout == "ct" else g.transpose(0, 2, 1), "read(normalize=) %s" % layout)


@pytest.mark.parametrize("name", ("cmvn_means", "cmvn_vars", "cmvn_both"))
def test_the_outside_cmvn_answers_from_flac_bytes(ctx, name):
    """Kaldi fbank and utterance CMVN in one read_mel call, against Speech2Text's CMVN of the outside fbank."""
    c = nc.outside_via_fbank(name)
    s = cx.open_streams(ctx, [_flac(c.stream, 16000)])
    spec = cx.MelSpec.kaldi(ctx)
    N = cx.Norm.cmvn(means=bool(c.o["mean"]), vars=bool(c.o["var"]))
    for layout in ("ct", "tc"):
        got, vf = s.read_mel([0], [0], c.T, spec, layout=layout, normalize=N)
        torch.cuda.synchronize()
        assert vf.tolist() == c.valid
        g = got.cpu().numpy()
        c.check(g if layout == "ct" else g.transpose(0, 2, 1), "read_mel(normalize=) %s" % layout)
    spec.close()


@pytest.mark.parametrize("layout", (sn.CT, sn.TC))
@pytest.mark.parametrize("name", nc.OUTSIDE)
def test_the_outside_answers_on_their_own_inputs(ctx, name, layout):
    """Context.norm_windows on the outside's own input rounded to float32, with stats: inside the interval, and the simulator's words."""
    c = nc.outside(name)
    a = nc.as_layout(c.x32, layout)
    d = torch.from_numpy(a).to(DEV)
    stats = torch.zeros((1, c.rows, 2), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.norm_windows(d, c.valid, layout, _norm(c.o), stats=stats)
    torch.cuda.synchronize()
    sstats = np.zeros((1, c.rows, 2), dtype=np.float32)
    sim = sn.norm_windows(a.copy(), c.valid, layout, c.o, sstats)
    assert nc.same_words(d.cpu().numpy(), sim) and nc.same_words(stats.cpu().numpy(), sstats)
    c.check(nc.from_layout(d.cpu().numpy(), layout), "norm_windows, layout %d" % layout)
