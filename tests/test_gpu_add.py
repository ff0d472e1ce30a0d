"""clx_add_windows on the GPU: over the edge matrix of add_cases.py the device's cells, gains and guard bands equal the wave
simulator's word for word in both layouts and the noise keeps every word; calls queued back to back on one stream without a sync
(tables growing and reused) give what they give alone; read(..., add=) and read_mel(..., add=) from FLAC bytes -- mono and stereo,
the set as its own noise source and a separate one, one stream resampled, a noise stream that ends inside the window, ids of -1,
channels=1 over a stereo noise -- equal read + read + Context.add_windows (+ mel_windows) bit for bit, and the simulator on the
same batches; add=None is the call without the argument."""
import numpy as np
import pytest
import torch

import add_cases as ac
import claxon_amd as cx
import simlib_add as sa
from gpu_guarded import device_out, written
from test_gpu_outside_features import _flac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _launch(ctx, c, layout, stream=None):
    """The case queued on the device: the buffers to be read back with _collect."""
    x, n = ac.data(c)
    B, rows, T = x.shape
    flat, body = device_out(x.size, offset_words=c["offset"])
    body.copy_(torch.from_numpy(ac.as_layout(x, layout).reshape(-1)))
    nflat, nbody = device_out(n.size, offset_words=c["noise_offset"])
    nbody.copy_(torch.from_numpy(ac.as_layout(n, layout).reshape(-1)))
    gflat, gbody = device_out(B, offset_words=1)
    torch.cuda.synchronize()                                 # (the fills first: the launches may go to another stream)
    ctx.add_windows((body.data_ptr(), B, rows, T), c["valid"], (nbody.data_ptr(), n.shape[0]), c["noise_valid"], c["index"], c["snr"], layout,
                    gains=gbody.data_ptr(), stream=stream)
    return flat, nflat, gflat


def _collect(c, layout, flat, nflat, gflat):
    x, n = ac.data(c)
    B, rows, T = x.shape
    cells = written(flat, x.size, (c["name"], layout), offset_words=c["offset"]).view(np.float32)
    cells = ac.from_layout(cells.reshape((B, T, rows) if layout == sa.TC else (B, rows, T)), layout)
    noise = written(nflat, n.size, (c["name"], layout, "noise"), offset_words=c["noise_offset"]).view(np.float32)
    assert ac.same_words(noise, ac.as_layout(n, layout).reshape(-1)), (c["name"], layout, "the noise was written")
    gains = written(gflat, B, (c["name"], layout, "gains"), offset_words=1).view(np.float32)
    return cells, gains


def _same_as_simulator(c, layout, cells, gains):
    want, wgains = ac.simulated(c["name"], layout)
    assert ac.same_words(gains, wgains), (c["name"], layout, "gains", gains, wgains)
    assert ac.same_words(cells, want), (c["name"], layout, "cells", int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))


@pytest.mark.parametrize("layout", (sa.CT, sa.TC))
@pytest.mark.parametrize("name", ac.NAMES)
def test_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = ac.case(name)
    bufs = _launch(ctx, c, layout)
    torch.cuda.synchronize()
    _same_as_simulator(c, layout, *_collect(c, layout, *bufs))


def test_calls_queued_back_to_back_on_one_stream(ctx):
    """Small, large (both tables grow), small again (both are reused), TC and CT in turn, nothing waited for in between."""
    st = torch.cuda.Stream(device=DEV)
    order = [("snr_range", sa.CT), ("T8195_rows3", sa.TC), ("zero_energy", sa.TC), ("T8195_rows3", sa.CT), ("T65_rows2", sa.CT)]
    # (one launch helper queues its fills on the current stream and waits for them; the add calls go to `st` one after the other)
    bufs = []
    for name, layout in order:
        c = ac.case(name)
        x, n = ac.data(c)
        flat, body = device_out(x.size, offset_words=c["offset"])
        body.copy_(torch.from_numpy(ac.as_layout(x, layout).reshape(-1)))
        nflat, nbody = device_out(n.size, offset_words=c["noise_offset"])
        nbody.copy_(torch.from_numpy(ac.as_layout(n, layout).reshape(-1)))
        gflat, gbody = device_out(x.shape[0], offset_words=1)
        bufs.append((c, layout, x.shape, n.shape[0], flat, body, nflat, nbody, gflat, gbody))
    torch.cuda.synchronize()
    for c, layout, shape, N, flat, body, nflat, nbody, gflat, gbody in bufs:
        ctx.add_windows((body.data_ptr(),) + tuple(shape), c["valid"], (nbody.data_ptr(), N), c["noise_valid"], c["index"], c["snr"], layout,
                        gains=gbody.data_ptr(), stream=st)
    st.synchronize()
    for c, layout, shape, N, flat, body, nflat, nbody, gflat, gbody in bufs:
        _same_as_simulator(c, layout, *_collect(c, layout, flat, nflat, gflat))


def _pcm(T, ch, seed, f0):
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    return np.clip(np.rint(300.0 * (np.arange(ch)[None, :] + 1) + 4000.0 * np.sin(2 * np.pi * f0 * t / 16000.0 + np.arange(ch)[None, :])
                           + rng.normal(0, 900, (T, ch))), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def speech(ctx):
    """Stream 0: mono, 16 kHz, 5000 samples.  1: stereo, 8 kHz, 3000 samples (resampled when read at 16 kHz).  2: mono, 16 kHz, 2100."""
    s = cx.open_streams(ctx, [_flac(_pcm(5000, 1, 21, 300.0), 16000), _flac(_pcm(3000, 2, 22, 170.0), 8000), _flac(_pcm(2100, 1, 23, 90.0), 16000)])
    assert s.problems == [None] * 3
    return s


@pytest.fixture(scope="module")
def noises(ctx):
    """A separate source.  Stream 0: stereo, 16 kHz, 4000 samples.  1: mono, 8 kHz, 1500 (3000 at 16 kHz).  2: stereo, 16 kHz, 900."""
    s = cx.open_streams(ctx, [_flac(_pcm(4000, 2, 31, 1100.0), 16000), _flac(_pcm(1500, 1, 32, 700.0), 8000), _flac(_pcm(900, 2, 33, 2300.0), 16000)])
    assert s.problems == [None] * 3
    return s


L = 2500
SID, STARTS = [0, 1, 0, 2, 1, 0], [0, 100, 3500, 0, 6000, 1000]       # whole windows, windows that run off their streams, one behind its stream
# per window: a whole noise; a resampled one; one that starts late in a short stream and ends inside the window; none; one for an
# empty window; one that ends inside the window at +inf
NID, NSTARTS, SNR = [0, 1, 2, -1, 0, 2], [700, 0, 300, 0, 0, 0], [10.0, 0.0, -5.0, 3.0, 20.0, float("inf")]
OWN_NID, OWN_NSTARTS = [2, 1, 0, -1, 2, 0], [0, 50, 4000, 0, 0, 4900]     # the reading set as its own source


def _two_reads(ctx, sset, src, nid, nstarts, layout, channels):
    """read + read + Context.add_windows: (the mixed batch, the plain one on the host, the noise on the host, valid, noise_valid, index, gains)."""
    plain, v = sset.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels)
    sel = [k for k, j in enumerate(nid) if j >= 0]
    noise, nv = src.read([nid[k] for k in sel], [nstarts[k] for k in sel], L, layout, sample_rate=16000, channels=channels)
    index = np.full(len(SID), -1, dtype=np.int32)
    index[sel] = np.arange(len(sel))
    gains = torch.full((len(SID),), -1.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()                                 # (the fill first: it runs on torch's stream, the add call on the context's)
    host, nhost = plain.cpu().numpy().copy(), noise.cpu().numpy().copy()
    ctx.add_windows(plain, v.numpy(), noise, nv.numpy(), index, SNR, cx._LAYOUTS[layout], gains=gains)
    torch.cuda.synchronize()
    assert torch.equal(noise.cpu().view(torch.int32), torch.from_numpy(nhost).view(torch.int32))
    return plain, host, nhost, v, nv, index, gains


@pytest.mark.parametrize("layout", ("tc", "ct"))
@pytest.mark.parametrize("own", (False, True))
@pytest.mark.parametrize("channels", (1, 2))
def test_read_add_is_read_read_add_windows(ctx, speech, noises, channels, own, layout):
    src, nid, nstarts = (speech, OWN_NID, OWN_NSTARTS) if own else (noises, NID, NSTARTS)
    f0 = src.frames_decoded
    got, v, g = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels, add=cx.Add(nid, nstarts, SNR, source=None if own else src),
                            return_gains=True)
    decoded = src.frames_decoded - f0
    two, host, nhost, v2, nv, index, g2 = _two_reads(ctx, speech, src, nid, nstarts, layout, channels)
    torch.cuda.synchronize()
    assert decoded * 2 == src.frames_decoded - f0 and decoded > 0                  # (the source counts its frames: the same both times)
    assert v.tolist() == v2.tolist() and 0 in v.tolist() and L in v.tolist() and any(0 < n < L for n in v.tolist())
    assert any(0 < n < m for n, m in zip(nv.tolist(), v.numpy()[index >= 0].tolist()))      # a noise that ends inside its window
    assert got.shape == two.shape and torch.equal(got.view(torch.int32), two.view(torch.int32))
    assert torch.equal(g.view(torch.int32), g2.view(torch.int32))
    gh = g.cpu().numpy()
    assert gh[3] == 0 and gh[4] == 0 and gh[5] == 0 and np.all(gh[:3] > 0)         # no noise, an empty window, +inf
    sgains = np.zeros(len(SID), dtype=np.float32)
    assert sa.add_windows(host, v.numpy(), nhost, nv.numpy(), index, SNR, cx._LAYOUTS[layout], sgains)
    assert ac.same_words(got.cpu().numpy(), host) and ac.same_words(gh, sgains)
    pair = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels, add=cx.Add(nid, nstarts, SNR, source=None if own else src))
    assert len(pair) == 2 and torch.equal(pair[0].view(torch.int32), got.view(torch.int32))


def test_read_add_at_the_native_rate_and_channel_count(ctx, speech, noises):
    """channels=None, no sample_rate: mono windows take mono noise; a stereo noise stream is refused by name."""
    sid, st, nid, nst = [0, 2, 0], [0, 100, 4000], [2, 0, -1], [0, 1000, 0]
    got, v, g = speech.read(sid, st, 1500, "ct", add=cx.Add(nid, nst, 6.0), return_gains=True)
    plain, _ = speech.read(sid, st, 1500, "ct")
    noise, nv = speech.read([2, 0], [0, 1000], 1500, "ct")
    ctx.add_windows(plain, v.numpy(), noise, nv.numpy(), [0, 1, -1], 6.0, cx.WINDOW_CT)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32)) and g.cpu().tolist()[2] == 0
    with pytest.raises(ValueError, match="noise stream 0 has 2 channels, the windows 1"):
        speech.read(sid, st, 1500, "ct", add=cx.Add([0, -1, -1], [0, 0, 0], 6.0, source=noises))


@pytest.mark.parametrize("layout", ("tc", "ct"))
def test_add_none_is_the_call_without_the_argument(speech, layout):
    a, va = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=2, add=None)
    b, vb = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=2)
    c, vc, g = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=2, add=cx.Add([-1] * len(SID), [0] * len(SID), 0.0), return_gains=True)
    torch.cuda.synchronize()
    assert va.tolist() == vb.tolist() == vc.tolist() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(c.view(torch.int32), b.view(torch.int32)) and g.cpu().tolist() == [0.0] * len(SID)
    spec = cx.MelSpec.kaldi(speech.ctx)
    m1, f1 = speech.read_mel(SID, STARTS, 8, spec, add=None)
    m2, f2 = speech.read_mel(SID, STARTS, 8, spec)
    torch.cuda.synchronize()
    spec.close()
    assert f1.tolist() == f2.tolist() and torch.equal(m1.view(torch.int32), m2.view(torch.int32))


@pytest.mark.parametrize("kind", ("kaldi", "whisper", "kaldi_reflected"))
def test_read_mel_add_is_the_features_of_the_noisy_waveform(ctx, speech, noises, kind):
    spec = {"kaldi": cx.MelSpec.kaldi, "whisper": cx.MelSpec.whisper, "kaldi_reflected": cx.MelSpec.kaldi_reflected}[kind](ctx)
    F = 12
    add = cx.Add(NID, NSTARTS, SNR, source=noises)
    got, vf = speech.read_mel(SID, STARTS, F, spec, layout="ct", add=add, normalize=cx.Norm.cmvn() if kind == "kaldi" else None)
    Lm = int(spec.window_len(F))
    audio, v = speech.read(SID, STARTS, Lm, "ct", sample_rate=spec.sample_rate, channels=1)
    noise, nv = noises.read([j for j in NID if j >= 0], [s for j, s in zip(NID, NSTARTS) if j >= 0], Lm, "ct", sample_rate=spec.sample_rate, channels=1)
    index = np.full(len(SID), -1, dtype=np.int32)
    index[[k for k, j in enumerate(NID) if j >= 0]] = np.arange(sum(j >= 0 for j in NID))
    clean = audio.clone()
    torch.cuda.synchronize()                                 # (the copy first: it runs on torch's stream, the add call on the context's)
    ctx.add_windows(audio, v.numpy(), noise, nv.numpy(), index, SNR, cx.WINDOW_CT)
    want = torch.empty_like(got)
    ctx.mel_windows(spec, audio.view(len(SID), Lm), v.numpy(), F, cx.WINDOW_CT, want)
    vf2 = spec.valid_frames(v.numpy(), F)
    if kind == "kaldi":
        ctx.norm_windows(want, vf2, cx.WINDOW_CT, cx.Norm.cmvn())
    torch.cuda.synchronize()
    spec.close()
    assert vf.tolist() == vf2.tolist() and not torch.equal(audio, clean)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
