"""clx_reverb_windows on the GPU: over the edge matrix of reverb_cases.py the device's cells, gains and guard bands equal the wave
simulator's word for word in both layouts, and the data and the responses keep every word; calls queued back to back on one stream
without a sync (tables growing and reused, CT and TC in turn) give what they give alone; read(..., reverb=) and
read_mel(..., reverb=) from FLAC bytes -- mono and stereo speech, one stream resampled, responses of which one is resampled and one
ends before `taps`, an id of -1, a window that runs off its stream and one behind its stream's end -- equal read + source.read +
Context.reverb_windows (+ add_windows, norm_windows, mel_windows) bit for bit, and the simulator on the same batches; reverb=None is
the call without the argument."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import reverb_cases as rc
import simlib_reverb as sr
from gpu_guarded import device_out, written
from test_gpu_outside_features import _flac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _launch(ctx, c, layout, stream=None):
    """The case queued on the device: the buffers to be read back with _collect."""
    x, ir = rc.data(c)
    B, rows, T = x.shape
    flat, body = device_out(x.size, offset_words=c["offset"])
    body.copy_(torch.from_numpy(rc.as_layout(x, layout).reshape(-1)))
    iflat, ibody = device_out(ir.size, offset_words=c["ir_offset"])
    ibody.copy_(torch.from_numpy(ir.reshape(-1)))
    oflat, obody = device_out(x.size, offset_words=c["out_offset"])
    gflat, gbody = device_out(B, offset_words=1)
    torch.cuda.synchronize()                                 # (the fills first: the launches may go to another stream)
    ctx.reverb_windows((body.data_ptr(), B, rows, T), c["valid"], (ibody.data_ptr(), ir.shape[0], c["K"]), c["lens"], c["index"], layout,
                       out=obody.data_ptr(), keep_power=bool(c["keep"]), gains=gbody.data_ptr(), stream=stream)
    return flat, iflat, oflat, gflat


def _collect(c, layout, flat, iflat, oflat, gflat):
    x, ir = rc.data(c)
    B, rows, T = x.shape
    kept = written(flat, x.size, (c["name"], layout, "data"), offset_words=c["offset"]).view(np.float32)
    assert rc.same_words(kept, rc.as_layout(x, layout).reshape(-1)), (c["name"], layout, "the data was written")
    kept = written(iflat, ir.size, (c["name"], layout, "responses"), offset_words=c["ir_offset"]).view(np.float32)
    assert rc.same_words(kept, ir.reshape(-1)), (c["name"], layout, "the responses were written")
    cells = written(oflat, x.size, (c["name"], layout), offset_words=c["out_offset"]).view(np.float32)
    cells = rc.from_layout(cells.reshape((B, T, rows) if layout == sr.TC else (B, rows, T)), layout)
    gains = written(gflat, B, (c["name"], layout, "gains"), offset_words=1).view(np.float32)
    return cells, gains


def _same_as_simulator(c, layout, cells, gains):
    want, wgains = rc.simulated(c["name"], layout)
    assert rc.same_words(gains, wgains), (c["name"], layout, "gains", gains, wgains)
    assert rc.same_words(cells, want), (c["name"], layout, "cells", int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))


@pytest.mark.parametrize("layout", (sr.CT, sr.TC))
@pytest.mark.parametrize("name", rc.NAMES)
def test_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = rc.case(name)
    bufs = _launch(ctx, c, layout)
    torch.cuda.synchronize()
    _same_as_simulator(c, layout, *_collect(c, layout, *bufs))


def test_calls_queued_back_to_back_on_one_stream(ctx):
    """Small, large with keep_power (both tables grow), small again (both are reused), TC and CT in turn, nothing waited for in
    between."""
    st = torch.cuda.Stream(device=DEV)
    T2 = 2 * rc.TILE + 3
    order = [("nan_and_inf_taps", sr.CT), ("T%d_rows3_b1" % T2, sr.TC), ("zero_energy", sr.TC), ("T%d_rows3_b1" % T2, sr.CT), ("T%d_rows2_b0" % (rc.CHUNK + 5), sr.CT)]
    bufs = []
    for name, layout in order:
        c = rc.case(name)
        x, ir = rc.data(c)
        flat, body = device_out(x.size, offset_words=c["offset"])
        body.copy_(torch.from_numpy(rc.as_layout(x, layout).reshape(-1)))
        iflat, ibody = device_out(ir.size, offset_words=c["ir_offset"])
        ibody.copy_(torch.from_numpy(ir.reshape(-1)))
        oflat, obody = device_out(x.size, offset_words=c["out_offset"])
        gflat, gbody = device_out(x.shape[0], offset_words=1)
        bufs.append((c, layout, x.shape, ir.shape[0], flat, body, iflat, ibody, oflat, obody, gflat, gbody))
    torch.cuda.synchronize()
    for c, layout, shape, N, flat, body, iflat, ibody, oflat, obody, gflat, gbody in bufs:
        ctx.reverb_windows((body.data_ptr(),) + tuple(shape), c["valid"], (ibody.data_ptr(), N, c["K"]), c["lens"], c["index"], layout,
                           out=obody.data_ptr(), keep_power=bool(c["keep"]), gains=gbody.data_ptr(), stream=st)
    st.synchronize()
    for c, layout, shape, N, flat, body, iflat, ibody, oflat, obody, gflat, gbody in bufs:
        _same_as_simulator(c, layout, *_collect(c, layout, flat, iflat, oflat, gflat))


def _pcm(T, ch, seed, f0):
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    return np.clip(np.rint(300.0 * (np.arange(ch)[None, :] + 1) + 4000.0 * np.sin(2 * np.pi * f0 * t / 16000.0 + np.arange(ch)[None, :])
                           + rng.normal(0, 900, (T, ch))), -32768, 32767).astype(np.int16)


def _rir(T, seed, tau):
    """Decaying noise behind a direct path."""
    rng = np.random.default_rng(seed)
    h = rng.normal(0, 6000, T) * np.exp(-np.arange(T) / tau)
    h[0] = 20000.0
    return np.clip(np.rint(h), -32768, 32767).astype(np.int16)[:, None]


@pytest.fixture(scope="module")
def speech(ctx):
    """Stream 0: mono, 16 kHz, 5000 samples.  1: stereo, 8 kHz, 3000 samples (resampled when read at 16 kHz).  2: mono, 16 kHz, 2100."""
    s = cx.open_streams(ctx, [_flac(_pcm(5000, 1, 21, 300.0), 16000), _flac(_pcm(3000, 2, 22, 170.0), 8000), _flac(_pcm(2100, 1, 23, 90.0), 16000)])
    assert s.problems == [None] * 3
    return s


@pytest.fixture(scope="module")
def rirs(ctx):
    """Mono responses.  Stream 0: 16 kHz, 700 samples.  1: 8 kHz, 300 (600 at 16 kHz).  2: 16 kHz, 300: it ends before TAPS."""
    s = cx.open_streams(ctx, [_flac(_rir(700, 41, 120.0), 16000), _flac(_rir(300, 42, 50.0), 8000), _flac(_rir(300, 43, 70.0), 16000)])
    assert s.problems == [None] * 3
    return s


@pytest.fixture(scope="module")
def noises(ctx):
    s = cx.open_streams(ctx, [_flac(_pcm(4000, 1, 31, 1100.0), 16000)])
    assert s.problems == [None]
    return s


L, TAPS = 2500, 2 * 256
SID, STARTS = [0, 1, 0, 2, 1, 0], [0, 100, 3500, 0, 6000, 1000]       # whole windows, windows that run off their streams, one behind its stream
RID, RSTARTS = [0, 1, 2, -1, 0, 2], [0, 3, 10, 0, 0, 0]               # a truncated response, a resampled one, a short one, none, one for an empty window


def _explicit(ctx, sset, src, layout, channels, keep, taps=TAPS, length=L):
    """read + source.read + Context.reverb_windows: (the wet batch, the dry one and the responses on the host, valid, ir_len, index, gains)."""
    dry, v = sset.read(SID, STARTS, length, layout, sample_rate=16000, channels=channels)
    sel = [k for k, j in enumerate(RID) if j >= 0]
    ir, il = src.read([RID[k] for k in sel], [RSTARTS[k] for k in sel], taps, "ct", sample_rate=16000, channels=None)
    index = np.full(len(SID), -1, dtype=np.int32)
    index[sel] = np.arange(len(sel))
    gains = torch.full((len(SID),), -1.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()                                 # (the fill first: it runs on torch's stream, the call on the context's)
    wet = ctx.reverb_windows(dry, v.numpy(), ir.view(len(sel), taps), il.numpy(), index, cx._LAYOUTS[layout], keep_power=keep, gains=gains)
    torch.cuda.synchronize()
    return wet, dry.cpu().numpy().copy(), ir.view(len(sel), taps).cpu().numpy().copy(), v, il, index, gains


@pytest.mark.parametrize("layout,channels,keep", (("tc", 1, True), ("ct", 1, False), ("tc", 2, False), ("ct", 2, True)))
def test_read_reverb_is_read_read_reverb_windows(ctx, speech, rirs, layout, channels, keep):
    f0, s0 = rirs.frames_decoded, speech.frames_decoded
    got, v = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels, reverb=cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS, keep_power=keep))
    torch.cuda.synchronize()
    decoded, sdecoded = rirs.frames_decoded - f0, speech.frames_decoded - s0
    wet, dry, ir, v2, il, index, gains = _explicit(ctx, speech, rirs, layout, channels, keep)
    assert decoded * 2 == rirs.frames_decoded - f0 and decoded > 0                 # the source counts the responses' frames, and only them
    assert sdecoded * 2 == speech.frames_decoded - s0 and sdecoded > 0
    assert v.tolist() == v2.tolist() and 0 in v.tolist() and L in v.tolist() and any(0 < n < L for n in v.tolist())
    assert il.tolist()[0] == TAPS and 0 < il.tolist()[2] < TAPS                    # one response truncated, one that ends before taps
    assert got.shape == wet.shape and torch.equal(got.view(torch.int32), wet.view(torch.int32))
    assert not np.array_equal(got.cpu().numpy(), dry)
    sim, sgains = np.full_like(dry, 7.0), np.zeros(len(SID), dtype=np.float32)
    assert sr.reverb_windows(dry, v.numpy(), ir, il.numpy(), index, cx._LAYOUTS[layout], sim, int(keep), sgains)
    assert rc.same_words(got.cpu().numpy(), sim) and rc.same_words(gains.cpu().numpy(), sgains)
    gh = gains.cpu().numpy()
    assert gh[3] == 1 and gh[4] == 1 and (np.all(gh[:3] != 1) if keep else np.all(gh == 1))
    k3 = got.cpu().numpy()[3]
    assert np.array_equal(k3.view(np.uint32), dry[3].view(np.uint32))               # the window without a response is the dry one


def test_taps_none_takes_the_longest_named_response(ctx, speech, rirs):
    got, v = speech.read(SID, STARTS, L, "ct", sample_rate=16000, channels=1, reverb=cx.Reverb(RID, rirs, starts=RSTARTS))
    torch.cuda.synchronize()
    wet = _explicit(ctx, speech, rirs, "ct", 1, True, taps=700)[0]
    assert torch.equal(got.view(torch.int32), wet.view(torch.int32))


@pytest.mark.parametrize("layout", ("tc", "ct"))
def test_reverb_then_add_then_normalize(ctx, speech, rirs, noises, layout):
    add = cx.Add([0, 0, -1, 0, 0, 0], [0, 500, 0, 100, 0, 1500], [10.0, 0.0, 3.0, -5.0, 20.0, 5.0], source=noises)
    norm = cx.Norm()
    got, v, g = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=2, normalize=norm, add=add, return_gains=True,
                            reverb=cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS))
    torch.cuda.synchronize()
    wet = _explicit(ctx, speech, rirs, layout, 2, True)[0]
    sel = [k for k, j in enumerate(add.stream_ids.tolist()) if j >= 0]
    noise, nv = noises.read([0] * len(sel), add.starts[sel], L, layout, sample_rate=16000, channels=2)
    index = np.full(len(SID), -1, dtype=np.int32)
    index[sel] = np.arange(len(sel))
    g2 = torch.full((len(SID),), -1.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.add_windows(wet, v.numpy(), noise, nv.numpy(), index, add.snr_db, cx._LAYOUTS[layout], gains=g2)
    ctx.norm_windows(wet, v.numpy(), cx._LAYOUTS[layout], norm)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), wet.view(torch.int32)) and torch.equal(g.view(torch.int32), g2.view(torch.int32))


def test_read_mel_reverb_is_the_features_of_the_reverberant_waveform(ctx, speech, rirs):
    spec = cx.MelSpec.kaldi(ctx)
    F = 12
    rv = cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS)
    got, vf = speech.read_mel(SID, STARTS, F, spec, layout="ct", reverb=rv)
    Lm = int(spec.window_len(F))
    audio, v = speech.read(SID, STARTS, Lm, "ct", sample_rate=spec.sample_rate, channels=1, reverb=rv)
    dry, _ = speech.read(SID, STARTS, Lm, "ct", sample_rate=spec.sample_rate, channels=1)
    want = torch.empty_like(got)
    torch.cuda.synchronize()
    ctx.mel_windows(spec, audio.view(len(SID), Lm), v.numpy(), F, cx.WINDOW_CT, want)
    torch.cuda.synchronize()
    vf2 = spec.valid_frames(v.numpy(), F)
    spec.close()
    assert vf.tolist() == vf2.tolist() and not torch.equal(audio, dry)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("layout", ("tc", "ct"))
def test_reverb_none_is_the_call_without_the_argument(speech, rirs, layout):
    a, va = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=2, reverb=None)
    b, vb = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=2)
    f0 = rirs.frames_decoded
    c, vc = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=2, reverb=cx.Reverb([-1] * len(SID), rirs))
    torch.cuda.synchronize()
    assert va.tolist() == vb.tolist() == vc.tolist() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(c.view(torch.int32), b.view(torch.int32)) and rirs.frames_decoded == f0
    spec = cx.MelSpec.kaldi(speech.ctx)
    m1, f1 = speech.read_mel(SID, STARTS, 8, spec, reverb=None)
    m2, f2 = speech.read_mel(SID, STARTS, 8, spec)
    torch.cuda.synchronize()
    spec.close()
    assert f1.tolist() == f2.tolist() and torch.equal(m1.view(torch.int32), m2.view(torch.int32))
