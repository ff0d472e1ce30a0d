"""clx_reverb_windows_fft on the GPU: over the edge matrix of reverb_fft_cases.py the device's cells, gains and guard bands equal the
wave simulator's word for word in both layouts, and the data and the responses keep every word; five calls queued back to back on one
stream without a sync (tables and workspace growing and reused, CT and TC in turn) give what they give alone;
read(..., reverb=Reverb(..., method="fft")), read(reverb=, add=, normalize=) and read_mel(reverb=) from FLAC bytes equal the explicit
chains (read, source.read, Context.reverb_windows(method="fft"), add_windows, norm_windows, mel_windows) bit for bit, and the simulator
on the same batch; method="direct" through the new argument is the call without it, and so is
method="auto" under REVERB_FFT_TAPS."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import reverb_fft_cases as rc
import simlib_reverb_fft as sf
from gpu_guarded import device_out, written
from test_gpu_outside_features import _flac
from test_gpu_reverb import _pcm, _rir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _buffers(c, layout):
    x, ir = rc.data(c)
    flat, body = device_out(x.size, offset_words=c["offset"])
    body.copy_(torch.from_numpy(rc.as_layout(x, layout).reshape(-1)))
    iflat, ibody = device_out(ir.size, offset_words=c["ir_offset"])
    ibody.copy_(torch.from_numpy(ir.reshape(-1)))
    oflat, obody = device_out(x.size, offset_words=c["out_offset"])
    gflat, gbody = device_out(x.shape[0], offset_words=1)
    return x.shape, ir.shape[0], (flat, iflat, oflat, gflat), (body, ibody, obody, gbody)


def _queue(ctx, c, layout, shape, n_ir, bodies, stream=None):
    body, ibody, obody, gbody = bodies
    ctx.reverb_windows((body.data_ptr(),) + tuple(shape), c["valid"], (ibody.data_ptr(), n_ir, c["K"]), c["lens"], c["index"], layout,
                       out=obody.data_ptr(), keep_power=bool(c["keep"]), gains=gbody.data_ptr(), stream=stream, method="fft")


def _collect(c, layout, flat, iflat, oflat, gflat):
    x, ir = rc.data(c)
    B, rows, T = x.shape
    kept = written(flat, x.size, (c["name"], layout, "data"), offset_words=c["offset"]).view(np.float32)
    assert rc.same_words(kept, rc.as_layout(x, layout).reshape(-1)), (c["name"], layout, "the data was written")
    kept = written(iflat, ir.size, (c["name"], layout, "responses"), offset_words=c["ir_offset"]).view(np.float32)
    assert rc.same_words(kept, ir.reshape(-1)), (c["name"], layout, "the responses were written")
    cells = written(oflat, x.size, (c["name"], layout), offset_words=c["out_offset"]).view(np.float32)
    cells = rc.from_layout(cells.reshape((B, T, rows) if layout == sf.TC else (B, rows, T)), layout)
    gains = written(gflat, B, (c["name"], layout, "gains"), offset_words=1).view(np.float32)
    return cells, gains


def _same_as_simulator(c, layout, cells, gains):
    want, wgains = rc.simulated(c["name"], layout)
    ok = rc.specified(c)
    assert rc.same_words(gains[ok], wgains[ok]), (c["name"], layout, "gains", gains, wgains)
    a, b = rc.masked(c, cells), rc.masked(c, want)
    assert rc.same_words(a, b), (c["name"], layout, "cells", int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))))


@pytest.mark.parametrize("layout", (sf.CT, sf.TC))
@pytest.mark.parametrize("name", rc.NAMES)
def test_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = rc.case(name)
    shape, n_ir, flats, bodies = _buffers(c, layout)
    torch.cuda.synchronize()                                 # (the fills first: the launches may go to another stream)
    _queue(ctx, c, layout, shape, n_ir, bodies)
    torch.cuda.synchronize()
    _same_as_simulator(c, layout, *_collect(c, layout, *flats))


def test_five_calls_queued_back_to_back_on_one_stream(ctx):
    """Small, large with keep_power (the tables and the workspace grow), small again (all are reused), TC and CT in turn, nothing
    waited for in between."""
    st = torch.cuda.Stream(device=DEV)
    T2 = 2 * rc.H + 3
    order = [("nan_tap", sf.CT), ("T%d_rows8_a1" % (rc.H + 5), sf.TC), ("zero_energy", sf.TC), ("T%d_rows3_a0" % T2, sf.CT), ("T%d_rows1_a0" % rc.H, sf.CT)]
    bufs = [(rc.case(name), layout) + _buffers(rc.case(name), layout) for name, layout in order]
    torch.cuda.synchronize()
    for c, layout, shape, n_ir, flats, bodies in bufs:
        _queue(ctx, c, layout, shape, n_ir, bodies, stream=st)
    st.synchronize()
    for c, layout, shape, n_ir, flats, bodies in bufs:
        _same_as_simulator(c, layout, *_collect(c, layout, *flats))


@pytest.fixture(scope="module")
def speech(ctx):
    """Stream 0: mono, 16 kHz, 5000 samples.  1: stereo, 8 kHz, 3000 samples (resampled when read at 16 kHz).  2: mono, 16 kHz, 2100."""
    s = cx.open_streams(ctx, [_flac(_pcm(5000, 1, 21, 300.0), 16000), _flac(_pcm(3000, 2, 22, 170.0), 8000), _flac(_pcm(2100, 1, 23, 90.0), 16000)])
    assert s.problems == [None] * 3
    return s


@pytest.fixture(scope="module")
def rirs(ctx):
    """Mono responses.  Stream 0: 16 kHz, 1500 samples.  1: 8 kHz, 300 (600 at 16 kHz).  2: 16 kHz, 300: it ends before TAPS."""
    s = cx.open_streams(ctx, [_flac(_rir(1500, 41, 300.0), 16000), _flac(_rir(300, 42, 50.0), 8000), _flac(_rir(300, 43, 70.0), 16000)])
    assert s.problems == [None] * 3
    return s


@pytest.fixture(scope="module")
def noises(ctx):
    s = cx.open_streams(ctx, [_flac(_pcm(4000, 1, 31, 1100.0), 16000)])
    assert s.problems == [None]
    return s


L, TAPS = 2500, 1024 + 200                                              # three blocks; a response of more than one partition
SID, STARTS = [0, 1, 0, 2, 1, 0], [0, 100, 3500, 0, 6000, 1000]       # whole windows, windows that run off their streams, one behind its stream
RID, RSTARTS = [0, 1, 2, -1, 0, 2], [0, 3, 10, 0, 0, 0]               # a truncated response, a resampled one, a short one, none, one for an empty window


def _explicit(ctx, sset, src, layout, channels, keep, method="fft", length=L):
    """read + source.read + Context.reverb_windows: (the wet batch, the dry one and the responses on the host, valid, ir_len, index, gains)."""
    dry, v = sset.read(SID, STARTS, length, layout, sample_rate=16000, channels=channels)
    sel = [k for k, j in enumerate(RID) if j >= 0]
    ir, il = src.read([RID[k] for k in sel], [RSTARTS[k] for k in sel], TAPS, "ct", sample_rate=16000, channels=None)
    index = np.full(len(SID), -1, dtype=np.int32)
    index[sel] = np.arange(len(sel))
    gains = torch.full((len(SID),), -1.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()                                 # (the fill first: it runs on torch's stream, the call on the context's)
    kw = {} if method is None else dict(method=method)
    wet = ctx.reverb_windows(dry, v.numpy(), ir.view(len(sel), TAPS), il.numpy(), index, cx._LAYOUTS[layout], keep_power=keep, gains=gains, **kw)
    torch.cuda.synchronize()
    return wet, dry.cpu().numpy().copy(), ir.view(len(sel), TAPS).cpu().numpy().copy(), v, il, index, gains


@pytest.mark.parametrize("layout,channels,keep", (("tc", 2, True), ("ct", 1, False)))
def test_read_reverb_fft_is_read_read_reverb_windows_fft(ctx, speech, rirs, layout, channels, keep):
    got, v = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels,
                         reverb=cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS, keep_power=keep, method="fft"))
    torch.cuda.synchronize()
    wet, dry, ir, v2, il, index, gains = _explicit(ctx, speech, rirs, layout, channels, keep)
    assert v.tolist() == v2.tolist() and 0 in v.tolist() and L in v.tolist() and any(0 < n < L for n in v.tolist())
    assert il.tolist()[0] == TAPS and 0 < il.tolist()[2] < TAPS                    # one response truncated, one that ends before taps
    assert got.shape == wet.shape and torch.equal(got.view(torch.int32), wet.view(torch.int32))
    sim, sgains = np.full_like(dry, 7.0), np.zeros(len(SID), dtype=np.float32)
    assert sf.reverb_windows(dry, v.numpy(), ir, il.numpy(), index, cx._LAYOUTS[layout], sim, int(keep), sgains)
    assert rc.same_words(got.cpu().numpy(), sim) and rc.same_words(gains.cpu().numpy(), sgains)
    direct = _explicit(ctx, speech, rirs, layout, channels, keep, method="direct")[0]
    assert not torch.equal(got.view(torch.int32), direct.view(torch.int32))       # (another method: its own words)
    assert np.array_equal(got.cpu().numpy()[3].view(np.uint32), dry[3].view(np.uint32))          # the window without a response is the dry one


@pytest.mark.parametrize("layout", ("tc", "ct"))
def test_reverb_fft_then_add_then_normalize(ctx, speech, rirs, noises, layout):
    add = cx.Add([0, 0, -1, 0, 0, 0], [0, 500, 0, 100, 0, 1500], [10.0, 0.0, 3.0, -5.0, 20.0, 5.0], source=noises)
    norm = cx.Norm()
    got, v, g = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=2, normalize=norm, add=add, return_gains=True,
                            reverb=cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS, method="fft"))
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


def test_read_mel_reverb_fft_is_the_features_of_the_reverberant_waveform(ctx, speech, rirs):
    spec = cx.MelSpec.kaldi(ctx)
    F = 12
    rv = cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS, method="fft")
    got, vf = speech.read_mel(SID, STARTS, F, spec, layout="ct", reverb=rv)
    Lm = int(spec.window_len(F))
    audio, v = speech.read(SID, STARTS, Lm, "ct", sample_rate=spec.sample_rate, channels=1, reverb=rv)
    direct, _ = speech.read(SID, STARTS, Lm, "ct", sample_rate=spec.sample_rate, channels=1, reverb=cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS))
    want = torch.empty_like(got)
    torch.cuda.synchronize()
    ctx.mel_windows(spec, audio.view(len(SID), Lm), v.numpy(), F, cx.WINDOW_CT, want)
    torch.cuda.synchronize()
    vf2 = spec.valid_frames(v.numpy(), F)
    spec.close()
    assert vf.tolist() == vf2.tolist() and not torch.equal(audio, direct)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_method_direct_is_the_call_without_the_argument(ctx, speech, rirs):
    a, va = speech.read(SID, STARTS, L, "tc", sample_rate=16000, channels=2, reverb=cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS, method="direct"))
    b, vb = speech.read(SID, STARTS, L, "tc", sample_rate=16000, channels=2, reverb=cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS))
    torch.cuda.synchronize()
    assert va.tolist() == vb.tolist() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    w1, w2 = _explicit(ctx, speech, rirs, "tc", 2, True, method="direct")[0], _explicit(ctx, speech, rirs, "tc", 2, True, method=None)[0]
    assert torch.equal(w1.view(torch.int32), w2.view(torch.int32)) and torch.equal(a.view(torch.int32), w1.view(torch.int32))
    assert TAPS < cx.REVERB_FFT_TAPS                          # method="auto" under the constant: the direct form's words
    c, vc = speech.read(SID, STARTS, L, "tc", sample_rate=16000, channels=2, reverb=cx.Reverb(RID, rirs, starts=RSTARTS, taps=TAPS, method="auto"))
    torch.cuda.synchronize()
    assert vc.tolist() == va.tolist() and torch.equal(c.view(torch.int32), a.view(torch.int32))
