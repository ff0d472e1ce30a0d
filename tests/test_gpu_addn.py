"""clx_addn_windows on the GPU: over the edge matrix of addn_cases.py the device's cells, gains and guard bands equal the wave
simulator's word for word in both layouts and the noises keep every word; calls queued back to back on one stream without a sync
(tables growing and reused), and interleaved on two streams, give what they give alone; read(..., add=[...]) and
read_mel(..., add=[...]) from FLAC bytes -- mono and stereo, the set as its own source plus a separate one, a looped 1000-sample
noise, three babble terms, two foreground terms at offsets, ids of -1 -- equal the reads + Context.addn_windows (+ mel_windows) bit
for bit, and the simulator on the same batches; a plain Add alone is that Add in a list, word for word."""
import numpy as np
import pytest
import torch

import addn_cases as dc
import claxon_amd as cx
import simlib_addn as sd
from gpu_guarded import device_out, written
from test_gpu_add import _pcm
from test_gpu_outside_features import _flac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _stage(c, layout):
    """The case's buffers on the device, filled: to be launched with _launch and read back with _collect."""
    x, noises = dc.data(c)
    flat, body = device_out(x.size, offset_words=c["offset"])
    body.copy_(torch.from_numpy(dc.as_layout(x, layout).reshape(-1)))
    nbufs = []
    for n, off in zip(noises, c["noise_offsets"]):
        nflat, nbody = device_out(n.size, offset_words=off)
        nbody.copy_(torch.from_numpy(dc.as_layout(n, layout).reshape(-1)))
        nbufs.append((nflat, nbody, n))
    first, terms = sd.flatten(c["terms"])
    gflat, gbody = device_out(int(first[-1]), offset_words=1)
    return dict(c=c, layout=layout, shape=x.shape, flat=flat, body=body, nbufs=nbufs, first=first, terms=terms, gflat=gflat, gbody=gbody)


def _launch(ctx, s, stream=None):
    c, terms = s["c"], s["terms"]
    ctx.addn_windows((s["body"].data_ptr(),) + tuple(s["shape"]), c["valid"], [(nb.data_ptr(), n.shape[0]) for _, nb, n in s["nbufs"]],
                     np.concatenate([np.asarray(v, dtype=np.uint32) for v in c["noise_valid"]]), s["first"], terms["batch"], terms["index"],
                     terms["offset"], terms["loop"], terms["snr_db"], s["layout"], gains=s["gbody"].data_ptr(), stream=stream)


def _collect(s):
    c, layout = s["c"], s["layout"]
    B, rows, T = s["shape"]
    cells = written(s["flat"], B * rows * T, (c["name"], layout), offset_words=c["offset"]).view(np.float32)
    cells = dc.from_layout(cells.reshape((B, T, rows) if layout == sd.TC else (B, rows, T)), layout)
    for (nflat, _, n), off in zip(s["nbufs"], c["noise_offsets"]):
        noise = written(nflat, n.size, (c["name"], layout, "noise"), offset_words=off).view(np.float32)
        assert dc.same_words(noise, dc.as_layout(n, layout).reshape(-1)), (c["name"], layout, "a noise batch was written")
    gains = written(s["gflat"], int(s["first"][-1]), (c["name"], layout, "gains"), offset_words=1).view(np.float32)
    return cells, gains


def _same_as_simulator(s):
    c, layout = s["c"], s["layout"]
    cells, gains = _collect(s)
    want, wgains = dc.simulated(c["name"], layout)
    assert dc.same_words(gains, wgains), (c["name"], layout, "gains", gains, wgains)
    assert dc.same_words(cells, want), (c["name"], layout, "cells", int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))


@pytest.mark.parametrize("layout", (sd.CT, sd.TC))
@pytest.mark.parametrize("name", dc.NAMES)
def test_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    s = _stage(dc.case(name), layout)
    torch.cuda.synchronize()                                 # (the fills first: the launches may go to another stream)
    _launch(ctx, s)
    torch.cuda.synchronize()
    _same_as_simulator(s)


ORDER = [("dead_between", sd.CT), ("T8195_rows3", sd.TC), ("disjoint", sd.TC), ("T8195_rows3", sd.CT), ("T65_rows2", sd.CT), ("offsets_1_2", sd.TC)]


def test_calls_queued_back_to_back_on_one_stream(ctx):
    """Small, large (both tables grow), small again (both are reused), TC and CT in turn, nothing waited for in between."""
    st = torch.cuda.Stream(device=DEV)
    staged = [_stage(dc.case(name), layout) for name, layout in ORDER]
    torch.cuda.synchronize()
    for s in staged:
        _launch(ctx, s, stream=st)
    st.synchronize()
    for s in staged:
        _same_as_simulator(s)


def test_calls_interleaved_on_two_streams(ctx):
    """The same sequence, its calls going to two streams in turn, and once more the other way round."""
    a, b = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    staged = [_stage(dc.case(name), layout) for name, layout in ORDER + ORDER[::-1]]
    torch.cuda.synchronize()
    for i, s in enumerate(staged):
        _launch(ctx, s, stream=(a, b)[i % 2])
    a.synchronize()
    b.synchronize()
    for s in staged:
        _same_as_simulator(s)


@pytest.fixture(scope="module")
def speech(ctx):
    """Stream 0: mono, 16 kHz, 5000 samples.  1: stereo, 16 kHz, 3000.  2: mono, 16 kHz, 1000 (the noise the set loops over itself)."""
    s = cx.open_streams(ctx, [_flac(_pcm(5000, 1, 41, 300.0), 16000), _flac(_pcm(3000, 2, 42, 170.0), 16000), _flac(_pcm(1000, 1, 43, 90.0), 16000)])
    assert s.problems == [None] * 3
    return s


@pytest.fixture(scope="module")
def noises(ctx):
    """A separate source.  Stream 0: stereo, 16 kHz, 4000 samples.  1: mono, 16 kHz, 1000.  2: mono, 8 kHz, 1500 (3000 at 16 kHz)."""
    s = cx.open_streams(ctx, [_flac(_pcm(4000, 2, 51, 1100.0), 16000), _flac(_pcm(1000, 1, 52, 700.0), 16000), _flac(_pcm(1500, 1, 53, 2300.0), 8000)])
    assert s.problems == [None] * 3
    return s


SID, STARTS = [0, 1, 0, 2], [0, 100, 3500, 0]                # a whole window, two that run off their streams, a short stream


def _recipe(noises, L):
    """Music: the set's own 1000-sample stream looped under three windows.  Babble: three speakers of the separate source, each at
    its own snr.  Foreground: two 1000-sample noises dropped in at offsets.  Ids of -1 throughout."""
    return [cx.Add([2, 2, 2, -1], [0, 0, 200, 0], 10.0, tile=True),
            cx.Add([0, 0, 1, 0], [0, 500, 0, 1000], 5.0, source=noises),
            cx.Add([2, 2, -1, 1], [100, 0, 0, 0], [8.0, 9.0, 0.0, 7.0], source=noises),
            cx.Add([1, 0, 2, 2], [0, 3000, 2500, 0], 12.0, source=noises),
            cx.Add([1, 1, 1, -1], [0, 0, 0, 0], 3.0, source=noises, offsets=[300, L - 500, 100, 0]),
            cx.Add([1, -1, 1, 1], [0, 0, 500, 0], 0.0, source=noises, offsets=[1500, 0, L - 1, 700])]


def _by_hand(ctx, sset, noises, adds, L, layout, channels, audio, v):
    """The reads and the Context.addn_windows call that read(add=[...]) stands for, on `audio`: (gains [B, S], the batch before on
    the host, the noise batches on the host, noise_valids, the per-window term lists)."""
    B, S = len(SID), len(adds)
    own = [s for s, a in enumerate(adds) if a.source is None]
    sep = [s for s, a in enumerate(adds) if a.source is noises]
    batches, nvs, terms = [], [], [[None] * S for _ in range(B)]
    for b, (src, mine) in enumerate(((sset, own), (noises, sep))):
        ids, sts, at = [], [], 0
        for s in mine:
            for k in range(B):
                j = int(adds[s].stream_ids[k])
                terms[k][s] = (b, at if j >= 0 else -1, min(int(adds[s].offsets[k]), L), int(adds[s].tile[k]), float(adds[s].snr_db[k]))
                if j >= 0:
                    ids.append(j)
                    sts.append(int(adds[s].starts[k]))
                    at += 1
        noise, nv = src.read(ids, sts, L, layout, sample_rate=16000, channels=channels)
        batches.append(noise)
        nvs.append(nv.numpy())
    gains = torch.full((B, S), -1.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()                                 # (the fill first: it runs on torch's stream, the call on the context's)
    host, nhosts = audio.cpu().numpy().copy(), [n.cpu().numpy().copy() for n in batches]
    first, flat = sd.flatten(terms)
    ctx.addn_windows(audio, v.numpy(), batches, np.concatenate(nvs), first, flat["batch"], flat["index"], flat["offset"], flat["loop"], flat["snr_db"],
                     cx._LAYOUTS[layout], gains=gains)
    torch.cuda.synchronize()
    for n, h in zip(batches, nhosts):
        assert torch.equal(n.cpu().view(torch.int32), torch.from_numpy(h).view(torch.int32))
    return gains, host, nhosts, nvs, terms


@pytest.mark.parametrize("layout", ("tc", "ct"))
@pytest.mark.parametrize("channels", (1, 2))
def test_read_add_list_is_the_reads_and_one_addn_windows(ctx, speech, noises, channels, layout):
    L = 2500
    adds = _recipe(noises, L)
    f0, n0 = speech.frames_decoded, noises.frames_decoded
    got, v, g = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels, add=adds, return_gains=True)
    torch.cuda.synchronize()                                 # (before torch allocates again: the call's noise batches are free by now)
    f1, n1 = speech.frames_decoded, noises.frames_decoded
    two, v2 = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels)
    g2, host, nhosts, nvs, terms = _by_hand(ctx, speech, noises, adds, L, layout, channels, two, v2)
    assert f1 - f0 == speech.frames_decoded - f1 and n1 - n0 == noises.frames_decoded - n1 > 0      # (one read a source, both times)
    assert v.tolist() == v2.tolist() and L in v.tolist() and any(0 < n < L for n in v.tolist())
    assert tuple(g.shape) == (len(SID), len(adds)) and torch.equal(g.view(torch.int32), g2.view(torch.int32))
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    gh = g.cpu().numpy()
    none = np.array([[a.stream_ids[k] < 0 for a in adds] for k in range(len(SID))])
    assert np.all(gh[none] == 0) and np.all(gh[~none & (v2.numpy()[:, None] > np.array([[min(int(a.offsets[k]), L) for a in adds] for k in range(len(SID))]))] > 0)
    assert 1000 in nvs[0].tolist() and any(t[3] for w in terms for t in w)             # the looped noise has its 1000 samples
    sgains = np.zeros(gh.size, dtype=np.float32)
    first, flat = sd.flatten(terms)
    assert sd.addn_windows(host, v.numpy(), nhosts, np.concatenate(nvs), first, flat, cx._LAYOUTS[layout], sgains)
    assert dc.same_words(got.cpu().numpy(), host) and dc.same_words(gh.reshape(-1), sgains)
    pair = speech.read(SID, STARTS, L, layout, sample_rate=16000, channels=channels, add=adds)
    torch.cuda.synchronize()                                 # (the launches go to the context's stream, the comparison to torch's)
    assert len(pair) == 2 and torch.equal(pair[0].view(torch.int32), got.view(torch.int32))


def test_read_mel_add_list_is_the_features_of_the_mixed_waveform(ctx, speech, noises):
    spec = cx.MelSpec.kaldi(ctx)
    F = 12
    Lm = int(spec.window_len(F))
    adds = _recipe(noises, Lm)
    got, vf = speech.read_mel(SID, STARTS, F, spec, layout="ct", add=adds)
    audio, v = speech.read(SID, STARTS, Lm, "ct", sample_rate=spec.sample_rate, channels=1)
    torch.cuda.synchronize()                                 # (the copy runs on torch's stream, the reads on the context's)
    clean = audio.clone()
    _by_hand(ctx, speech, noises, adds, Lm, "ct", 1, audio, v)
    want = torch.empty_like(got)
    ctx.mel_windows(spec, audio.view(len(SID), Lm), v.numpy(), F, cx.WINDOW_CT, want)
    torch.cuda.synchronize()
    spec.close()
    assert vf.tolist() == spec.valid_frames(v.numpy(), F).tolist() and not torch.equal(audio, clean)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("layout", ("tc", "ct"))
def test_a_plain_add_alone_is_that_add_in_a_list(speech, noises, layout):
    """The one goes through clx_add_windows, the other through clx_addn_windows: the same words; gains [B] against [B, 1].  And an
    Add with an offset or a tile, alone, keeps [B]."""
    add = cx.Add([0, 2, -1, 1], [700, 0, 0, 0], [10.0, 0.0, 3.0, -5.0], source=noises)
    a, va, ga = speech.read(SID, STARTS, 2500, layout, sample_rate=16000, channels=2, add=add, return_gains=True)
    b, vb, gb = speech.read(SID, STARTS, 2500, layout, sample_rate=16000, channels=2, add=[add], return_gains=True)
    placed = cx.Add([0, 2, -1, 1], [700, 0, 0, 0], [10.0, 0.0, 3.0, -5.0], source=noises, offsets=[0, 0, 0, 0], tile=[False, True, False, False])
    c, vc, gc = speech.read(SID, STARTS, 2500, layout, sample_rate=16000, channels=2, add=placed, return_gains=True)
    torch.cuda.synchronize()
    assert tuple(ga.shape) == (4,) and tuple(gb.shape) == (4, 1) and tuple(gc.shape) == (4,)
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32).reshape(-1)) and ga.cpu().tolist()[2] == 0
    assert va.tolist() == vb.tolist() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    # (window 1's noise, 3000 samples at 16 kHz, covers its 2500 samples looped or not; the others are not looped)
    assert torch.equal(c.view(torch.int32), a.view(torch.int32)) and torch.equal(gc.view(torch.int32), ga.view(torch.int32))


def test_a_source_that_no_window_names_is_not_read(speech, noises):
    """An Add that is -1 throughout, on a separate source whose streams differ in channel count, beside a live Add, at the native
    rate and channel count: the source is not read (an empty read there would have no channel count to give), the call is the one
    without that Add, and its gains are 0."""
    sid, st = [0, 2], [0, 0]
    live = cx.Add([2, 0], [0, 1000], 6.0, offsets=[100, 0])
    f0 = noises.frames_decoded
    a, va, ga = speech.read(sid, st, 1500, "ct", add=[live, cx.Add([-1, -1], [0, 0], 3.0, source=noises, tile=True)], return_gains=True)
    b, vb, gb = speech.read(sid, st, 1500, "ct", add=[live], return_gains=True)
    torch.cuda.synchronize()
    assert noises.frames_decoded == f0 and va.tolist() == vb.tolist()
    assert tuple(ga.shape) == (2, 2) and torch.equal(ga[:, :1].contiguous().view(torch.int32), gb.view(torch.int32))
    assert ga[:, 1].cpu().tolist() == [0.0, 0.0] and bool((gb > 0).all())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
