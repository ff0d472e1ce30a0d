"""clx_specaug_windows on the GPU: over the edge matrix of specaug_cases.py the device's cells, fills and guard bands equal the wave
simulator's word for word in both layouts; calls of different sizes queued back to back on one stream without a sync (tables
growing and reused) give what each gives alone; read_mel(..., augment=plan) from FLAC bytes -- a mono and a stereo stream, one of
them resampled, Kaldi fbank with CMVN -- equals read_mel(...) followed by Context.specaug_windows bit for bit, and the simulator on
the same batch; augment=None is the call without the argument; and a policy is the plan its draw gives."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_specaug as ss
import specaug_cases as sc
from gpu_guarded import device_out, written
from test_gpu_norm import SID, STARTS, _pcm
from test_gpu_outside_features import _flac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _launch(ctx, c, layout, stream=None):
    """The case queued on the device: (input, its host copy, flat output, flat fills) to be read back with _collect."""
    x = sc.data(c)
    B = x.shape[0]
    host = sc.as_layout(x, layout)
    src = torch.from_numpy(host).to(DEV)
    flat, body = device_out(x.size, offset_words=c["offset"])
    fflat, fbody = device_out(B, offset_words=1)
    torch.cuda.synchronize()                                 # (the fills first: the launches may go to another stream)
    ctx.specaug_windows((src.data_ptr(), B, c["rows"], c["T"]), c["valid"], layout, c["warp"], c["fm"], c["tm"], c["fill"],
                        out=body.data_ptr(), fills=fbody.data_ptr(), stream=stream)
    return src, host, flat, fflat


def _same_as_simulator(c, layout, src, host, flat, fflat):
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    cells = written(flat, B * rows * T, (c["name"], layout), offset_words=c["offset"]).view(np.float32)
    cells = sc.from_layout(cells.reshape((B, T, rows) if layout == ss.TC else (B, rows, T)), layout)
    fills = written(fflat, B, (c["name"], layout, "fills"), offset_words=1).view(np.float32)
    want, wfills = sc.simulated(c["name"], layout)
    assert sc.same_words(cells, want), (c["name"], layout, "cells", int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))
    assert sc.same_words(fills, wfills), (c["name"], layout, "fills")
    assert sc.same_words(src.cpu().numpy(), host), (c["name"], layout, "the input was written")


@pytest.mark.parametrize("layout", (ss.CT, ss.TC))
@pytest.mark.parametrize("name", sc.NAMES)
def test_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = sc.case(name)
    bufs = _launch(ctx, c, layout)
    torch.cuda.synchronize()
    _same_as_simulator(c, layout, *bufs)


def test_calls_queued_back_to_back_on_one_stream(ctx):
    """Small, large (both tables grow), small again (both are reused), TC and CT, the mean and a constant in turn, nothing waited for
    in between."""
    st = torch.cuda.Stream(device=DEV)
    order = [("short", ss.CT), ("masks32", ss.TC), ("ends", ss.TC), ("mean_chunks", ss.CT), ("rows256", ss.TC), ("masks", ss.CT), ("ends", ss.CT)]
    bufs = []
    for name, layout in order:
        c = sc.case(name)
        x = sc.data(c)
        host = sc.as_layout(x, layout)
        flat, body = device_out(x.size, offset_words=c["offset"])
        fflat, fbody = device_out(x.shape[0], offset_words=1)
        bufs.append((c, layout, torch.from_numpy(host).to(DEV), host, flat, body, fflat, fbody))
    torch.cuda.synchronize()
    for c, layout, src, host, flat, body, fflat, fbody in bufs:
        ctx.specaug_windows((src.data_ptr(), len(c["valid"]), c["rows"], c["T"]), c["valid"], layout, c["warp"], c["fm"], c["tm"], c["fill"],
                            out=body.data_ptr(), fills=fbody.data_ptr(), stream=st)
    st.synchronize()
    for c, layout, src, host, flat, body, fflat, fbody in bufs:
        _same_as_simulator(c, layout, src, host, flat, fflat)


@pytest.fixture(scope="module")
def streams(ctx):
    """A mono stream at 16 kHz and a stereo one at 8 kHz (resampled when read at 16 kHz)."""
    s = cx.open_streams(ctx, [_flac(_pcm(5000, 1, 11), 16000), _flac(_pcm(3000, 2, 12), 8000)])
    assert s.problems == [None, None]
    return s


FRAMES = 24


def _plan(vf, rows, fill):
    """A plan by hand for the call's valid_frames: a warp wherever the window is long enough, masks that reach past V and the rows."""
    B = len(vf)
    warp = np.array([(V // 2, V // 2 + 2) if V >= 6 else (0, 0) for V in vf])
    fm = np.array([[(3, 4), (rows - 2, 9)]] * B)
    tm = np.array([[(1, 2), (max(V - 1, 0), 5), (0, 0)] for V in vf])
    return cx.SpecAugmentPlan(warp, fm, tm, fill)


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("fill", ("mean", 0.0))
def test_read_mel_augment_is_read_mel_then_specaug_windows(ctx, streams, layout, fill):
    spec = cx.MelSpec.kaldi(ctx)
    N = cx.Norm.cmvn()
    plain, vf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, normalize=N)
    none, vf0 = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, normalize=N, augment=None)
    plan = _plan(vf.tolist(), spec.n_out, fill)
    got, vf2 = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, normalize=N, augment=plan)
    torch.cuda.synchronize()
    assert vf.tolist() == vf0.tolist() == vf2.tolist() and 0 in vf.tolist() and FRAMES in vf.tolist() and any(plan.warp[:, 0] > 0)
    assert torch.equal(plain.view(torch.int32), none.view(torch.int32))
    host = plain.cpu().numpy().copy()
    two = ctx.specaug_windows(plain, vf.numpy(), cx._LAYOUTS[layout], plan.warp, plan.freq_masks, plan.time_masks, plan.fill)
    torch.cuda.synchronize()
    spec.close()
    assert got.shape == plain.shape and got.data_ptr() != plain.data_ptr()
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    assert sc.same_words(plain.cpu().numpy(), host)          # (the step is out of place)
    sim = ss.specaug_windows(host, np.empty_like(host), vf.numpy(), cx._LAYOUTS[layout], plan.warp, plan.freq_masks, plan.time_masks, plan.fill)
    g = got.cpu().numpy()
    assert sc.same_words(g, sim)
    g, h = (g, host) if layout == "ct" else (g.transpose(0, 2, 1), host.transpose(0, 2, 1))
    for k, V in enumerate(vf.tolist()):
        assert np.array_equal(g[k, :, V:].view(np.uint32), h[k, :, V:].view(np.uint32))        # dead frames keep their words
        if V >= 6 and fill == 0.0:
            assert np.all(g[k, 3:7, :V] == 0) and np.all(g[k, :, 1:3] == 0) and np.all(g[k, :, V - 1] == 0) and np.any(g[k, :, 3:V - 1] != 0)


def test_a_policy_is_the_plan_its_draw_gives(ctx, streams):
    spec = cx.MelSpec.kaldi(ctx)
    kw = dict(time_warp=3, freq_masks=2, freq_width=10, time_masks=3, time_width=6, max_time_fraction=0.5, p=1.0, fill="mean")
    got, vf = streams.read_mel(SID, STARTS, FRAMES, spec, augment=cx.SpecAugment(seed=7, **kw))
    plan = cx.SpecAugment(seed=7, **kw).draw(vf.numpy(), spec.n_out)
    want, vf2 = streams.read_mel(SID, STARTS, FRAMES, spec, augment=plan)
    plain, _ = streams.read_mel(SID, STARTS, FRAMES, spec)
    torch.cuda.synchronize()
    spec.close()
    assert vf.tolist() == vf2.tolist() and plan.warp.any() and plan.time_masks[..., 1].any()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not torch.equal(got.view(torch.int32), plain.view(torch.int32))


def test_read_mel_refuses_a_plan_that_does_not_fit(ctx, streams):
    spec = cx.MelSpec.kaldi(ctx)
    B, z = len(SID), np.zeros((len(SID), 1, 2), dtype=np.int64)
    bad = [cx.SpecAugmentPlan(np.zeros((B + 1, 2)), np.zeros((B + 1, 1, 2)), np.zeros((B + 1, 1, 2))),
           cx.SpecAugmentPlan(np.zeros((B, 2)), z + [[spec.n_out, 1]], z),
           cx.SpecAugmentPlan(np.zeros((B, 2)), z, z + [[FRAMES + 1, 1]]),
           cx.SpecAugmentPlan(np.full((B, 2), FRAMES), z, z)]
    for plan in bad:
        with pytest.raises(ValueError, match="augment"):
            streams.read_mel(SID, STARTS, FRAMES, spec, augment=plan)
    # masks of width 0 wherever they start, and masks that run past the rows and the frames, are what specaug_windows accepts
    fine = cx.SpecAugmentPlan(np.zeros((B, 2)), z + [[spec.n_out, 0]], np.concatenate([z + [[FRAMES + 9, 0]], z + [[FRAMES - 1, 50]]], axis=1), 0.0)
    got, vf = streams.read_mel(SID, STARTS, FRAMES, spec, augment=fine)
    plain, _ = streams.read_mel(SID, STARTS, FRAMES, spec)
    torch.cuda.synchronize()
    g, h = got.cpu().numpy(), plain.cpu().numpy()
    for k, V in enumerate(vf.tolist()):
        assert np.array_equal(g[k, :, :FRAMES - 1], h[k, :, :FRAMES - 1]) and np.all(g[k, :, FRAMES - 1] == (0 if V == FRAMES else h[k, :, FRAMES - 1]))
    spec.close()
