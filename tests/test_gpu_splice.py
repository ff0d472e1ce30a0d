"""clx_splice_windows on the GPU: over the edge matrix of splice_cases.py the device's cells and guard bands equal the wave
simulator's word for word in both layouts and the input keeps its words; calls of growing and shrinking sizes queued back to back on
one stream without a sync, and on two streams, give what each gives alone; read_mel(..., splice=, normalize=, augment=) from FLAC
bytes -- a mono and a stereo stream, one of them resampled -- equals read_mel(...) followed by Context.splice_windows,
Context.norm_windows and Context.specaug_windows bit for bit, shapes and valid_frames' included; splice=None is the call without
the argument."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_splice as sp
import splice_cases as sc
from gpu_guarded import device_out, written
from test_gpu_norm import SID, STARTS, _pcm
from test_gpu_outside_features import _flac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _buffers(c, layout):
    """(input on the device, its host copy, flat guarded output, the slice of it the call may write)."""
    x = sc.data(c)
    host = sc.as_layout(x, layout)
    B, R, To = sc.out_shape(c)
    flat, body = device_out(B * R * To, offset_words=c["offset"])
    return torch.from_numpy(host).to(DEV), host, flat, body


def _queue(ctx, c, layout, src, body, stream=None):
    ctx.splice_windows((src.data_ptr(), len(c["valid"]), c["rows"], c["T"]), c["valid"], layout, sc.plan(c), out=body.data_ptr(), stream=stream)


def _same_as_simulator(c, layout, src, host, flat):
    B, R, To = sc.out_shape(c)
    cells = written(flat, B * R * To, (c["name"], layout), offset_words=c["offset"]).view(np.float32)
    cells = sc.from_layout(cells.reshape((B, To, R) if layout == sp.TC else (B, R, To)), layout)
    want = sc.simulated(c["name"], layout)
    assert sc.same_words(cells, want), (c["name"], layout, int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))
    assert sc.same_words(src.cpu().numpy(), host), (c["name"], layout, "the input was written")


@pytest.mark.parametrize("layout", (sp.CT, sp.TC))
@pytest.mark.parametrize("name", sc.NAMES)
def test_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = sc.case(name)
    src, host, flat, body = _buffers(c, layout)
    torch.cuda.synchronize()
    _queue(ctx, c, layout, src, body)
    torch.cuda.synchronize()
    _same_as_simulator(c, layout, src, host, flat)


ORDER = [("short", sp.CT), ("mixed", sp.TC), ("s6", sp.TC), ("sub64", sp.CT), ("rows256_m16", sp.TC), ("b1", sp.CT), ("rows80_lfr", sp.CT),
         ("copy_words", sp.TC)]


def test_calls_queued_back_to_back_on_one_stream(ctx):
    """Small, large (the table grows), small again (it is reused), TC and CT in turn, nothing waited for in between."""
    st = torch.cuda.Stream(device=DEV)
    bufs = [(sc.case(name), layout) + _buffers(sc.case(name), layout) for name, layout in ORDER]
    torch.cuda.synchronize()
    for c, layout, src, host, flat, body in bufs:
        _queue(ctx, c, layout, src, body, st)
    st.synchronize()
    for c, layout, src, host, flat, body in bufs:
        _same_as_simulator(c, layout, src, host, flat)


def test_calls_queued_on_two_streams(ctx):
    """The same calls dealt out to two streams in turn: every call finds the table it uploaded."""
    sts = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    bufs = [(sc.case(name), layout) + _buffers(sc.case(name), layout) for name, layout in ORDER + ORDER[::-1]]
    torch.cuda.synchronize()
    for i, (c, layout, src, host, flat, body) in enumerate(bufs):
        _queue(ctx, c, layout, src, body, sts[i % 2])
    for st in sts:
        st.synchronize()
    for c, layout, src, host, flat, body in bufs:
        _same_as_simulator(c, layout, src, host, flat)


@pytest.fixture(scope="module")
def streams(ctx):
    """A mono stream at 16 kHz and a stereo one at 8 kHz (resampled when read at 16 kHz)."""
    s = cx.open_streams(ctx, [_flac(_pcm(5000, 1, 11), 16000), _flac(_pcm(3000, 2, 12), 8000)])
    assert s.problems == [None, None]
    return s


FRAMES = 24


def _plan(vf, rows):
    """A fixed SpecAugment plan for the spliced batch: a warp where the window is long enough, masks that reach past V and the rows."""
    warp = np.array([(V // 2, V // 2 + 1) if V >= 4 else (0, 0) for V in vf])
    fm = np.array([[(3, 4), (rows - 2, 9)]] * len(vf))
    tm = np.array([[(1, 1), (max(V - 1, 0), 5)] for V in vf])
    return cx.SpecAugmentPlan(warp, fm, tm, 0.0)


def _two_routes(ctx, streams, spec, layout, splice, augment):
    """read_mel with everything at once, and read_mel followed by the three window calls: (got, vf', want, plain, vf)."""
    N, L = cx.Norm.cmvn(), cx._LAYOUTS[layout]
    plain, vf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout)
    vf2 = splice.frames_out(vf.numpy())
    aug = _plan(vf2.tolist(), splice.n_out(spec.n_out)) if augment else None
    got, gvf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, splice=splice, normalize=N, augment=aug)
    torch.cuda.synchronize()
    host = plain.cpu().numpy().copy()
    want = ctx.splice_windows(plain, vf.numpy(), L, splice)
    torch.cuda.synchronize()
    assert sc.same_words(plain.cpu().numpy(), host)          # (the step is out of place)
    sim = sp.splice_windows(host, np.empty(tuple(want.shape), dtype=np.float32), vf.numpy(), L, splice)
    assert sc.same_words(want.cpu().numpy(), sim)
    ctx.norm_windows(want, vf2, L, N)
    if augment:
        want = ctx.specaug_windows(want, vf2, L, aug.warp, aug.freq_masks, aug.time_masks, aug.fill)
    torch.cuda.synchronize()
    assert gvf.tolist() == vf2.tolist() and gvf.dtype == vf.dtype
    R, To = splice.n_out(spec.n_out), splice.frames_out(FRAMES)
    assert tuple(got.shape) == ((len(SID), R, To) if layout == "ct" else (len(SID), To, R)) == tuple(want.shape)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    return got, gvf, vf


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("augment", (False, True))
def test_read_mel_lfr_cmvn_is_the_three_calls(ctx, streams, layout, augment):
    spec = cx.MelSpec.kaldi(ctx, n_mels=23)                  # (7 x 23 = 161 rows: CMVN and SpecAugment take 256 at most)
    got, gvf, vf = _two_routes(ctx, streams, spec, layout, cx.Splice.lfr(), augment)
    spec.close()
    assert 0 in vf.tolist() and FRAMES in vf.tolist() and gvf.tolist() == [-(-v // 6) for v in vf.tolist()] and got.shape[1 if layout == "ct" else 2] == 161


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("augment", (False, True))
def test_read_mel_mfcc_deltas_cmvn_is_the_three_calls(ctx, streams, layout, augment):
    spec = cx.MelSpec.mfcc(ctx)
    got, gvf, vf = _two_routes(ctx, streams, spec, layout, cx.Splice.deltas(), augment)
    spec.close()
    assert gvf.tolist() == vf.tolist() and got.shape[1 if layout == "ct" else 2] == 39


def test_splice_none_is_the_call_without_the_argument(ctx, streams):
    spec = cx.MelSpec.kaldi(ctx)
    N = cx.Norm.cmvn()
    a, va = streams.read_mel(SID, STARTS, FRAMES, spec, normalize=N)
    b, vb = streams.read_mel(SID, STARTS, FRAMES, spec, normalize=N, splice=None)
    torch.cuda.synchronize()
    assert va.tolist() == vb.tolist() and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    # 560 rows are spliced; the CMVN behind them is refused by clx_norm_windows, in its own words
    c, vc = streams.read_mel(SID, STARTS, FRAMES, spec, splice=cx.Splice.lfr())
    torch.cuda.synchronize()
    assert tuple(c.shape) == (len(SID), 560, 4) and vc.tolist() == [-(-v // 6) for v in va.tolist()]
    with pytest.raises(cx.ClaxonError, match="clx_norm_windows: rows must be 1..256"):
        streams.read_mel(SID, STARTS, FRAMES, spec, splice=cx.Splice.lfr(), normalize=N)
    with pytest.raises(ValueError, match="read_mel: splice must be a Splice or None"):
        streams.read_mel(SID, STARTS, FRAMES, spec, splice="lfr")
    torch.cuda.synchronize()
    spec.close()
