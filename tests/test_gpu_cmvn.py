"""clx_cmvn_global_windows and clx_cmvn_sliding_windows on the GPU: over a subset of cmvn_cases.py -- both kernels, both layouts,
both center values, norm_vars on and off, the three-tile T, the row chunk's edges, 560 and 8192 rows -- the device's cells and guard
words equal the wave simulator's word for word and the sliding input keeps its words; calls whose tables grow, queued back to
back on one stream and on two, give what the same call gives alone on a fresh context; read_mel(splice=Splice.lfr(), cmvn=global)
on MelSpec.kaldi and read_mel(cmvn=Cmvn.xvector()) on MelSpec.mfcc equal read_mel followed by Context.cmvn_windows bit for bit;
read_mel's ValueErrors.  Every comparison stands behind a synchronise."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import cmvn_cases as cc
import simlib_cmvn as sc
from gpu_guarded import device_out, written
from test_gpu_norm import SID, STARTS, _pcm
from test_gpu_outside_features import _flac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = (sc.CT, sc.TC)


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _cmvn(c):
    return cx.Cmvn.sliding(c["N"], c["M"], bool(c["center"]), bool(c["norm_vars"]), pad=c["pad"])


def _sliding_buffers(c, layout):
    x = cc.data(c)
    host = cc.as_layout(x, layout)
    flat, body = device_out(x.size, offset_words=c["offset"])
    return torch.from_numpy(host).to(DEV), host, flat, body


def _sliding_queue(ctx, c, layout, src, body, stream=None):
    ctx.cmvn_windows((src.data_ptr(), len(c["valid"]), c["rows"], c["T"]), c["valid"], layout, _cmvn(c), out=body.data_ptr(), stream=stream)


def _cells(c, layout, flat):
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    cells = written(flat, B * rows * T, (c["name"], layout), offset_words=c["offset"]).view(np.float32)
    return cc.from_layout(cells.reshape((B, T, rows) if layout == sc.TC else (B, rows, T)), layout)


def _sliding_same(c, layout, src, host, flat, want=None):
    cells = _cells(c, layout, flat)
    want = cc.simulated_sliding(c["name"], layout) if want is None else want
    if c["kind"] == "nonfinite":
        # IEEE says where a NaN comes out, not which: the host's and the device's differ in sign and payload.  The same cells are
        # NaN, and every other word is equal.
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(cells), nan) and 0 < np.count_nonzero(nan) < nan.size // 2, (c["name"], layout)
        cells, want = np.where(nan, np.float32(0), cells), np.where(nan, np.float32(0), want)
    assert cc.same_words(cells, want), (c["name"], layout, int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))
    assert cc.same_words(src.cpu().numpy(), host), (c["name"], layout, "the input was written")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", cc.GPU_SLIDING)
def test_sliding_on_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = cc.sliding_case(name)
    src, host, flat, body = _sliding_buffers(c, layout)
    torch.cuda.synchronize()
    _sliding_queue(ctx, c, layout, src, body)
    torch.cuda.synchronize()
    _sliding_same(c, layout, src, host, flat)


def _global_buffers(c, layout):
    x, shift, scale = cc.global_data(c)
    flat, body = device_out(x.size, offset_words=c["offset"])
    body.copy_(torch.from_numpy(cc.as_layout(x, layout).reshape(-1)))
    return flat, body, cx.Cmvn.global_(shift, scale, pad=c["pad"])


def _global_queue(ctx, c, layout, body, cmvn, stream=None):
    ctx.cmvn_windows((body.data_ptr(), len(c["valid"]), c["rows"], c["T"]), c["valid"], layout, cmvn, stream=stream)


def _global_same(c, layout, flat, want=None):
    cells = _cells(c, layout, flat)
    want = cc.simulated_global(c["name"], layout) if want is None else want
    assert cc.same_words(cells, want), (c["name"], layout, int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", cc.GLOBAL_NAMES)
def test_global_on_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = cc.global_case(name)
    flat, body, cmvn = _global_buffers(c, layout)
    torch.cuda.synchronize()
    _global_queue(ctx, c, layout, body, cmvn)
    torch.cuda.synchronize()
    _global_same(c, layout, flat)


# small tables first, then ones that grow (8192 rows: 16 387 words; six windows), then small again: ("g" | "s", case, layout)
ORDER = [("s", "wide_c1_v1", sc.CT), ("g", "g_b1", sc.CT), ("g", "g_rows560", sc.TC), ("s", "N300_c0_v1_a", sc.TC), ("g", "g_rows8192", sc.CT),
         ("s", "rows80", sc.TC), ("g", "g_rows13", sc.TC), ("s", "xvector", sc.CT)]


def _alone(kind, name, layout):
    """The call made alone on a context that has made no other, synchronised before and after: its cells."""
    fresh = cx.Context(0, wait_s=120)
    try:
        if kind == "s":
            c = cc.sliding_case(name)
            src, host, flat, body = _sliding_buffers(c, layout)
            torch.cuda.synchronize()
            _sliding_queue(fresh, c, layout, src, body)
        else:
            c = cc.global_case(name)
            flat, body, cmvn = _global_buffers(c, layout)
            torch.cuda.synchronize()
            _global_queue(fresh, c, layout, body, cmvn)
        torch.cuda.synchronize()
        return _cells(c, layout, flat)
    finally:
        fresh.close()


def _queued(order, streams):
    ctx = cx.Context(0, wait_s=120)
    try:
        made = []
        for kind, name, layout in order:
            if kind == "s":
                c = cc.sliding_case(name)
                made.append((kind, c, layout) + _sliding_buffers(c, layout))
            else:
                c = cc.global_case(name)
                made.append((kind, c, layout) + _global_buffers(c, layout))
        torch.cuda.synchronize()
        for i, m in enumerate(made):
            st = streams[i % len(streams)]
            if m[0] == "s":
                _sliding_queue(ctx, m[1], m[2], m[3], m[6], st)
            else:
                _global_queue(ctx, m[1], m[2], m[4], m[5], st)
        for st in streams:
            st.synchronize()
        torch.cuda.synchronize()
        for m in made:
            want = _alone(m[0], m[1]["name"], m[2])
            if m[0] == "s":
                _sliding_same(m[1], m[2], m[3], m[4], m[5], want)
            else:
                _global_same(m[1], m[2], m[3], want)
    finally:
        ctx.close()


def test_calls_whose_tables_grow_queued_back_to_back_on_one_stream():
    _queued(ORDER, [torch.cuda.Stream(device=DEV)])


def test_calls_whose_tables_grow_queued_on_two_streams():
    _queued(ORDER + ORDER[::-1], [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)])


@pytest.fixture(scope="module")
def streams(ctx):
    """A mono stream at 16 kHz and a stereo one at 8 kHz (resampled when read at 16 kHz)."""
    s = cx.open_streams(ctx, [_flac(_pcm(5000, 1, 11), 16000), _flac(_pcm(3000, 2, 12), 8000)])
    assert s.problems == [None, None]
    return s


FRAMES = 24


@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_read_mel_lfr_global_cmvn_is_read_mel_then_cmvn_windows(ctx, streams, layout):
    rng = np.random.default_rng(7)
    cmvn = cx.Cmvn.global_(rng.uniform(3, 9, 560), rng.uniform(0.1, 0.5, 560), pad=-2.0)
    spec, L = cx.MelSpec.kaldi(ctx), cx._LAYOUTS[layout]
    got, gvf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, splice=cx.Splice.lfr(), cmvn=cmvn)
    want, vf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, splice=cx.Splice.lfr())
    torch.cuda.synchronize()
    host = want.cpu().numpy().copy()
    assert ctx.cmvn_windows(want, vf.numpy(), L, cmvn) is want
    torch.cuda.synchronize()
    spec.close()
    assert gvf.tolist() == vf.tolist() and 0 in vf.tolist() and max(vf.tolist()) == 4
    assert tuple(got.shape) == tuple(want.shape) == ((len(SID), 560, 4) if layout == "ct" else (len(SID), 4, 560))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    sim = sc.global_windows(host, vf.numpy(), L, cmvn.shift, cmvn.scale, cmvn.pad)
    assert cc.same_words(want.cpu().numpy(), sim)


@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_read_mel_mfcc_xvector_cmvn_is_read_mel_then_cmvn_windows(ctx, streams, layout):
    cmvn = cx.Cmvn.xvector(pad=1.0)
    spec, L = cx.MelSpec.mfcc(ctx), cx._LAYOUTS[layout]
    got, gvf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, cmvn=cmvn)
    plain, vf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout)
    torch.cuda.synchronize()
    host = plain.cpu().numpy().copy()
    want = ctx.cmvn_windows(plain, vf.numpy(), L, cmvn)
    torch.cuda.synchronize()
    spec.close()
    assert want is not plain and cc.same_words(plain.cpu().numpy(), host)        # (the step is out of place)
    assert gvf.tolist() == vf.tolist() and tuple(got.shape) == tuple(plain.shape)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    sim = sc.sliding_windows(host, np.empty_like(host), vf.numpy(), L, 300, 100, 1, 0, 1.0)
    assert cc.same_words(want.cpu().numpy(), sim)


def test_read_mel_refuses_what_it_should_and_none_is_the_call_without(ctx, streams):
    spec = cx.MelSpec.kaldi(ctx)
    a, va = streams.read_mel(SID, STARTS, FRAMES, spec)
    b, vb = streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=None)
    torch.cuda.synchronize()
    assert va.tolist() == vb.tolist() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError, match="read_mel: cmvn must be a Cmvn or None"):
        streams.read_mel(SID, STARTS, FRAMES, spec, cmvn="global")
    with pytest.raises(ValueError, match="read_mel: cmvn must be a Cmvn or None"):
        streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Norm.cmvn())
    with pytest.raises(ValueError, match="read_mel: the Cmvn has 80 rows, the features 560"):
        streams.read_mel(SID, STARTS, FRAMES, spec, splice=cx.Splice.lfr(), cmvn=cx.Cmvn.global_(np.zeros(80), np.ones(80)))
    with pytest.raises(ValueError, match="read_mel: the Cmvn has 560 rows, the features 80"):
        streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Cmvn.global_(np.zeros(560), np.ones(560)))
    with pytest.raises(ValueError, match="read_mel: cmvn and normalize exclude each other"):
        streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Cmvn.xvector(), normalize=cx.Norm.cmvn())
    with pytest.raises(ValueError, match="cmvn_windows: a global Cmvn works in place"):
        ctx.cmvn_windows(a, va.numpy(), cx.WINDOW_CT, cx.Cmvn.global_(np.zeros(80), np.ones(80)), out=b)
    with pytest.raises(ValueError, match="cmvn_windows: the Cmvn has 3 rows, the batch 80"):
        ctx.cmvn_windows(a, va.numpy(), cx.WINDOW_CT, cx.Cmvn.global_(np.zeros(3), np.ones(3)))
    with pytest.raises(cx.ClaxonError, match="clx_cmvn_sliding_windows: d_out must not be d_in"):
        ctx.cmvn_windows(a, va.numpy(), cx.WINDOW_CT, cx.Cmvn.xvector(), out=a)
    torch.cuda.synchronize()
    spec.close()
