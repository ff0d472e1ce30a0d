"""clx_cmvn_stats_windows and clx_cmvn_grouped_windows on the GPU: over a subset of cmvn_stats_cases.py -- both layouts, both entry
points, the strand and chunk edges, 16 / 17 / 560 / 8192 rows, unsorted and absent groups, 65536 groups, cells that are not
finite -- the device's words and guard words equal the wave simulator's word for word; a reset and two accumulating calls on one
stream; two CmvnStats fed on two streams at once, each equal to its calls alone on a fresh context; read_mel(stats=, groups=)
equals read_mel followed by CmvnStats.accumulate, read_mel(cmvn=Cmvn.grouped(...), groups=) equals read_mel followed by
Context.cmvn_windows(groups=), a one-group stats.cmvn() through the global path equals the grouped path; the ValueErrors.
Every comparison stands behind a synchronise."""
import ctypes as C

import numpy as np
import pytest
import torch

import claxon_amd as cx
import cmvn_stats_cases as cc
import simlib_cmvn_stats as ss
from gpu_guarded import device_out, written
from test_gpu_cmvn import FRAMES
from test_gpu_norm import SID, STARTS, _pcm
from test_gpu_outside_features import _flac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUPS = [1, 0, 2, -1, 1]                # of the five windows of SID: group 2 has one window, one window takes no part


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _device64(words):
    """(the whole float64 device buffer of NAN64 words, the `words` doubles of it a call may write)."""
    flat = torch.from_numpy(np.full(words + 2 * cc.GUARD, cc.NAN64, dtype=np.uint64).view(np.float64)).to(DEV)
    assert flat.data_ptr() % 8 == 0
    return flat, flat[cc.GUARD:cc.GUARD + words]


def _written64(flat, words, what):
    h = flat.cpu().numpy().view(np.uint64)
    assert np.all(h[:cc.GUARD] == cc.NAN64) and np.all(h[cc.GUARD + words:] == cc.NAN64), (what, "a guard word around the accumulator was written")
    body = h[cc.GUARD:cc.GUARD + words]
    assert not np.any(body == cc.NAN64), (what, "a word of the accumulator was not written")
    return body.view(np.float64)


def _handle(stream):
    h = getattr(stream, "cuda_stream", stream)
    return C.c_void_p(h) if h else None


def _stats_queue(ctx, c, layout, src, acc, accumulate, stream=None):
    valid = np.asarray(c["valid"], dtype=np.uint32)
    g = None if c["groups"] is None else np.asarray(c["groups"], dtype=np.int32)
    opts = cx._CmvnStatsOpts(int(accumulate), 0)
    ctx._check(cx.lib().clx_cmvn_stats_windows(ctx._h, src.data_ptr(), len(valid), c["rows"], c["T"], valid.ctypes.data, layout,
                                               None if g is None else g.ctypes.data, c["n_groups"], acc.data_ptr(), C.byref(opts), _handle(stream)))


def _same_stats(c, got, want, what):
    got, want = got.reshape(want.shape), want
    if c["kind"] == "nonfinite":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and 0 < np.count_nonzero(nan), what
        got, want = np.where(nan, 0.0, got), np.where(nan, 0.0, want)
    assert cc.same_words64(got, want), (what, int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64))))


@pytest.mark.parametrize("layout", cc.LAYOUTS)
@pytest.mark.parametrize("name", cc.GPU)
def test_the_accumulator_on_the_gpu_is_the_simulators_word_for_word(ctx, name, layout):
    c = cc.case(name)
    words = int(np.prod(cc.stats_shape(c)))
    src = torch.from_numpy(cc.as_layout(cc.data(c), layout)).to(DEV)
    flat, acc = _device64(words)
    torch.cuda.synchronize()
    _stats_queue(ctx, c, layout, src, acc, False)
    torch.cuda.synchronize()
    _same_stats(c, _written64(flat, words, (name, layout)), cc.simulated_stats(name, layout), (name, layout))
    assert cc.same_words(src.cpu().numpy(), cc.as_layout(cc.data(c), layout)), (name, layout, "the input was written")


@pytest.mark.parametrize("layout", cc.LAYOUTS)
@pytest.mark.parametrize("name", cc.GPU)
def test_the_grouped_apply_on_the_gpu_is_the_simulators_word_for_word(ctx, name, layout):
    c = cc.case(name)
    x = cc.data(c)
    B, rows, T = x.shape
    want, want_ss = cc.simulated_grouped(name, layout)
    flat, body = device_out(x.size, offset_words=c["offset"])
    body.copy_(torch.from_numpy(cc.as_layout(x, layout).reshape(-1)))
    sflat, sbody = device_out(c["n_groups"] * 2 * rows, offset_words=1)
    host_stats = cc.simulated_stats(name, ss.CT)
    stats = torch.from_numpy(host_stats).to(DEV)
    valid = np.asarray(c["valid"], dtype=np.uint32)
    g = None if c["groups"] is None else np.asarray(c["groups"], dtype=np.int32)
    opts = cx._CmvnGroupedOpts(c["norm_vars"], c["pad"], 0)
    torch.cuda.synchronize()
    ctx._check(cx.lib().clx_cmvn_grouped_windows(ctx._h, body.data_ptr(), B, rows, T, valid.ctypes.data, layout, None if g is None else g.ctypes.data,
                                                 c["n_groups"], stats.data_ptr(), sbody.data_ptr(), C.byref(opts), None))
    torch.cuda.synchronize()
    cells = written(flat, x.size, (name, layout), offset_words=c["offset"]).view(np.float32)
    cells = cc.from_layout(cells.reshape((B, T, rows) if layout == ss.TC else (B, rows, T)), layout)
    got_ss = written(sflat, c["n_groups"] * 2 * rows, (name, layout, "shift_scale"), offset_words=1).view(np.float32).reshape(want_ss.shape)
    if c["kind"] == "nonfinite":
        for a, b in ((cells, want), (got_ss, want_ss)):
            nan = np.isnan(b)
            assert np.array_equal(np.isnan(a), nan) and 0 < np.count_nonzero(nan) < nan.size // 2, (name, layout)
            assert cc.same_words(np.where(nan, np.float32(0), a), np.where(nan, np.float32(0), b)), (name, layout)
    else:
        assert cc.same_words(got_ss, want_ss), (name, layout, "shift_scale")
        assert cc.same_words(cells, want), (name, layout, int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))
    assert cc.same_words64(stats.cpu().numpy(), host_stats), (name, layout, "the accumulator was written")


@pytest.mark.parametrize("layout", cc.LAYOUTS)
@pytest.mark.parametrize("name", ["T65", "T4097", "unsorted", "many_groups"])
def test_a_reset_and_two_accumulating_calls_on_one_stream(ctx, name, layout):
    c = cc.case(name)
    words = int(np.prod(cc.stats_shape(c)))
    srcs = [torch.from_numpy(cc.as_layout(cc.data(c, i), layout)).to(DEV) for i in range(3)]
    flat, acc = _device64(words)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    for i, src in enumerate(srcs):
        _stats_queue(ctx, c, layout, src, acc, i > 0, st)
    st.synchronize()
    torch.cuda.synchronize()
    _same_stats(c, _written64(flat, words, (name, layout)), cc.simulated_stats(name, layout, 3), (name, layout))


# (case, layout) of the calls each of the two accumulators is fed, tables that grow among them
FEEDS = [[("T65", ss.CT), ("T65", ss.TC), ("T65", ss.CT)], [("rows560", ss.TC), ("rows560", ss.CT), ("rows560", ss.TC)]]


def _feed(ctx, feed, stream):
    """A CmvnStats fed feed's calls on `stream` (data(c, i) for call i), nothing waited for: (stats, the tensors kept alive)."""
    c = cc.case(feed[0][0])
    s = cx.CmvnStats(ctx, c["rows"], c["n_groups"])
    keep = []
    for i, (name, layout) in enumerate(feed):
        x = cc.data(c, i)
        B, rows, T = x.shape
        keep.append(torch.from_numpy(cc.as_layout(x, layout)).to(DEV))
    torch.cuda.synchronize()
    return s, c, keep


def test_two_accumulators_fed_on_two_streams_at_once_equal_their_calls_alone():
    ctx = cx.Context(0, wait_s=120)
    try:
        streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
        fed = [_feed(ctx, feed, st) for feed, st in zip(FEEDS, streams)]
        torch.cuda.synchronize()
        for i in range(3):                                   # interleaved: the two streams' calls hand the context's tables to each other
            for (s, c, keep), feed, st in zip(fed, FEEDS, streams):
                s.accumulate((keep[i].data_ptr(), len(c["valid"]), c["rows"], c["T"]), c["valid"], feed[i][1], c["groups"], stream=st)
        got = [s.numpy() for s, _, _ in fed]                 # (waits for the device)
        for g, feed in zip(got, FEEDS):
            fresh = cx.Context(0, wait_s=120)
            try:
                s, c, keep = _feed(fresh, feed, None)
                for i in range(3):
                    s.accumulate(keep[i], c["valid"], feed[i][1], c["groups"])
                    torch.cuda.synchronize()
                alone = s.numpy()
            finally:
                fresh.close()
            assert cc.same_words64(g, alone), feed[0][0]
            want = ss.restate_stats(cc.data(c, 0), c["valid"], c["groups"], c["n_groups"])
            for i in (1, 2):
                want = ss.restate_stats(cc.data(c, i), c["valid"], c["groups"], c["n_groups"], want, True)
            assert cc.same_words64(g, want[0] if c["n_groups"] == 1 else want), feed[0][0]
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def streams(ctx):
    """A mono stream at 16 kHz and a stereo one at 8 kHz (resampled when read at 16 kHz)."""
    s = cx.open_streams(ctx, [_flac(_pcm(5000, 1, 11), 16000), _flac(_pcm(3000, 2, 12), 8000)])
    assert s.problems == [None, None]
    return s


def _specs(ctx, which):
    if which == "lfr":
        return cx.MelSpec.kaldi(ctx), dict(splice=cx.Splice.lfr()), 560
    return cx.MelSpec.mfcc(ctx), dict(vad=cx.Vad.voxceleb()), 13


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("which", ("lfr", "mfcc_vad"))
def test_read_mel_stats_is_read_mel_then_accumulate(ctx, streams, which, layout):
    spec, kw, rows = _specs(ctx, which)
    L = cx._LAYOUTS[layout]
    a, b = cx.CmvnStats(ctx, rows, 3), cx.CmvnStats(ctx, rows, 3)
    got, gvf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, stats=a, groups=GROUPS, **kw)
    plain, vf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, **kw)
    torch.cuda.synchronize()
    assert gvf.tolist() == vf.tolist() and torch.equal(got.view(torch.int32), plain.view(torch.int32)), "stats= changed what read_mel returns"
    # the batch the accumulator saw: behind splice= and the VAD decision, before the selection
    raw_kw = dict(kw)
    if "vad" in raw_kw:
        raw_kw["vad"] = cx.Vad.voxceleb(select=False)
    raw, rvf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, **raw_kw)
    torch.cuda.synchronize()
    assert b.accumulate(raw, rvf.numpy(), L, GROUPS) is b
    na, nb = a.numpy(), b.numpy()
    spec.close()
    assert na.shape == (3, 2, rows + 1) and cc.same_words64(na, nb)
    assert na[:, 0, rows].tolist() == [float(sum(int(v) for v, g in zip(rvf.tolist(), GROUPS) if g == j)) for j in range(3)] and na[:, 0, rows].sum() > 0
    host = raw.cpu().numpy()
    x = host.transpose(0, 2, 1) if layout == "tc" else host
    assert cc.same_words64(na, ss.restate_stats(np.ascontiguousarray(x), rvf.numpy(), GROUPS, 3))
    a.close()
    b.close()


@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_read_mel_grouped_cmvn_is_read_mel_then_cmvn_windows(ctx, streams, layout):
    spec, L = cx.MelSpec.kaldi(ctx), cx._LAYOUTS[layout]
    s = cx.CmvnStats(ctx, 80, 3)
    streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, stats=s, groups=GROUPS)
    cmvn = cx.Cmvn.grouped(s, norm_vars=True, pad=-2.0)
    assert cmvn.rows == 80
    got, gvf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, cmvn=cmvn, groups=GROUPS)
    want, vf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout)
    torch.cuda.synchronize()
    host = want.cpu().numpy().copy()
    assert ctx.cmvn_windows(want, vf.numpy(), L, cmvn, groups=GROUPS) is want
    torch.cuda.synchronize()
    spec.close()
    assert gvf.tolist() == vf.tolist() and torch.equal(got.view(torch.int32), want.view(torch.int32))
    shsc = np.zeros((3, 2, 80), dtype=np.float32)
    sim = ss.grouped_windows(host.copy(), vf.numpy(), L, GROUPS, 3, s.numpy(), shsc, True, -2.0)
    assert cc.same_words(want.cpu().numpy(), sim)
    assert not cc.same_words(sim, host)
    s.close()


@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_one_groups_cmvn_through_the_global_path_is_the_grouped_path(ctx, streams, layout):
    spec, L = cx.MelSpec.kaldi(ctx), cx._LAYOUTS[layout]
    s = cx.CmvnStats(ctx, 560)
    streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, splice=cx.Splice.lfr(), stats=s)
    assert s.numpy().shape == (2, 561) and s.as_wenet()["frame_num"] == int(s.numpy()[0, 560]) > 0
    a, va = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, splice=cx.Splice.lfr(), cmvn=s.cmvn(pad=0.5))
    b, vb = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, splice=cx.Splice.lfr(), cmvn=cx.Cmvn.grouped(s, pad=0.5))
    torch.cuda.synchronize()
    spec.close()
    assert va.tolist() == vb.tolist() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    # add_: another rank's accumulator on top; reset: zeros
    before = s.numpy()
    assert cc.same_words64(s.add_(before).numpy(), before + before)
    assert np.all(s.reset().numpy().view(np.uint64) == 0)
    s.close()


@pytest.mark.parametrize("current", ("default", "side"))
def test_reset_then_accumulate_with_no_stream_named_is_ordered(ctx, streams, current):
    """reset() followed at once by accumulate() and by read_mel(stats=), none given a stream, on an accumulator that held other
    words: all three take torch's current stream (the default one, or a side stream made current), so the zeros stand in front of
    the fold.  The context's own stream is kept busy with earlier calls through (pointer, B, rows, T) tuples meanwhile."""
    c = cc.case("T4097")
    x = cc.data(c)
    src = torch.from_numpy(x).to(DEV)
    busy = cx.CmvnStats(ctx, c["rows"], c["n_groups"])
    s = cx.CmvnStats(ctx, c["rows"], c["n_groups"])
    spec = cx.MelSpec.mfcc(ctx)
    m = cx.CmvnStats(ctx, 13, 3)
    plain, vf = streams.read_mel(SID, STARTS, FRAMES, spec)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side if current == "side" else torch.cuda.current_stream()):
        for i in range(3):                                   # other words first
            s.accumulate(src, c["valid"], ss.CT, c["groups"])
            m.accumulate(plain, vf.numpy(), cx.WINDOW_CT, GROUPS)
        for i in range(8):                                   # the context's own stream (a tuple names no tensor, so no torch stream)
            busy.accumulate((src.data_ptr(), len(c["valid"]), c["rows"], c["T"]), c["valid"], ss.CT, c["groups"])
        s.reset()
        s.accumulate(src, c["valid"], ss.CT, c["groups"])
        m.reset()
        streams.read_mel(SID, STARTS, FRAMES, spec, stats=m, groups=GROUPS)
    torch.cuda.synchronize()
    assert cc.same_words64(s.numpy(), cc.simulated_stats("T4097", ss.CT)), current
    assert cc.same_words64(m.numpy(), ss.restate_stats(plain.cpu().numpy(), vf.numpy(), GROUPS, 3)), current
    assert m.numpy()[:, 0, 13].sum() > 0
    spec.close()
    for a in (busy, s, m):
        a.close()


def test_the_value_errors(ctx, streams):
    spec = cx.MelSpec.kaldi(ctx)
    s1, s3, s560 = cx.CmvnStats(ctx, 80), cx.CmvnStats(ctx, 80, 3), cx.CmvnStats(ctx, 560)
    a, va = streams.read_mel(SID, STARTS, FRAMES, spec)
    b, vb = streams.read_mel(SID, STARTS, FRAMES, spec, stats=None, groups=None)
    torch.cuda.synchronize()
    assert va.tolist() == vb.tolist() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError, match="read_mel: stats must be an open CmvnStats"):
        streams.read_mel(SID, STARTS, FRAMES, spec, stats="stats")
    with pytest.raises(ValueError, match="read_mel: the CmvnStats has 560 rows, the features 80"):
        streams.read_mel(SID, STARTS, FRAMES, spec, stats=s560)
    with pytest.raises(ValueError, match="read_mel: the CmvnStats has 80 rows, the features 560"):
        streams.read_mel(SID, STARTS, FRAMES, spec, splice=cx.Splice.lfr(), stats=s1)
    with pytest.raises(ValueError, match="read_mel: the Cmvn has 560 rows, the features 80"):
        streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Cmvn.grouped(s560))
    with pytest.raises(ValueError, match="read_mel: groups must be 5 whole numbers"):
        streams.read_mel(SID, STARTS, FRAMES, spec, stats=s3, groups=[0, 1])
    with pytest.raises(ValueError, match="read_mel: groups must lie in -1..2"):
        streams.read_mel(SID, STARTS, FRAMES, spec, stats=s3, groups=[0, 1, 3, 0, 0])
    with pytest.raises(ValueError, match="read_mel: groups must lie in -1..0"):
        streams.read_mel(SID, STARTS, FRAMES, spec, stats=s3, cmvn=cx.Cmvn.grouped(s1), groups=[0, 1, 2, 0, 0])
    with pytest.raises(ValueError, match="read_mel: groups= needs stats= or a grouped cmvn="):
        streams.read_mel(SID, STARTS, FRAMES, spec, groups=GROUPS)
    with pytest.raises(ValueError, match="read_mel: groups= needs stats= or a grouped cmvn="):
        streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Cmvn.xvector(), groups=GROUPS)
    with pytest.raises(ValueError, match="read_mel: the grouped Cmvn's CmvnStats has 3 groups: give groups="):
        streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Cmvn.grouped(s3))
    with pytest.raises(ValueError, match="read_mel: stats= is the CmvnStats the grouped cmvn= reads"):
        streams.read_mel(SID, STARTS, FRAMES, spec, stats=s3, cmvn=cx.Cmvn.grouped(s3), groups=GROUPS)
    with pytest.raises(ValueError, match="cmvn_windows: groups= goes with a grouped Cmvn"):
        ctx.cmvn_windows(a, va.numpy(), cx.WINDOW_CT, cx.Cmvn.global_(np.zeros(80), np.ones(80)), groups=GROUPS)
    with pytest.raises(ValueError, match="cmvn_windows: the Cmvn's CmvnStats has 3 groups: give groups="):
        ctx.cmvn_windows(a, va.numpy(), cx.WINDOW_CT, cx.Cmvn.grouped(s3))
    with pytest.raises(ValueError, match="cmvn_windows: a grouped Cmvn works in place"):
        ctx.cmvn_windows(a, va.numpy(), cx.WINDOW_CT, cx.Cmvn.grouped(s1), out=b)
    with pytest.raises(ValueError, match="CmvnStats.accumulate: the CmvnStats has 560 rows, the batch 80"):
        s560.accumulate(a, va.numpy(), cx.WINDOW_CT)
    with pytest.raises(ValueError, match="CmvnStats.cmvn: needs groups == 1"):
        s3.cmvn()
    with pytest.raises(ValueError, match="CmvnStats.as_wenet: needs groups == 1"):
        s3.as_wenet()
    with pytest.raises(ValueError, match="Cmvn: stats must be finite, with a count above 0"):
        s1.cmvn()                                            # (nothing accumulated yet)
    with pytest.raises(ValueError, match="Cmvn: grouped\\(\\) needs an open CmvnStats"):
        cx.Cmvn.grouped(np.zeros((2, 81)))
    with pytest.raises(cx.ClaxonError, match="clx_cmvn_stats_windows: valid\\[k\\] is larger than T"):
        s1.accumulate(a, [FRAMES + 1] * len(SID), cx.WINDOW_CT)
    torch.cuda.synchronize()
    assert all(np.all(s.numpy() == 0) for s in (s1, s3, s560)), "a refused call accumulated"
    for s in (s1, s3, s560):
        s.close()
    with pytest.raises(ValueError, match="CmvnStats: accumulate\\(\\) on a closed CmvnStats"):
        s1.accumulate(a, va.numpy(), cx.WINDOW_CT)
    spec.close()
