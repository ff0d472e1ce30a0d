"""clx_vad_windows and clx_select_windows on the GPU: over the GPU_* subsets of vad_cases.py, in both layouts, the device's mask,
thresholds, counts, selected cells and guard words equal the wave simulator's word for word, and the inputs keep their words;
calls whose tables grow, queued back to back on one stream and on two, give what the same call gives alone on a fresh context;
read_mel(cmvn=Cmvn.xvector(), vad=..., return_vad=True) on MelSpec.mfcc equals read_mel, vad_windows on the raw features,
cmvn_windows and select_windows bit for bit, with valid_frames equal to the counts; select=False leaves read_mel's own words;
read_mel's ValueErrors; augment= behind vad= draws from the counts.  Every comparison stands behind a synchronise."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_vad as sv
import vad_cases as vc
from gpu_guarded import NAN_FILL, device_out, written
from test_gpu_norm import SID, STARTS, _pcm
from test_gpu_outside_features import _flac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = (sv.CT, sv.TC)
FILL_BYTES = np.array([NAN_FILL], dtype=np.uint32).view(np.uint8)


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _vad(c):
    return cx.Vad(c["E"], c["s"], c["c"], c["p"], c["row"])


def _vad_buffers(c, layout):
    """(source tensor, its host copy, the mask's guarded buffer and slice, the thresholds' guarded buffer and slice)"""
    host = vc.as_layout(vc.vad_data(c), layout)
    B, T = len(c["valid"]), c["T"]
    mflat, mbody = device_out((B * T + 3) // 4, offset_words=c["offset"])
    tflat, tbody = device_out(B, offset_words=(c["offset"] + 1) % 4)
    return torch.from_numpy(host).to(DEV), host, mflat, mbody, tflat, tbody


def _vad_queue(ctx, c, layout, src, mbody, tbody, stream=None):
    ctx.vad_windows((src.data_ptr(), len(c["valid"]), c["rows"], c["T"]), c["valid"], layout, _vad(c), mask=mbody.data_ptr(),
                    thresholds=tbody.data_ptr(), stream=stream)


def _vad_results(c, layout, mflat, tflat):
    """(mask uint8 [B, T], thresholds float32 [B]) behind the guard checks; the bytes behind the mask in its last word keep the fill."""
    B, T = len(c["valid"]), c["T"]
    words = (B * T + 3) // 4
    raw = written(mflat, words, (c["name"], layout, "mask"), offset_words=c["offset"]).view(np.uint8)
    assert np.array_equal(raw[B * T:], FILL_BYTES[(B * T) % 4:] if (B * T) % 4 else FILL_BYTES[:0]), (c["name"], "a byte behind the mask was written")
    thr = written(tflat, B, (c["name"], layout, "thresholds"), offset_words=(c["offset"] + 1) % 4).view(np.float32)
    return raw[:B * T].reshape(B, T).copy(), thr.copy()


def _vad_same(c, layout, src, host, mflat, tflat, want=None):
    mask, thr = _vad_results(c, layout, mflat, tflat)
    want_mask, want_thr = vc.simulated_vad(c["name"], layout) if want is None else want
    assert np.array_equal(mask, want_mask), (c["name"], layout, int(np.count_nonzero(mask != want_mask)))
    assert vc.same_words(thr, want_thr), (c["name"], layout, thr, want_thr)
    assert vc.same_words(src.cpu().numpy(), host), (c["name"], layout, "the input was written")
    return mask, thr


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", vc.GPU_VAD)
def test_the_decision_on_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = vc.vad_case(name)
    src, host, mflat, mbody, tflat, tbody = _vad_buffers(c, layout)
    torch.cuda.synchronize()
    _vad_queue(ctx, c, layout, src, mbody, tbody)
    torch.cuda.synchronize()
    _vad_same(c, layout, src, host, mflat, tflat)


def _select_buffers(c, layout):
    x, mask = vc.select_data(c)
    host = vc.as_layout(x, layout)
    flat, body = device_out(x.size, offset_words=c["offset"])
    cflat, cbody = device_out(len(c["valid"]), offset_words=1)
    return torch.from_numpy(host).to(DEV), host, torch.from_numpy(mask).to(DEV), mask, flat, body, cflat, cbody


def _select_queue(ctx, c, layout, src, mask, body, stream=None):
    """Context.select_windows on raw pointers: returns the host counts (the call waits for them)."""
    return ctx.select_windows((src.data_ptr(), len(c["valid"]), c["rows"], c["T"]), c["valid"], mask.data_ptr(), layout, c["pad"],
                              out=body.data_ptr(), stream=stream)[1]


def _cells(c, layout, flat):
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    cells = written(flat, B * rows * T, (c["name"], layout), offset_words=c["offset"]).view(np.float32)
    return vc.from_layout(cells.reshape((B, T, rows) if layout == sv.TC else (B, rows, T)), layout)


def _select_same(c, layout, made, counts, want=None):
    src, host, mask, mask_host, flat = made[:5]
    cells = _cells(c, layout, flat)
    want_cells, want_counts = vc.simulated_select(c["name"], layout) if want is None else want
    assert counts.dtype == np.int64 and counts.tolist() == want_counts.tolist(), (c["name"], layout, counts, want_counts)
    assert vc.same_words(cells, want_cells), (c["name"], layout, int(np.count_nonzero(cells.view(np.uint32) != want_cells.view(np.uint32))))
    assert vc.same_words(src.cpu().numpy(), host) and np.array_equal(mask.cpu().numpy(), mask_host), (c["name"], layout, "an input was written")
    return cells, counts


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", vc.GPU_SELECT)
def test_the_selection_on_the_gpu_is_the_simulator_word_for_word(ctx, name, layout):
    c = vc.select_case(name)
    made = _select_buffers(c, layout)
    torch.cuda.synchronize()
    counts = _select_queue(ctx, c, layout, made[0], made[2], made[5])
    torch.cuda.synchronize()
    _select_same(c, layout, made, counts)


def test_the_device_counts_are_the_host_counts(ctx):
    """d_counts of the C call, which the Python layer does not use: the words the host copy holds, inside their guards."""
    import ctypes as C
    c = vc.select_case("random_rows30")
    made = _select_buffers(c, sv.CT)
    B = len(c["valid"])
    valid = np.asarray(c["valid"], dtype=np.uint32)
    opts = cx._SelectOpts(c["pad"], (C.c_uint32 * 3)(0, 0, 0))
    st = torch.cuda.current_stream()
    torch.cuda.synchronize()
    rc = cx.lib().clx_select_windows(ctx._h, made[0].data_ptr(), made[5].data_ptr(), B, c["rows"], c["T"], valid.ctypes.data, made[2].data_ptr(),
                                     sv.CT, C.byref(opts), made[7].data_ptr(), None, C.c_void_p(st.cuda_stream))
    assert rc == cx.OK
    torch.cuda.synchronize()
    got = written(made[6], B, "d_counts", offset_words=1)
    assert got.tolist() == vc.simulated_select("random_rows30", sv.CT)[1].tolist()
    assert vc.same_words(_cells(c, sv.CT, made[4]), vc.simulated_select("random_rows30", sv.CT)[0])


# small tables first, then ones that grow (ten windows of three tiles: 80 words; 560 rows), then small again: ("v" | "s", case, layout)
ORDER = [("v", "nonfinite", sv.CT), ("s", "second_rows560", sv.TC), ("v", "wide_c0", sv.TC), ("s", "ones_rows1", sv.CT), ("v", "c128_p0.12_s0.5", sv.CT),
         ("s", "random_rows80", sv.TC), ("v", "c2_p0.999_s0.0", sv.TC), ("s", "bytes_rows1", sv.CT), ("v", "voxceleb", sv.TC),
         ("s", "padding_counts_nothing", sv.CT)]


def _alone(kind, name, layout):
    """The call made alone on a context that has made no other, synchronised before and after: what it gave."""
    fresh = cx.Context(0, wait_s=120)
    try:
        if kind == "v":
            c = vc.vad_case(name)
            src, host, mflat, mbody, tflat, tbody = _vad_buffers(c, layout)
            torch.cuda.synchronize()
            _vad_queue(fresh, c, layout, src, mbody, tbody)
            torch.cuda.synchronize()
            return _vad_results(c, layout, mflat, tflat)
        c = vc.select_case(name)
        made = _select_buffers(c, layout)
        torch.cuda.synchronize()
        counts = _select_queue(fresh, c, layout, made[0], made[2], made[5])
        torch.cuda.synchronize()
        return _cells(c, layout, made[4]), counts
    finally:
        fresh.close()


def _queued(order, streams):
    ctx = cx.Context(0, wait_s=120)
    try:
        made = []
        for kind, name, layout in order:
            c = vc.vad_case(name) if kind == "v" else vc.select_case(name)
            made.append((kind, c, layout, _vad_buffers(c, layout) if kind == "v" else _select_buffers(c, layout)))
        torch.cuda.synchronize()
        counts = {}
        for i, (kind, c, layout, b) in enumerate(made):
            st = streams[i % len(streams)]
            if kind == "v":
                _vad_queue(ctx, c, layout, b[0], b[3], b[5], st)
            else:
                counts[i] = _select_queue(ctx, c, layout, b[0], b[2], b[5], st)
        for st in streams:
            st.synchronize()
        torch.cuda.synchronize()
        for i, (kind, c, layout, b) in enumerate(made):
            want = _alone(kind, c["name"], layout)
            if kind == "v":
                _vad_same(c, layout, b[0], b[1], b[2], b[4], want)
            else:
                _select_same(c, layout, b, counts[i], want)
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
# the recipe's options, and ones that are sure to drop frames: a frame is above when its C0 is above the window's mean
VADS = {"voxceleb": cx.Vad.voxceleb(), "mean": cx.Vad(0.0, 1.0, 1, 0.5, pad=-2.0)}


@pytest.mark.parametrize("which", sorted(VADS))
@pytest.mark.parametrize("layout", ("ct", "tc"))
def test_read_mel_xvector_front_end_is_its_four_steps(ctx, streams, layout, which):
    cmvn, vad = cx.Cmvn.xvector(pad=1.0), VADS[which]
    spec, L = cx.MelSpec.mfcc(ctx), cx._LAYOUTS[layout]
    got, gvf, gmask = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout, cmvn=cmvn, vad=vad, return_vad=True)
    raw, vf = streams.read_mel(SID, STARTS, FRAMES, spec, layout=layout)
    torch.cuda.synchronize()
    host = raw.cpu().numpy().copy()
    mask = ctx.vad_windows(raw, vf.numpy(), L, vad)
    normed = ctx.cmvn_windows(raw, vf.numpy(), L, cmvn)
    want, counts = ctx.select_windows(normed, vf.numpy(), mask, L, vad.pad)
    torch.cuda.synchronize()
    spec.close()
    assert tuple(got.shape) == tuple(raw.shape) and tuple(gmask.shape) == (len(SID), FRAMES) and gmask.dtype == torch.uint8
    assert torch.equal(gmask, mask) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert gvf.dtype == torch.int64 and gvf.tolist() == counts.tolist() == [int(mask[k, :v].sum()) for k, v in enumerate(vf.tolist())]
    assert not any(bool(mask[k, v:].any()) for k, v in enumerate(vf.tolist()))
    if which == "mean":                                      # (a cell at or below its window's mean exists wherever a frame does)
        assert all(n < v for n, v in zip(counts.tolist(), vf.tolist()) if v) and sum(counts.tolist()) > 0
    # ... and those four steps are the simulator's
    sim_mask, _ = sv.vad_windows(host, vf.numpy(), L, vad.energy_threshold, vad.energy_mean_scale, vad.frames_context, vad.proportion_threshold, vad.row)
    assert np.array_equal(mask.cpu().numpy(), sim_mask)
    sim, sim_counts = sv.select_windows(normed.cpu().numpy(), np.empty_like(host), vf.numpy(), sim_mask, L, vad.pad)
    assert vc.same_words(want.cpu().numpy(), sim) and sim_counts.tolist() == counts.tolist()


def test_select_false_returns_read_mels_own_words(ctx, streams):
    spec = cx.MelSpec.mfcc(ctx)
    vad = cx.Vad(0.0, 1.0, 1, 0.5, select=False)
    a, va = streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Cmvn.xvector())
    b, vb, mask = streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Cmvn.xvector(), vad=vad, return_vad=True)
    c, vcc = streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Cmvn.xvector(), vad=vad)
    d, vd = streams.read_mel(SID, STARTS, FRAMES, spec, cmvn=cx.Cmvn.xvector(), vad=None)
    raw, _ = streams.read_mel(SID, STARTS, FRAMES, spec)
    torch.cuda.synchronize()
    want = ctx.vad_windows(raw, va.numpy(), cx.WINDOW_CT, vad)
    torch.cuda.synchronize()
    spec.close()
    assert va.tolist() == vb.tolist() == vcc.tolist() == vd.tolist()
    for t in (b, c, d):
        assert torch.equal(a.view(torch.int32), t.view(torch.int32))
    assert torch.equal(mask, want) and 0 < int(mask.sum()) < sum(va.tolist())


def test_read_mel_refuses_what_it_should(ctx, streams):
    spec = cx.MelSpec.mfcc(ctx)
    with pytest.raises(ValueError, match="read_mel: vad must be a Vad or None"):
        streams.read_mel(SID, STARTS, FRAMES, spec, vad="voxceleb")
    with pytest.raises(ValueError, match="read_mel: vad must be a Vad or None"):
        streams.read_mel(SID, STARTS, FRAMES, spec, vad=cx.Cmvn.xvector())
    with pytest.raises(ValueError, match="read_mel: return_vad=True needs vad="):
        streams.read_mel(SID, STARTS, FRAMES, spec, return_vad=True)
    with pytest.raises(ValueError, match="read_mel: the Vad reads row %d, the features have %d" % (spec.n_out, spec.n_out)):
        streams.read_mel(SID, STARTS, FRAMES, spec, vad=cx.Vad(row=spec.n_out))
    a, va = streams.read_mel(SID, STARTS, FRAMES, spec)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="vad_windows: vad must be a Vad"):
        ctx.vad_windows(a, va.numpy(), cx.WINDOW_CT, None)
    with pytest.raises(ValueError, match="vad_windows: the Vad reads row 99"):
        ctx.vad_windows(a, va.numpy(), cx.WINDOW_CT, cx.Vad(row=99))
    with pytest.raises(ValueError, match="vad_windows: mask must be a contiguous uint8 tensor"):
        ctx.vad_windows(a, va.numpy(), cx.WINDOW_CT, cx.Vad(), mask=torch.zeros((len(SID), FRAMES + 1), dtype=torch.uint8, device=DEV))
    mask = ctx.vad_windows(a, va.numpy(), cx.WINDOW_CT, cx.Vad())
    with pytest.raises(ValueError, match="select_windows: mask must be a contiguous uint8 tensor"):
        ctx.select_windows(a, va.numpy(), mask.to(torch.int32), cx.WINDOW_CT)
    with pytest.raises(ValueError, match="select_windows: pad must be a number"):
        ctx.select_windows(a, va.numpy(), mask, cx.WINDOW_CT, pad="0")
    with pytest.raises(cx.ClaxonError, match="clx_select_windows: d_dst must not overlap d_src"):
        ctx.select_windows(a, va.numpy(), mask, cx.WINDOW_CT, out=a)
    torch.cuda.synchronize()
    spec.close()


def test_augment_behind_vad_draws_from_the_counts(ctx, streams):
    spec = cx.MelSpec.mfcc(ctx)
    vad = VADS["mean"]
    sel, counts = streams.read_mel(SID, STARTS, FRAMES, spec, vad=vad)
    _, vf = streams.read_mel(SID, STARTS, FRAMES, spec)
    torch.cuda.synchronize()
    B, V = len(SID), vf.numpy()
    assert np.all(counts.numpy()[V > 0] < V[V > 0]) and V.max() >= 3
    z = np.zeros((B, 1, 2), dtype=np.int64)
    warp = np.where((V >= 2)[:, None], np.stack([V - 1, V - 1], axis=1), 0)
    old = cx.SpecAugmentPlan(warp, z, z, 0.0)               # fits the valid_frames in front of the selection ...
    streams.read_mel(SID, STARTS, FRAMES, spec, augment=old)
    with pytest.raises(ValueError, match="read_mel: a warp of augment is neither"):   # ... and not the counts behind it
        streams.read_mel(SID, STARTS, FRAMES, spec, vad=vad, augment=old)
    policy = dict(freq_masks=1, freq_width=3, time_masks=1, time_width=4)
    got, gvf = streams.read_mel(SID, STARTS, FRAMES, spec, vad=vad, augment=cx.SpecAugment(seed=5, **policy))
    plan = cx.SpecAugment(seed=5, **policy).draw(counts.numpy(), spec.n_out)
    torch.cuda.synchronize()
    want = ctx.specaug_windows(sel, counts.numpy(), cx.WINDOW_CT, plan.warp, plan.freq_masks, plan.time_masks, plan.fill)
    torch.cuda.synchronize()
    spec.close()
    assert gvf.tolist() == counts.tolist() and torch.equal(got.view(torch.int32), want.view(torch.int32))
