"""clx_reverb_windows under the wave simulator (tests/wavesim/sim_reverb.cpp runs the production kernels of clx_reverb.hip, and
clx_add's sum kernels between them, on host buffers): over the edge matrix of reverb_cases.py the simulator equals the numpy
restatement of claxon_hip.h's definition word for word -- cells and gains, in both layouts, which are therefore bit-equal to each
other --, padding becomes +0.0, the data and the responses are never written and no NaN parked behind a live range reaches a
result; cells and gains lie inside the float64 reference's bounds; a NaN tap and an infinite tap reach the outputs
behind them and no other; every refusal has its text; and the Python side (Reverb, the reverb= arguments, Context.reverb_windows)
refuses what it should before anything touches a device."""
import numpy as np
import pytest

import claxon_amd as cx
import reverb_cases as rc
import simlib_reverb as sr

FINITE = [n for n in rc.NAMES if rc.case(n)["kind"] != "special"]


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_simulator_is_the_restatement_word_for_word(name):
    c = rc.case(name)
    x, ir = rc.data(c)
    want, wgains = rc.restated(name)
    for layout in (sr.CT, sr.TC):
        got, gains = rc.simulated(name, layout)
        assert rc.same_words(got, want), (name, layout, "cells", int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))))
        assert rc.same_words(gains, wgains), (name, layout, "gains", gains, wgains)
    assert rc.same_words(rc.simulated(name, sr.CT)[0], rc.simulated(name, sr.TC)[0])
    ww = want.view(np.uint32)
    for k, v in enumerate(c["valid"]):
        j = c["index"][k]
        assert np.all(ww[k, :, v:] == 0), (name, k, "padding is +0.0")
        if j < 0 or c["lens"][j] == 0:
            assert np.array_equal(ww[k, :, :v], x.view(np.uint32)[k, :, :v]) and wgains[k] == 1, (name, k, "a window without a response")
        if c["kind"] != "special":
            assert not np.any(np.isnan(want[k])) and not np.isnan(wgains[k]), (name, k, "a NaN from behind a live range")
        if not c["keep"]:
            assert wgains[k] == 1, (name, k)


@pytest.mark.parametrize("name", FINITE)
def test_cells_and_gains_lie_inside_the_reference_bounds(name):
    c = rc.case(name)
    x, ir = rc.data(c)
    for k, v in enumerate(c["valid"]):
        x[k, :, v:] = 0.0                                    # (the reference takes the live cells only; keep its input finite)
    for j, n in enumerate(c["lens"]):
        ir[j, n:] = 0.0
    y64, mag, N, g64 = sr.reference(x, c["valid"], ir, c["lens"], c["index"], c["keep"])
    got, gains = rc.simulated(name, sr.CT)
    B = len(c["valid"])
    if not c["keep"]:
        err = np.abs(got.astype(np.float64) - y64)
        bound = sr.cell_bound(mag, N)
        print("%s: worst error / bound = %.3g" % (name, float((err / np.maximum(bound, 1e-300)).max())))
        assert np.all(err <= bound), (name, float(err.max()))
        assert np.all(gains == 1)
        return
    grel = sr.gain_rel(y64, mag, N, c["valid"])
    scaled = g64 != 1
    rel = np.abs(gains.astype(np.float64) / g64 - 1)
    print("%s: worst |g / g_ref - 1| / bound = %.3g" % (name, float((rel / grel).max())))
    assert np.all(rel <= grel), (name, rel, grel)
    err = np.abs(got.astype(np.float64) - g64[:, None, None] * y64)
    bound = np.where(scaled[:, None, None], sr.scaled_bound(got, y64, g64, mag, N, grel), sr.cell_bound(mag, N))
    assert np.all(err <= bound), (name, float((err / np.maximum(bound, 1e-300)).max()))
    for k in range(B):                                       # the point of keep_power: the window's power is the dry signal's
        v = c["valid"][k]
        if scaled[k] and v:
            ex, ey = float((x[k, :, :v].astype(np.float64) ** 2).sum()), float((got[k, :, :v].astype(np.float64) ** 2).sum())
            assert abs(ey / ex - 1) < 1e-5, (name, k, ex, ey)


def test_the_reference_is_a_plain_convolution():
    """The float64 reference is numpy's convolve of the live samples with the live taps; a direct double loop over a small window
    agrees with it to float64 rounding, and with the simulator to the derived bound."""
    rng = np.random.default_rng(3)
    x, h = rng.standard_normal((1, 1, 40)).astype(np.float32), rng.standard_normal((1, 9)).astype(np.float32)
    y64, mag, N, _ = sr.reference(x, [33], h, [7], [0], 0)
    for t in range(33):
        d = sum(float(h[0, k]) * float(x[0, 0, t - k]) for k in range(min(t, 6) + 1))
        assert abs(d - y64[0, 0, t]) <= 16 * 2.0 ** -53 * mag[0, 0, t]
        assert N[0, t] == min(t + 1, 7)
    assert np.all(y64[0, 0, 33:] == 0)
    out = np.full_like(x, 7.0)
    assert sr.reverb_windows(x, [33], h, [7], [0], sr.CT, out)
    assert np.all(np.abs(out.astype(np.float64) - y64) <= sr.cell_bound(mag, N)) and np.all(out[0, 0, 33:] == 0)


def test_a_nan_tap_and_an_infinite_tap_reach_the_outputs_behind_them_and_no_other():
    """Taps that reach before the crop are skipped, not multiplied by +0.0: the outputs t < k of a NaN or infinite tap h[k] are
    finite, those from k on are not; a tap at or behind valid[k] is never read."""
    c = rc.case("nan_and_inf_taps")
    for layout in (sr.CT, sr.TC):
        got, gains = rc.simulated("nan_and_inf_taps", layout)
        assert np.all(np.isfinite(got[0, :, :rc.NAN_TAP])) and np.all(np.isnan(got[0, :, rc.NAN_TAP:]))
        assert np.all(np.isfinite(got[1, :, :rc.INF_TAP])) and np.all(np.isposinf(got[1, :, rc.INF_TAP:]))
        assert c["valid"][2] <= rc.NAN_TAP and np.all(np.isfinite(got[2]))
        assert np.all(np.isfinite(got[3, :, :rc.INF_TAP])) and np.all(np.isposinf(got[3, :, rc.INF_TAP:]))
        assert np.all(gains == 1)


def test_windows_that_share_a_response_are_what_they_are_alone():
    name = "T%d_rows2_a1" % (rc.TILE + 1)
    c = rc.case(name)
    shared = [k for k, j in enumerate(c["index"]) if j == 4]
    assert len(shared) == 3 and len({c["valid"][k] for k in shared}) == 3
    x, ir = rc.data(c)
    got, gains = rc.simulated(name, sr.TC)
    for k in shared:
        one, g1 = sr.restate(x[k:k + 1], c["valid"][k:k + 1], ir, c["lens"], [4], c["keep"])
        assert rc.same_words(got[k:k + 1], one) and rc.same_words(gains[k:k + 1], g1)


def test_nothing_to_do_succeeds_and_launches_nothing():
    assert not sr.reverb_windows(None, None, None, None, None, sr.CT, None, shape=(0, 3, 5), n_ir=0)
    assert not sr.reverb_windows(None, None, None, None, None, sr.TC, None, 1, shape=(4, 3, 0), n_ir=2, K=9)
    x = np.full((2, 2, 9), 7.0, dtype=np.float32)
    x[1, :, 4:] = np.float32("nan")
    out = np.full_like(x, -3.0)
    g = np.full(2, -1.0, dtype=np.float32)
    assert sr.reverb_windows(x, [9, 4], None, None, [-1, -1], sr.CT, out, 1, g)     # no response anywhere: a copy, padding zeroed
    assert np.all(out[0] == 7.0) and np.all(out[1, :, :4] == 7.0) and np.all(out[1, :, 4:].view(np.uint32) == 0) and np.all(g == 1)


def _refusal_args():
    return dict(data=np.ones(2 * 3 * 5, dtype=np.float32), out=np.zeros(2 * 3 * 5, dtype=np.float32), ir=np.ones(2 * 4, dtype=np.float32), rows=3,
                valid=[5, 2], lens=[4, 1], index=[1, 0], layout=sr.CT, keep=None, reserved=0, K=4, n_ir=2)


REFUSALS = [
    (dict(keep=2), "clx_reverb_windows: opts->keep_power must be 0 or 1 and opts->reserved 0"),
    (dict(keep=1, reserved=4), "clx_reverb_windows: opts->keep_power must be 0 or 1 and opts->reserved 0"),
    (dict(layout=7), "clx_reverb_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
    (dict(rows=0), "clx_reverb_windows: rows must be 1..8"),
    (dict(rows=9), "clx_reverb_windows: rows must be 1..8"),
    (dict(K=0), "clx_reverb_windows: K must be 1..65536"),
    (dict(K=65537), "clx_reverb_windows: K must be 1..65536"),
    (dict(valid=None), "clx_reverb_windows: null argument"),
    (dict(index=None), "clx_reverb_windows: null argument"),
    (dict(data=None), "clx_reverb_windows: null argument"),
    (dict(out=None), "clx_reverb_windows: null argument"),
    (dict(ir=None), "clx_reverb_windows: null argument"),
    (dict(lens=None), "clx_reverb_windows: null argument"),
    (dict(valid=[3, 6]), "clx_reverb_windows: valid[k] is larger than T"),
    (dict(lens=[4, 5]), "clx_reverb_windows: ir_len[j] is larger than K"),
    (dict(index=[0, 2]), "clx_reverb_windows: ir_index[k] must be -1 .. n_ir - 1"),
    (dict(index=[-2, 0]), "clx_reverb_windows: ir_index[k] must be -1 .. n_ir - 1"),
    (dict(out="data"), "clx_reverb_windows: d_out overlaps d_data"),
    (dict(out="data+7"), "clx_reverb_windows: d_out overlaps d_data"),
]


@pytest.mark.parametrize("change,text", REFUSALS)
def test_every_refusal_has_its_text_and_writes_nothing(change, text):
    a = _refusal_args()
    a.update(change)
    big = np.ones(2 * 3 * 5 + 7, dtype=np.float32)
    if isinstance(a["out"], str):
        a["data"], a["out"] = big[:30], (big[:30] if a["out"] == "data" else big[7:])
    before = None if a["out"] is None else a["out"].copy()
    with pytest.raises(cx.ClaxonError) as e:
        sr.reverb_windows(a["data"], a["valid"], a["ir"], a["lens"], a["index"], a["layout"], a["out"], a["keep"], shape=(2, a["rows"], 5),
                          n_ir=a["n_ir"], K=a["K"], reserved=a["reserved"])
    assert text in str(e.value)
    assert before is None or np.array_equal(before, a["out"])


def test_the_stated_sizes_are_the_sources():
    L = sr.lib()
    assert (L.sim_reverb_tile(), L.sim_reverb_chunk(), L.sim_reverb_group(), L.sim_reverb_max_rows(), L.sim_reverb_max_taps(), L.sim_reverb_lds_bytes(),
            L.sim_reverb_table_bytes()) == (2048, 256, 8, 8, 65536, 10240, 28)
    assert "clx_reverb_windows" in cx.EXPORTS and cx.REVERB_TAPS_LIMIT == 65536


def _bare_set(ctx, n_streams=2, channels=1):
    """A StreamSet as far as the refusals look at it: no device, no streams."""
    s = cx.StreamSet.__new__(cx.StreamSet)
    s.ctx, s._descs = ctx, np.zeros(0, dtype=cx.FRAME_DESC_DTYPE)
    s.problems, s.channels, s.sample_rates = [None] * n_streams, [channels] * n_streams, [16000] * n_streams
    s._lengths = np.full(n_streams, 100, dtype=np.int64)
    return s


def test_reverb_is_a_plain_value():
    src = _bare_set(object())
    r = cx.Reverb([0, -1, 1], src)
    assert len(r) == 3 and r.source is src and r.taps is None and r.keep_power is True and r.starts.tolist() == [0, 0, 0]
    r = cx.Reverb([0, 1], src, starts=[5, 7], taps=800, keep_power=False)
    assert r.starts.tolist() == [5, 7] and r.taps == 800 and r.keep_power is False and "2 windows" in repr(r)
    assert len(cx.Reverb([], src)) == 0
    cx.Reverb([-1], src, starts=[-5])                        # (the start of a window without a response is not looked at)
    assert cx.Reverb([0], src, taps=65536).taps == 65536


@pytest.mark.parametrize("args,kw", [(([0, 1], None), {}), (([0], "a set"), {}), (([0, 1], "src"), dict(starts=[0])), (([-2], "src"), {}),
                                     (([0], "src"), dict(starts=[-1])), (([0], "src"), dict(taps=0)), (([0], "src"), dict(taps=65537)),
                                     (([0], "src"), dict(taps=2.5)), (([0], "src"), dict(taps=True))])
def test_reverb_refuses(args, kw):
    args = tuple(_bare_set(object()) if a == "src" else a for a in args)
    with pytest.raises(ValueError):
        cx.Reverb(*args, **kw)


def test_read_and_read_mel_refuse_a_bad_reverb_before_any_work():
    ctx, other = object(), object()
    s, src = _bare_set(ctx), _bare_set(ctx)
    for bad in ("rir", 3, dict(taps=8), cx.Norm()):
        with pytest.raises(ValueError, match="reverb must be a Reverb"):
            s.read([0], [0], 16, reverb=bad)
        with pytest.raises(ValueError, match="reverb must be a Reverb"):
            s.read_mel([0], [0], 4, None, reverb=bad)
    with pytest.raises(ValueError, match="reverb has 1 windows, the call 2"):
        s.read([0, 1], [0, 0], 16, reverb=cx.Reverb([0], src))
    with pytest.raises(ValueError, match="a stream its source does not have"):
        s.read([0, 1], [0, 0], 16, reverb=cx.Reverb([0, 2], src))
    with pytest.raises(ValueError, match="another context"):
        s.read([0], [0], 16, reverb=cx.Reverb([0], _bare_set(other)))
    closed = _bare_set(ctx)
    closed.close()
    with pytest.raises(ValueError, match="source is closed"):
        s.read([0], [0], 16, reverb=cx.Reverb([0], closed))
    with pytest.raises(ValueError, match="response stream 1 has 2 channels, not one"):
        s.read([0], [0], 16, reverb=cx.Reverb([1], _bare_set(ctx, channels=2)))
    long = _bare_set(ctx)
    long._lengths = np.full(2, 70000, dtype=np.int64)
    with pytest.raises(ValueError, match="the longest response has 70000 samples"):
        s.read([0], [0], 16, reverb=cx.Reverb([1], long))


@pytest.mark.parametrize("kw,text", [
    (dict(valid=[1]), "valid has 1 entries for 2 windows"), (dict(ir_index=[0]), "ir_index has 1 entries"),
    (dict(ir_len=[1, 1]), "ir_len has 2 entries for 1 windows")])
def test_reverb_windows_refuses_lengths_that_do_not_match(kw, text):
    c = cx.Context.__new__(cx.Context)
    a = dict(valid=[4, 4], ir_len=[4], ir_index=[0, -1])
    a.update(kw)
    with pytest.raises(ValueError, match=text):
        c.reverb_windows((0, 2, 1, 4), a["valid"], (0, 1, 4), a["ir_len"], a["ir_index"], cx.WINDOW_CT, out=0)
