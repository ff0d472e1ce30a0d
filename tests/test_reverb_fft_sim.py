"""clx_reverb_windows_fft under the wave simulator (tests/wavesim/sim_reverb_fft.cpp runs the production kernels of
clx_reverb_fft.hip, clx_add's sum kernels and clx_reverb's gain and scale kernels on host buffers): over the edge matrix of
reverb_fft_cases.py the simulator equals the numpy restatement of claxon_hip.h's schedule word for word -- cells and gains, in both
layouts, which are therefore bit-equal to each other --, padding becomes +0.0, the data and the responses are never written and no NaN
parked behind a live range reaches a result; a (window, row) convolved alone has the words it has in its batch; a window with a NaN
tap leaves its neighbour's words alone; cells and gains lie inside the bound DESIGN.md 4.19 derives around the float64 reference
(simlib_reverb.reference: np.convolve); every refusal has its text; and the Python side (method=) refuses what it should before
anything touches a device."""
import numpy as np
import pytest

import claxon_amd as cx
import reverb_fft_cases as rc
import simlib_reverb as sr
import simlib_reverb_fft as sf

FINITE = [n for n in rc.NAMES if rc.case(n)["kind"] != "nan_tap"]


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_simulator_is_the_restatement_word_for_word(name):
    c = rc.case(name)
    x, ir = rc.data(c)
    want, wgains = rc.restated(name)
    ok = rc.specified(c)
    for layout in (sf.CT, sf.TC):
        got, gains = rc.simulated(name, layout)
        a, b = rc.masked(c, got), rc.masked(c, want)
        assert rc.same_words(a, b), (name, layout, "cells", int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))))
        assert rc.same_words(gains[ok], wgains[ok]), (name, layout, "gains", gains, wgains)
    assert rc.same_words(rc.masked(c, rc.simulated(name, sf.CT)[0]), rc.masked(c, rc.simulated(name, sf.TC)[0]))
    ww = want.view(np.uint32)
    for k, v in enumerate(c["valid"]):
        j = c["index"][k]
        assert np.all(ww[k, :, v:] == 0), (name, k, "padding is +0.0")
        if j < 0 or c["lens"][j] == 0:
            assert np.array_equal(ww[k, :, :v], x.view(np.uint32)[k, :, :v]) and wgains[k] == 1, (name, k, "a window without a response")
        if ok[k]:
            assert not np.any(np.isnan(want[k])) and not np.isnan(wgains[k]), (name, k, "a NaN from behind a live range")
        if not c["keep"]:
            assert wgains[k] == 1, (name, k)


@pytest.mark.parametrize("name", FINITE)
def test_cells_and_gains_lie_inside_the_derived_bound(name):
    c = rc.case(name)
    x, ir = rc.data(c)
    for k, v in enumerate(c["valid"]):
        x[k, :, v:] = 0.0                                    # (the reference takes the live cells only; keep its input finite)
    for j, n in enumerate(c["lens"]):
        ir[j, n:] = 0.0
    y64, _, _, g64 = sf.reference(x, c["valid"], ir, c["lens"], c["index"], c["keep"])
    e = sf.cell_bound(x, c["valid"], ir, c["lens"], c["index"])
    got, gains = rc.simulated(name, sf.CT)
    B = len(c["valid"])
    if not c["keep"]:
        err = np.abs(got.astype(np.float64) - y64)
        print("%s: worst error / bound = %.3g" % (name, float((err / np.maximum(e, 1e-300)).max())))
        assert np.all(err <= e), (name, float(err.max()))
        assert np.all(gains == 1)
        return
    grel = sf.gain_rel(y64, e, c["valid"])
    scaled = g64 != 1
    rel = np.abs(gains.astype(np.float64) / g64 - 1)
    print("%s: worst |g / g_ref - 1| / bound = %.3g" % (name, float((rel / grel).max())))
    assert np.all(rel <= grel), (name, rel, grel)
    err = np.abs(got.astype(np.float64) - g64[:, None, None] * y64)
    bound = np.where(scaled[:, None, None], sf.scaled_bound(got, y64, g64, e, grel), e)
    print("%s: worst scaled error / bound = %.3g" % (name, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound), (name, float((err / np.maximum(bound, 1e-300)).max()))
    for k in range(B):                                       # the point of keep_power: the window's power is the dry signal's
        v = c["valid"][k]
        if scaled[k] and v:
            ex, ey = float((x[k, :, :v].astype(np.float64) ** 2).sum()), float((got[k, :, :v].astype(np.float64) ** 2).sum())
            assert abs(ey / ex - 1) < 1e-5, (name, k, ex, ey)


def test_the_constant_of_the_bound_is_the_derivation():
    """c(N, P) written out: sqrt N (rho + eps (1 + rho)) / u with eps = t eta / (1 - t eta), t = log2 N, eta = 7 u, and
    rho = sqrt 2 (2 eps + eps^2 + sqrt 2 gamma_2P (1 + eps)^2)."""
    assert (sf.N, sf.HOP, sf.LOG) == (2048, 1024, 11) and sf.ETA == 7 * 2.0 ** -24
    for P in (1, 3, 16, 64):
        assert abs(sf.c_of(P) / (45.2548 * (294.79 + 4.0 * P)) - 1) < 1e-3, (P, sf.c_of(P))


def test_a_row_alone_has_the_words_it_has_in_its_batch():
    """Locality: every (window, row) of the eight-row, six-window case -- three of its windows share a response --, convolved alone
    as a 1 x 1 batch in the other layout, gives the unscaled words it has in the batch."""
    name = "T%d_rows8_a1" % (rc.H + 5)
    c = rc.case(name)
    assert c["rows"] == 8 and len([j for j in c["index"] if j == 5]) == 3 and len({c["valid"][k] for k in range(6) if c["index"][k] == 5}) == 3
    x, ir = rc.data(c)
    B, rows, T = x.shape
    tc = np.zeros((B, T, rows), dtype=np.float32)
    assert sf.reverb_windows(rc.as_layout(x, sf.TC).copy(), c["valid"], ir, c["lens"], c["index"], sf.TC, tc, 0)
    out = rc.from_layout(tc, sf.TC)
    for k in range(B):
        j = c["index"][k]
        for r in range(rows):
            one = np.full((1, 1, T), 7.0, dtype=np.float32)
            row = x[k:k + 1, r:r + 1].copy()
            if j < 0:
                assert sf.reverb_windows(row, c["valid"][k:k + 1], None, None, [-1], sf.CT, one, 0)
            else:
                assert sf.reverb_windows(row, c["valid"][k:k + 1], ir[j:j + 1].copy(), c["lens"][j:j + 1], [0], sf.CT, one, 0)
            assert rc.same_words(one[0, 0], out[k, r]), (k, r)


def test_a_nan_tap_leaves_the_other_window_alone():
    c = rc.case("nan_tap")
    x, ir = rc.data(c)
    for layout in (sf.CT, sf.TC):
        got, gains = rc.simulated("nan_tap", layout)
        alone, g1 = sf.restate(x[1:2], c["valid"][1:2], ir, c["lens"], c["index"][1:2], c["keep"])
        assert np.all(np.isfinite(got[1])) and rc.same_words(got[1:2], alone) and rc.same_words(gains[1:2], g1)
        assert np.all(got[0, :, c["valid"][0]:].view(np.uint32) == 0)
        assert np.any(np.isnan(got[0]))                      # (the FFT form cannot keep a non-finite tap from the cells before it)


def test_shared_partitions_are_transformed_once():
    """Three windows that name one response of 2 H + 1 taps with 2 H + 3, 1 and 2 H + 2 live samples: the two whole partitions once,
    the ragged ends (2 H + 1 taps for two of them, one tap for the third) once each."""
    T = 2 * rc.H + 3
    x = np.ones((3, 1, T), dtype=np.float32)
    ir = np.ones((1, rc.K), dtype=np.float32)
    out = np.zeros_like(x)
    assert sf.reverb_windows(x, [T, 1, T - 1], ir, [2 * rc.H + 1], [0, 0, 0], sf.CT, out, 0)
    assert sf.LAST == dict(slots=3 * 3 + 4, jobs=4)
    e = sf.cell_bound(x, [T, 1, T - 1], ir, [2 * rc.H + 1], [0, 0, 0])
    assert np.all(np.abs(out[0, 0, :5] - [1, 2, 3, 4, 5]) <= e[0, 0, :5]) and abs(out[1, 0, 0] - 1) <= e[1, 0, 0] and np.all(out[1, 0, 1:] == 0)


def test_nothing_to_do_succeeds_and_launches_nothing():
    assert not sf.reverb_windows(None, None, None, None, None, sf.CT, None, shape=(0, 3, 5), n_ir=0)
    assert not sf.reverb_windows(None, None, None, None, None, sf.TC, None, 1, shape=(4, 3, 0), n_ir=2, K=9)
    x = np.full((2, 2, 9), 7.0, dtype=np.float32)
    x[1, :, 4:] = np.float32("nan")
    out = np.full_like(x, -3.0)
    g = np.full(2, -1.0, dtype=np.float32)
    assert sf.reverb_windows(x, [9, 4], None, None, [-1, -1], sf.CT, out, 1, g)     # no response anywhere: a copy, padding zeroed
    assert np.all(out[0] == 7.0) and np.all(out[1, :, :4] == 7.0) and np.all(out[1, :, 4:].view(np.uint32) == 0) and np.all(g == 1)


def _refusal_args():
    return dict(data=np.ones(2 * 3 * 5, dtype=np.float32), out=np.zeros(2 * 3 * 5, dtype=np.float32), ir=np.ones(2 * 4, dtype=np.float32), rows=3,
                valid=[5, 2], lens=[4, 1], index=[1, 0], layout=sf.CT, keep=None, reserved=0, reserved2=0, K=4, n_ir=2)


REFUSALS = [
    (dict(keep=2), "clx_reverb_windows_fft: opts->keep_power must be 0 or 1 and opts->reserved 0"),
    (dict(keep=1, reserved=4), "clx_reverb_windows_fft: opts->keep_power must be 0 or 1 and opts->reserved 0"),
    (dict(keep=0, reserved2=1), "clx_reverb_windows_fft: opts->keep_power must be 0 or 1 and opts->reserved 0"),
    (dict(layout=7), "clx_reverb_windows_fft: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
    (dict(rows=0), "clx_reverb_windows_fft: rows must be 1..8"),
    (dict(rows=9), "clx_reverb_windows_fft: rows must be 1..8"),
    (dict(K=0), "clx_reverb_windows_fft: K must be 1..65536"),
    (dict(K=65537), "clx_reverb_windows_fft: K must be 1..65536"),
    (dict(valid=None), "clx_reverb_windows_fft: null argument"),
    (dict(index=None), "clx_reverb_windows_fft: null argument"),
    (dict(data=None), "clx_reverb_windows_fft: null argument"),
    (dict(out=None), "clx_reverb_windows_fft: null argument"),
    (dict(ir=None), "clx_reverb_windows_fft: null argument"),
    (dict(lens=None), "clx_reverb_windows_fft: null argument"),
    (dict(valid=[3, 6]), "clx_reverb_windows_fft: valid[k] is larger than T"),
    (dict(lens=[4, 5]), "clx_reverb_windows_fft: ir_len[j] is larger than K"),
    (dict(index=[0, 2]), "clx_reverb_windows_fft: ir_index[k] must be -1 .. n_ir - 1"),
    (dict(index=[-2, 0]), "clx_reverb_windows_fft: ir_index[k] must be -1 .. n_ir - 1"),
    (dict(out="data"), "clx_reverb_windows_fft: d_out overlaps d_data"),
    (dict(out="data+7"), "clx_reverb_windows_fft: d_out overlaps d_data"),
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
        sf.reverb_windows(a["data"], a["valid"], a["ir"], a["lens"], a["index"], a["layout"], a["out"], a["keep"], shape=(2, a["rows"], 5),
                          n_ir=a["n_ir"], K=a["K"], reserved=a["reserved"], reserved2=a["reserved2"])
    assert str(e.value).endswith(text) or text in str(e.value)
    assert "clx_reverb_windows:" not in str(e.value)
    assert before is None or np.array_equal(before, a["out"])


def test_the_stated_sizes_are_the_sources():
    L = sf.lib()
    assert (L.sim_rvfft_hop(), L.sim_rvfft_n(), L.sim_rvfft_bins(), L.sim_rvfft_spec(), L.sim_rvfft_lds_bytes(), L.sim_rvfft_win_bytes()) \
        == (1024, 2048, 1025, 1040, 16384, 40)
    assert "clx_reverb_windows_fft" in cx.EXPORTS and cx.REVERB_METHODS == ("direct", "fft", "auto")
    tw = sf.twiddles().astype(np.float64)
    q = np.arange(sf.N // 2)
    assert np.array_equal(tw[:, 0], np.cos(2 * np.pi * q / sf.N).astype(np.float32)) or np.abs(tw[:, 0] - np.cos(2 * np.pi * q / sf.N)).max() <= 2.0 ** -24
    assert np.abs(tw[:, 1] + np.sin(2 * np.pi * q / sf.N)).max() <= 2.0 ** -24 and tw[0, 0] == 1 and tw[0, 1] == 0


def _bare_set(ctx, n_streams=2, channels=1):
    """A StreamSet as far as the refusals look at it: no device, no streams."""
    s = cx.StreamSet.__new__(cx.StreamSet)
    s.ctx, s._descs = ctx, np.zeros(0, dtype=cx.FRAME_DESC_DTYPE)
    s.problems, s.channels, s.sample_rates = [None] * n_streams, [channels] * n_streams, [16000] * n_streams
    s._lengths = np.full(n_streams, 100, dtype=np.int64)
    return s


def test_reverb_takes_a_method_and_shows_it():
    src = _bare_set(object())
    assert cx.Reverb([0, -1], src).method == "direct" and "method='direct'" in repr(cx.Reverb([0, -1], src))
    r = cx.Reverb([0, 1], src, taps=800, method="fft")
    assert r.method == "fft" and "method='fft'" in repr(r) and "2 windows" in repr(r)


@pytest.mark.parametrize("bad", ("FFT", "overlap-save", "", None, 1, True, b"fft"))
def test_a_method_that_is_neither_is_refused_before_any_device(bad):
    with pytest.raises(ValueError, match="method must be one of 'direct', 'fft', 'auto', not"):
        cx.Reverb([0], _bare_set(object()), method=bad)
    c = cx.Context.__new__(cx.Context)
    with pytest.raises(ValueError, match="reverb_windows: method must be one of 'direct', 'fft', 'auto', not"):
        c.reverb_windows((0, 2, 1, 4), [4, 4], (0, 1, 4), [4], [0, -1], cx.WINDOW_CT, out=0, method=bad)


def test_auto_chooses_by_the_taps_against_the_probed_constant():
    """REVERB_FFT_TAPS is the smallest probed tap count from which the FFT form's read beat the direct form's by more than the
    spread (profiles/reverb_fft_probe.txt)."""
    import json
    import os
    rows = [json.loads(l) for l in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "reverb_fft_probe.txt"))]
    wins = sorted(r["taps"] for r in rows if r["what"] == "ratio" and r["fft_faster_than_direct_beyond_spread"])
    assert wins and cx.REVERB_FFT_TAPS == wins[0] == 4000
    assert cx.reverb_method_for("auto", 3999) == "direct" and cx.reverb_method_for("auto", 4000) == "fft" and cx.reverb_method_for("auto", 65536) == "fft"
    assert cx.reverb_method_for("direct", 65536) == "direct" and cx.reverb_method_for("fft", 1) == "fft"
    assert cx.Reverb([0], _bare_set(object()), method="auto").method == "auto"
    with pytest.raises(ValueError):
        cx.reverb_method_for("fastest", 8)


def test_reverb_windows_fft_refuses_lengths_that_do_not_match():
    c = cx.Context.__new__(cx.Context)
    with pytest.raises(ValueError, match="valid has 1 entries for 2 windows"):
        c.reverb_windows((0, 2, 1, 4), [1], (0, 1, 4), [4], [0, -1], cx.WINDOW_CT, out=0, method="fft")
