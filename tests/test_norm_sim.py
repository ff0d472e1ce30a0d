"""clx_norm_windows under the wave simulator (tests/wavesim/sim_norm.cpp runs the production kernels of clx_norm.hip on host
buffers): over the edge matrix of norm_cases.py the simulator equals the numpy restatement of claxon_hip.h's definition bit for bit
-- cells and stats, in both layouts, which are therefore bit-equal to each other --, lies inside the float64 reference's interval
(DESIGN.md 4.15), leaves the guard bands alone and never reads a padding cell; every refusal has its text; and the Python side
(Norm, the normalize= arguments) refuses what it should before anything touches a device."""
import numpy as np
import pytest

import claxon_amd as cx
import norm_cases as nc
import simlib_norm as sn


@pytest.mark.parametrize("name", nc.NAMES)
def test_the_simulator_is_the_restatement_word_for_word(name):
    c = nc.case(name)
    x = nc.data(c)
    want, wstats = sn.restate(x, c["valid"], c["o"])
    for layout in (sn.CT, sn.TC):
        got, stats = nc.simulated(name, layout)
        assert nc.same_words(got, want), (name, layout, "cells")
        if c["stats"]:
            assert nc.same_words(stats, wstats), (name, layout, "stats")
    assert nc.same_words(nc.simulated(name, sn.CT)[0], nc.simulated(name, sn.TC)[0])
    for k, n in enumerate(c["valid"]):                       # (padding is pad, whatever it held)
        assert np.all(want[k, :, n:] == np.float32(c["o"]["pad"]))


@pytest.mark.parametrize("name", nc.NAMES)
def test_the_simulator_lies_inside_the_reference_interval(name):
    c = nc.case(name)
    x = nc.data(c)
    for k, n in enumerate(c["valid"]):
        x[k, :, n:] = 0.0                                    # (the reference takes the live cells only; keep its input finite)
    ref, mu, sc = sn.reference(x, c["valid"], c["o"])
    allow = sn.bound(x, c["valid"], c["o"])
    got, stats = nc.simulated(name, sn.CT)
    fin = np.isfinite(ref) & np.isfinite(allow)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err[fin] <= allow[fin]), (name, float(np.max(err[fin] / np.maximum(allow[fin], 1e-300))))
    assert np.array_equal(np.isnan(got), np.isnan(ref)) or c["kind"] == "constant"
    if c["kind"] == "normal" and c["o"]["var"] and c["o"]["mean"]:
        for k, n in enumerate(c["valid"]):                   # the point of it all: zero mean and unit variance over the live cells
            if n > 8:
                live = got[k, :, :n].astype(np.float64)
                assert np.all(np.abs(live.mean(axis=1)) < 1e-5) and np.all(np.abs(live.std(axis=1, ddof=c["o"]["ddof"]) - 1) < 1e-3)


def test_a_constant_row_with_eps_0_is_nan_and_a_lone_cell_with_ddof_1_has_variance_0():
    got, stats = nc.simulated("constant_row", sn.CT)
    assert np.all(np.isnan(got[0, 0, :70])) and np.all(np.isnan(got[1, 1, :70]))          # 0 / 0
    assert stats[0, 0, 0] == np.float32(1.25) and stats[0, 0, 1] == 0 and np.all(np.isfinite(got[0, 1, :70]))
    got, stats = nc.simulated("one_live_ddof1", sn.CT)
    assert np.all(stats[:2, :, 1] == 0) and np.all(np.isnan(got[:2, :, 0])) and np.all(got[:2, :, 1:] == 0)
    # not centred: x / 0 is +-Inf where x is not 0
    x = np.full((1, 1, 5), 2.0, dtype=np.float32)
    sn.norm_windows(x, [5], sn.CT, sn.opts(0, 1, 0, 0.0, 0.0))
    assert np.all(np.isposinf(x))


def test_an_empty_window_is_all_pad_and_its_stats_are_defined():
    x = np.full((2, 9, 2), 7.0, dtype=np.float32)            # [B, T, rows]
    st = np.zeros((2, 2, 2), dtype=np.float32)
    sn.norm_windows(x, [0, 0], sn.TC, sn.opts(1, 1, 0, 1e-7, -2.0), st)
    assert np.all(x == -2.0) and np.all(st[..., 0] == 0) and np.all(st[..., 1] == np.sqrt(np.float32(1e-7)))


def test_nothing_to_do_succeeds_and_touches_nothing():
    x = np.zeros((0, 2, 9), dtype=np.float32)
    sn.norm_windows(x, np.zeros(0, np.uint32), sn.CT, sn.opts())
    sn.norm_windows(None, None, sn.CT, sn.opts(), shape=(0, 3, 5))
    sn.norm_windows(None, None, sn.TC, sn.opts(), shape=(4, 3, 0))


REFUSALS = [
    (dict(o=None), "clx_norm_windows: null options"),
    (dict(o=sn.opts(mean=2)), "clx_norm_windows: mean must be 0 or 1"),
    (dict(o=sn.opts(var=2)), "clx_norm_windows: var must be 0 or 1"),
    (dict(o=sn.opts(ddof=2)), "clx_norm_windows: ddof must be 0 or 1"),
    (dict(o=sn.opts(0, 0)), "clx_norm_windows: mean and var are both 0: nothing to do"),
    (dict(o=sn.opts(eps=-1e-9)), "clx_norm_windows: eps must be finite and not negative"),
    (dict(o=sn.opts(eps=float("inf"))), "clx_norm_windows: eps must be finite and not negative"),
    (dict(o=sn.opts(eps=float("nan"))), "clx_norm_windows: eps must be finite and not negative"),
    (dict(o=sn.opts(pad=float("inf"))), "clx_norm_windows: pad must be finite"),
    (dict(o=sn.opts(pad=float("nan"))), "clx_norm_windows: pad must be finite"),
    (dict(layout=7), "clx_norm_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
    (dict(rows=0), "clx_norm_windows: rows must be 1..256"),
    (dict(rows=257), "clx_norm_windows: rows must be 1..256"),
    (dict(valid=[3, 6]), "clx_norm_windows: valid[k] is larger than T"),
    (dict(data=None), "clx_norm_windows: null argument"),
    (dict(valid=None), "clx_norm_windows: null argument"),
]


@pytest.mark.parametrize("change,text", REFUSALS)
def test_every_refusal_has_its_text_and_writes_nothing(change, text):
    a = dict(data=np.ones(2 * 3 * 5, dtype=np.float32), rows=3, valid=[5, 2], layout=sn.CT, o=sn.opts())
    a.update(change)
    before = None if a["data"] is None else a["data"].copy()
    with pytest.raises(cx.ClaxonError) as e:
        sn.norm_windows(a["data"], a["valid"], a["layout"], a["o"], shape=(2, a["rows"], 5))
    assert text in str(e.value)
    assert before is None or np.array_equal(before, a["data"])


def test_the_stated_sizes_are_the_sources():
    L = sn.lib()
    assert (L.sim_norm_chunk(), L.sim_norm_strands(), L.sim_norm_max_rows()) == (sn.CHUNK, sn.STRANDS, sn.MAX_ROWS) == (4096, 64, 256)
    assert sn.MAX_ROWS >= 256 >= 8                           # every n_out of a MelSpec (n_mels <= 256) and 1..8 channels


def test_norm_is_a_plain_value_with_the_three_named_constructors():
    n = cx.Norm()
    assert (n.mean, n.var, n.ddof, n.eps, n.pad) == (True, True, 0, 0.0, 0.0)
    w, c, s = cx.Norm.wav2vec2(), cx.Norm.cmvn(), cx.Norm.seamless()
    e = float(np.float32(1e-7))
    assert (w.mean, w.var, w.ddof, w.eps, w.pad) == (True, True, 0, e, 0.0)
    assert (c.mean, c.var, c.ddof, c.eps, c.pad) == (True, True, 0, 0.0, 0.0) and c == cx.Norm()
    assert (s.mean, s.var, s.ddof, s.eps, s.pad) == (True, True, 1, e, 0.0)
    m = cx.Norm.cmvn(vars=False)
    assert (m.mean, m.var) == (True, False) and cx.Norm.cmvn(means=False).mean is False
    assert sn.of_norm(cx.Norm(ddof=1, eps=1e-7, pad=-1)) == sn.opts(1, 1, 1, e, -1.0)
    assert "ddof=1" in repr(s)


@pytest.mark.parametrize("kw", [dict(mean=2), dict(var=-1), dict(ddof=2), dict(ddof=0.5), dict(mean="yes"), dict(mean=False, var=False),
                                dict(eps=-1e-9), dict(eps=float("inf")), dict(eps=float("nan")), dict(eps=1e39), dict(eps="0"),
                                dict(pad=float("inf")), dict(pad=float("nan")), dict(pad=None), dict(pad=True)])
def test_norm_refuses(kw):
    with pytest.raises(ValueError):
        cx.Norm(**kw)


def test_cmvn_means_off_and_vars_off_is_refused():
    with pytest.raises(ValueError):
        cx.Norm.cmvn(means=False, vars=False)


@pytest.mark.parametrize("bad", ["cmvn", True, 1, dict(mean=True), sn.opts()])
def test_read_and_read_mel_refuse_a_normalize_that_is_no_norm(bad):
    """(The refusal comes before anything else is looked at: no device, no stream set's state.)"""
    s = cx.StreamSet.__new__(cx.StreamSet)
    with pytest.raises(ValueError, match="normalize must be a Norm"):
        s.read([0], [0], 16, normalize=bad)
    with pytest.raises(ValueError, match="normalize must be a Norm"):
        s.read_mel([0], [0], 4, None, normalize=bad)
    c = cx.Context.__new__(cx.Context)
    with pytest.raises(ValueError, match="norm must be a Norm"):
        c.norm_windows((0, 1, 1, 1), [1], cx.WINDOW_CT, bad)
