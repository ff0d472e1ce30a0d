"""clx_addn_windows under the wave simulator (tests/wavesim/sim_addn.cpp runs the production kernels of clx_addn.hip on host
buffers): over the edge matrix of addn_cases.py the simulator equals the numpy restatement of claxon_hip.h's definition word for
word -- cells and gains, in both layouts --, padding and the cells no term covers keep their words, no noise is written and no NaN
parked behind a live range reaches a result; gains and cells lie inside the float64 reference's bounds; one term a
window at offset 0 without loop is clx_add_windows word for word; a looped term is the unlooped one on a noise tiled by the host;
every refusal has its text; and the Python side (Add's offsets and tile, add=[...], Context.addn_windows) refuses what it should
before anything touches a device."""
import numpy as np
import pytest

import add_cases as ac
import addn_cases as dc
import claxon_amd as cx
import simlib_add as sa
import simlib_addn as sd
from test_add_sim import _bare_set

INF = float("inf")


@pytest.mark.parametrize("name", dc.NAMES)
def test_the_simulator_is_the_restatement_word_for_word(name):
    c = dc.case(name)
    x, noises = dc.data(c)
    want, wgains = sd.restate(x, c["valid"], noises, c["noise_valid"], c["terms"])
    for layout in (sd.CT, sd.TC):
        got, gains = dc.simulated(name, layout)
        assert dc.same_words(got, want), (name, layout, "cells", int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))))
        assert dc.same_words(gains, wgains), (name, layout, "gains", gains, wgains)
    xw, ww = x.view(np.uint32), want.view(np.uint32)
    m = 0
    for k, vs in enumerate(c["valid"]):
        reached = np.zeros(c["T"], dtype=bool)
        for term in c["terms"][k]:
            off, end, _ = sd.cover(term, vs, c["noise_valid"])
            if wgains[m] != 0:
                reached[off:end] = True
            m += 1
        assert np.all(ww[k, :, vs:] == ac.PAD_WORD), (name, k, "padding")
        assert np.array_equal(ww[k][:, ~reached], xw[k][:, ~reached]), (name, k, "cells no live term covers")
        assert not np.any(np.isnan(want[k, :, :vs])), (name, k, "a NaN from behind a live range")
    assert not np.any(np.isnan(wgains)), name


@pytest.mark.parametrize("name", dc.NAMES)
def test_gains_and_cells_lie_inside_the_reference_bounds(name):
    c = dc.case(name)
    x, noises = dc.data(c)
    for k, v in enumerate(c["valid"]):
        x[k, :, v:] = 0.0                                    # (the reference takes the live cells only; keep its input finite)
    for n, nv in zip(noises, c["noise_valid"]):
        for j, v in enumerate(nv):
            n[j, :, v:] = 0.0
    ref, gref, gn, cnt = sd.reference(x, c["valid"], noises, c["noise_valid"], c["terms"])
    got, gains = dc.simulated(name, sd.CT)
    hit = gref != 0
    assert np.array_equal(hit, gains != 0), (name, gains, gref)
    rel = np.abs(gains[hit].astype(np.float64) / gref[hit] - 1)
    print("%s: worst |g / g_ref - 1| = %.3g of %.3g" % (name, rel.max() if rel.size else 0.0, sd.GAIN_REL))
    assert np.all(rel < sd.GAIN_REL), (name, float(rel.max()))
    for k, vs in enumerate(c["valid"]):
        err = np.abs(got[k, :, :vs].astype(np.float64) - ref[k, :, :vs])
        bound = sd.cell_bound(x[k, :, :vs], gn[k, :, :vs], cnt[k, :, :vs])
        assert np.all(err <= bound), (name, k, float(err.max()))
    assert cnt.max() <= sd.MAX_TERMS


def test_the_matrix_holds_what_it_says():
    """The axes of the edge matrix are in it, counted over terms that are live -- an index, a finite snr, a cover that is not empty:
    every period looped at least twice round, from offset 0 and from offset 3; a looped P > Vs; the offsets 0, 1, 3, 4095, 4096 and
    Vs - 1 with a cover, Vs and above without; 0, 1, 2 and 16 terms a window; two batches; Vs of 0, 1 and T; every pair of word
    offsets.  And the matrix runs: one case through the simulator."""
    twice, offsets, dead_offsets, counts, p_above, vs_seen = {0: set(), 3: set()}, set(), set(), set(), False, set()
    for c in dc.MATRIX:
        for k, w in enumerate(c["terms"]):
            counts.add(len(w))
            vs = c["valid"][k]
            vs_seen.add("0" if vs == 0 else "1" if vs == 1 else "T" if vs == c["T"] else "")
            for term in w:
                off, end, P = sd.cover(term, vs, c["noise_valid"])
                if term[1] < 0 or np.isinf(term[4]):
                    continue
                if end == off:
                    dead_offsets.add("Vs" if off == vs else "above" if off > vs else off)
                    continue
                offsets.add("Vs-1" if off == vs - 1 else off)
                if term[3] and end - off >= 2 * P and off in twice:
                    twice[off].add(P)
                p_above = p_above or bool(term[3] and P > vs)
    assert set(dc.PERIODS) <= twice[0] and set(dc.PERIODS) <= twice[3], twice
    assert p_above
    assert {0, 1, 3, sd.CHUNK - 1, sd.CHUNK, "Vs-1"} <= offsets and {"Vs", "above"} <= dead_offsets
    assert {0, 1, 2, 16} <= counts and {"0", "1", "T"} <= vs_seen
    assert any(len(c["noise_valid"]) == 2 for c in dc.MATRIX)
    assert {(c["offset"], c["noise_offsets"][0]) for c in dc.MATRIX} >= {(a, b) for a in range(4) for b in range(4)}
    cells, gains = dc.simulated("disjoint", sd.CT)
    assert gains.size == sum(len(w) for w in dc.case("disjoint")["terms"]) and np.all(gains != 0)


@pytest.mark.parametrize("name", ac.NAMES)
def test_one_plain_term_a_window_is_clx_add_windows_word_for_word(name):
    """Every case of add_cases.py as one term a window with offset 0 and no loop: clx_add_windows' simulated gains and cells."""
    c = ac.case(name)
    x, n = ac.data(c)
    d = dict(name=name, offset=c["offset"], noise_offsets=[c["noise_offset"]], noise_valid=[c["noise_valid"]],
             terms=[[(0, j, 0, 0, s)] for j, s in zip(c["index"], c["snr"])])
    for layout in (sd.CT, sd.TC):
        want, wgains = ac.simulated(name, layout)
        got, gains, launched = dc.run(d, x, [n], layout, dc._sim_call(c["valid"], layout))
        assert launched and dc.same_words(got, want) and dc.same_words(gains, wgains), (name, layout)


@pytest.mark.parametrize("name", ["T65_rows3", "T4097_rows2", "offsets_1_2", "loops_T12296_rows1", "loops_T12296_rows3"])
def test_a_looped_term_is_the_unlooped_one_on_a_noise_tiled_by_the_host(name):
    c = dc.case(name)
    x, noises = dc.data(c)
    T = c["T"]
    tiled, tiled_valid = [], []
    for n, nv in zip(noises, c["noise_valid"]):
        t = n.copy()
        for j, P in enumerate(nv):
            if P:
                t[j] = n[j][:, np.arange(T) % P]
        tiled.append(t)
        tiled_valid.append([T if P else 0 for P in nv])
    # (an unlooped term keeps its own noise window: the tiled ones go into further batches that only the looped terms name)
    nb = len(noises)
    d = dict(c, noise_valid=c["noise_valid"] + tiled_valid, noise_offsets=c["noise_offsets"] + c["noise_offsets"],
             terms=[[(b + nb, j, off, 0, s) if lp and j >= 0 else (b, j, off, lp, s) for b, j, off, lp, s in w] for w in c["terms"]])
    assert any(lp for w in c["terms"] for _, _, _, lp, _ in w) and not any(lp for w in d["terms"] for _, j, _, lp, _ in w if j >= 0)
    for layout in (sd.CT, sd.TC):
        want, wgains = dc.simulated(name, layout)
        got, gains, _ = dc.run(d, x, noises + tiled, layout, dc._sim_call(c["valid"], layout))
        assert dc.same_words(got, want) and dc.same_words(gains, wgains), (name, layout)


def test_every_gain_is_taken_from_the_signal_as_it_arrives():
    """Two terms on one window: each gain is what the term gets alone -- the second does not see the first in the signal -- and the
    ratio of mean powers over the cells that meet is the term's snr, a looped noise counted as often as it sounds."""
    c = dc.case("T65_rows3")
    x, noises = dc.data(c)
    _, gains = dc.simulated("T65_rows3", sd.CT)
    first, _ = sd.flatten(c["terms"])
    for k in (0, 5):
        vs = c["valid"][k]
        for i, term in enumerate(c["terms"][k]):
            _, alone = sd.restate(x[k:k + 1], [vs], noises, c["noise_valid"], [[term]])
            assert dc.same_words(alone, gains[first[k] + i:first[k] + i + 1]), (k, i)
            off, end, P = sd.cover(term, vs, c["noise_valid"])
            heard = noises[term[0]][term[1]][:, np.arange(end - off) % P].astype(np.float64)
            ps = float((x[k, :, :vs].astype(np.float64) ** 2).sum()) / vs
            pn = float(alone[0]) ** 2 * float((heard ** 2).sum()) / (end - off)
            assert abs(10 * np.log10(ps / pn) - term[4]) < 1e-5, (k, i)


def test_nothing_to_do_succeeds_and_launches_nothing():
    x = np.full((2, 2, 9), 7.0, dtype=np.float32)
    n = np.full((1, 2, 9), 3.0, dtype=np.float32)
    g = np.full(2, -1.0, dtype=np.float32)
    first, terms = sd.flatten([[(0, -1, 0, 0, 0.0)], [(5, -1, 2, 1, 1.0)]])              # every index -1 (the batch is not looked at)
    assert not sd.addn_windows(x, [9, 9], [n], [9], first, terms, sd.CT, g)
    first0, terms0 = sd.flatten([[], []])                                                # no terms at all
    assert not sd.addn_windows(x, [9, 9], [n], [9], first0, terms0, sd.CT, g)
    assert np.all(x == 7.0) and np.all(g == -1.0)
    assert not sd.addn_windows(None, None, None, None, None, None, sd.CT, shape=(0, 3, 5), n_noise=[])
    assert not sd.addn_windows(None, None, None, None, None, None, sd.TC, shape=(4, 3, 0), n_noise=[2])
    first, terms = sd.flatten([[(0, 0, 0, 1, INF)], [(0, 0, 9, 1, 0.0), (0, 0, 3, 0, INF)]])     # +inf, an offset at Vs: launched, nothing added
    g = np.full(3, -1.0, dtype=np.float32)
    assert sd.addn_windows(x, [9, 9], [n], [9], first, terms, sd.CT, g, reserved=0)
    assert np.all(x == 7.0) and np.all(g.view(np.uint32) == 0)


_T2 = [[(0, 1, 0, 0, 0.0)], [(0, 0, 1, 1, 3.0)]]
REFUSALS = [
    (dict(reserved=1), "clx_addn_windows: opts must be NULL or all zero"),
    (dict(layout=7), "clx_addn_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
    (dict(rows=0), "clx_addn_windows: rows must be 1..8"),
    (dict(rows=9), "clx_addn_windows: rows must be 1..8"),
    (dict(n_batches=9), "clx_addn_windows: more than 8 noise batches"),
    (dict(valid=None), "clx_addn_windows: valid is null"),
    (dict(first=None), "clx_addn_windows: term_first is null"),
    (dict(flat=None), "clx_addn_windows: terms is null"),
    (dict(data=None), "clx_addn_windows: d_data is null"),
    (dict(noises=None), "clx_addn_windows: d_noise is null"),
    (dict(noises=[None]), "clx_addn_windows: a term names a noise batch whose pointer is null"),
    (dict(noise_valid=None), "clx_addn_windows: noise_valid is null"),
    (dict(null_counts=True), "clx_addn_windows: n_noise is null"),
    (dict(first=[1, 1, 2]), "clx_addn_windows: term_first[0] must be 0"),
    (dict(first=[0, 2, 1]), "clx_addn_windows: term_first must not descend"),
    (dict(terms=[[(0, 0, 0, 0, 0.0)] * 17, []]), "clx_addn_windows: more than 16 terms in a window"),
    (dict(valid=[3, 6]), "clx_addn_windows: valid[k] is larger than T"),
    (dict(noise_valid=[5, 6]), "clx_addn_windows: noise_valid[j] is larger than T"),
    (dict(terms=[[(0, 2, 0, 0, 0.0)], []]), "clx_addn_windows: terms[m].index is outside its batch (n_noise[batch])"),
    (dict(terms=[[(0, -2, 0, 0, 0.0)], []]), "clx_addn_windows: terms[m].index is below -1"),
    (dict(terms=[[(1, 0, 0, 0, 0.0)], []]), "clx_addn_windows: terms[m].batch must be 0 .. n_batches - 1"),
    (dict(terms=[[(-1, 0, 0, 0, 0.0)], []]), "clx_addn_windows: terms[m].batch must be 0 .. n_batches - 1"),
    (dict(terms=[[(0, 0, 0, 2, 0.0)], []]), "clx_addn_windows: terms[m].loop must be 0 or 1"),
    (dict(terms=[[(0, 0, 0, 0, float("nan"))], []]), "clx_addn_windows: terms[m].snr_db is NaN"),
    (dict(terms=[[(0, 0, 0, 0, -INF)], []]), "clx_addn_windows: terms[m].snr_db must be within -200 .. 200, or +inf"),
    (dict(terms=[[(0, 0, 0, 0, 200.5)], []]), "clx_addn_windows: terms[m].snr_db must be within -200 .. 200, or +inf"),
    (dict(terms=[[], [(0, 0, 0, 1, -201.0)]]), "clx_addn_windows: terms[m].snr_db must be within -200 .. 200, or +inf"),
]


@pytest.mark.parametrize("change,text", REFUSALS)
def test_every_refusal_has_its_text_and_writes_nothing(change, text):
    a = dict(data=np.ones(2 * 3 * 5, dtype=np.float32), noises=[np.ones(2 * 3 * 5, dtype=np.float32)], rows=3, valid=[5, 2], noise_valid=[5, 1],
             terms=_T2, layout=sd.CT, reserved=None, n_batches=None, null_counts=False)
    a.update(change)
    first, flat = sd.flatten(a["terms"])
    first, flat = a.get("first", first), a.get("flat", flat)
    before = None if a["data"] is None else a["data"].copy()
    with pytest.raises(cx.ClaxonError) as e:
        sd.addn_windows(a["data"], a["valid"], a["noises"], a["noise_valid"], first, flat, a["layout"], shape=(2, a["rows"], 5), n_noise=[2],
                        reserved=a["reserved"], n_batches=a["n_batches"], null_counts=a["null_counts"])
    assert text in str(e.value)
    assert before is None or np.array_equal(before, a["data"])


def test_the_stated_sizes_are_the_sources():
    L = sd.lib()
    assert (L.sim_addn_max_terms(), L.sim_addn_max_batches(), L.sim_addn_max_rows(), L.sim_addn_rec_bytes(), L.sim_addn_term_bytes()) \
        == (sd.MAX_TERMS, sd.MAX_BATCHES, sd.MAX_ROWS, 32, cx.ADDN_TERM_DTYPE.itemsize) == (16, 8, 8, 32, 20)
    assert (cx.ADDN_MAX_TERMS, cx.ADDN_MAX_BATCHES) == (16, 8)
    assert "clx_addn_windows" in cx.EXPORTS


def test_add_takes_offsets_and_tile():
    a = cx.Add([0, -1, 2], [5, 0, 7], 10)
    assert a.plain and a.offsets.tolist() == [0, 0, 0] and a.tile.tolist() == [False] * 3
    b = cx.Add([0, 1], [0, 0], 3.0, offsets=[0, 16000], tile=True)
    assert not b.plain and b.offsets.tolist() == [0, 16000] and b.tile.tolist() == [True, True]
    assert not cx.Add([0], [0], 0.0, offsets=1).plain and not cx.Add([0, 1], [0, 0], 0.0, tile=[False, True]).plain
    assert cx.Add([0, 1], [0, 0], 0.0, offsets=[0, 0], tile=[False, False]).plain


@pytest.mark.parametrize("kw", [dict(offsets=-1), dict(offsets=[0, -3]), dict(offsets=[0]), dict(offsets=[0, 1, 2]), dict(tile=[True]),
                                dict(tile=[True, False, True]), dict(offsets=1.5), dict(tile=1), dict(offsets=[[0, 1]]), dict(tile="yes")])
def test_add_refuses_bad_offsets_and_tiles(kw):
    with pytest.raises(ValueError):
        cx.Add([0, 1], [0, 0], 0.0, **kw)


def test_read_and_read_mel_refuse_a_bad_list_before_any_work():
    ctx = object()
    s = _bare_set(ctx)
    one = cx.Add([0], [0], 0.0)
    for bad in ([], [one] * 17, [one, "noise"], (one, None)):
        with pytest.raises(ValueError, match="add must be an Add, a list of 1..16 Adds or None"):
            s.read([0], [0], 16, add=bad)
        with pytest.raises(ValueError, match="add must be an Add, a list of 1..16 Adds or None"):
            s.read_mel([0], [0], 4, None, add=bad)
    with pytest.raises(ValueError, match="add has 2 windows, the call 1"):            # (the refusals of Add._plan, per Add)
        s.read([0], [0], 16, add=[one, cx.Add([0, 1], [0, 0], 0.0)])
    with pytest.raises(ValueError, match="a stream its source does not have"):
        s.read([0], [0], 16, add=[one, cx.Add([2], [0], 0.0, tile=True)])
    with pytest.raises(ValueError, match="another context"):
        s.read([0], [0], 16, add=[cx.Add([0], [0], 0.0, source=_bare_set(object()))])
    with pytest.raises(ValueError, match="more than 8 distinct sources"):
        s.read([0], [0], 16, add=[cx.Add([0], [0], 0.0, source=_bare_set(ctx)) for _ in range(9)])


@pytest.mark.parametrize("kw,text", [
    (dict(valid=[1]), "valid has 1 entries for 2 windows"), (dict(term_first=[0, 1]), "term_first has 2 entries for 2 windows"),
    (dict(noise_valid=[1, 1]), "noise_valid has 2 entries for 1 windows"), (dict(index=[0]), "index has 1 entries for 2 terms"),
    (dict(snr_db=[1.0, 2.0, 3.0]), "snr_db has 3 entries for 2 terms"), (dict(offset=[0, -1]), "offset is out of range"),
    (dict(offset=[0, 1 << 32]), "offset is out of range")])
def test_addn_windows_refuses_lengths_that_do_not_match(kw, text):
    c = cx.Context.__new__(cx.Context)
    a = dict(valid=[4, 4], noise_valid=[4], term_first=[0, 1, 2], batch=0, index=[0, -1], offset=0, loop=0, snr_db=0.0)
    a.update(kw)
    with pytest.raises(ValueError, match=text):
        c.addn_windows((0, 2, 1, 4), a["valid"], [(0, 1)], a["noise_valid"], a["term_first"], a["batch"], a["index"], a["offset"], a["loop"],
                       a["snr_db"], cx.WINDOW_CT)
