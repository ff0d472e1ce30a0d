"""clx_add_windows under the wave simulator (tests/wavesim/sim_add.cpp runs the production kernels of clx_add.hip on host buffers):
over the edge matrix of add_cases.py the simulator equals the numpy restatement of claxon_hip.h's definition word for word -- cells
and gains, in both layouts, which are therefore bit-equal to each other --, padding and the cells behind the noise's end keep their
words, the noise is never written and no NaN parked behind a live range reaches a result; gains and cells lie inside the float64
reference's bounds; every refusal has its text; and the Python side (Add, the add= arguments, Context.add_windows)
refuses what it should before anything touches a device."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest

import add_cases as ac
import claxon_amd as cx
import simlib_add as sa

INF = float("inf")


@pytest.mark.parametrize("name", ac.NAMES)
def test_the_simulator_is_the_restatement_word_for_word(name):
    c = ac.case(name)
    x, n = ac.data(c)
    want, wgains = sa.restate(x, c["valid"], n, c["noise_valid"], c["index"], c["snr"])
    for layout in (sa.CT, sa.TC):
        got, gains = ac.simulated(name, layout)
        assert ac.same_words(got, want), (name, layout, "cells", int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))))
        assert ac.same_words(gains, wgains), (name, layout, "gains", gains, wgains)
    assert ac.same_words(ac.simulated(name, sa.CT)[0], ac.simulated(name, sa.TC)[0])
    xw, ww = x.view(np.uint32), want.view(np.uint32)
    for k, vs in enumerate(c["valid"]):
        j = c["index"][k]
        vn = min(c["noise_valid"][j], vs) if j >= 0 else 0
        assert np.all(ww[k, :, vs:] == ac.PAD_WORD), (name, k, "padding")
        assert np.array_equal(ww[k, :, vn:], xw[k, :, vn:]), (name, k, "cells behind the noise's end")
        assert not np.any(np.isnan(want[k, :, :vs])) and not np.isnan(wgains[k]), (name, k, "a NaN from behind a live range")
        if wgains[k] == 0:
            assert np.array_equal(ww[k], xw[k]), (name, k, "a window without a gain")


@pytest.mark.parametrize("name", ac.NAMES)
def test_gains_and_cells_lie_inside_the_reference_bounds(name):
    c = ac.case(name)
    x, n = ac.data(c)
    for k, v in enumerate(c["valid"]):
        x[k, :, v:] = 0.0                                    # (the reference takes the live cells only; keep its input finite)
    ref, gref, gn = sa.reference(x, c["valid"], n, c["noise_valid"], c["index"], c["snr"])
    got, gains = ac.simulated(name, sa.CT)
    hit = gref != 0                                          # neither energy is zero, some noise is live, q is not 0
    assert np.array_equal(hit, gains != 0), (name, gains, gref)
    rel = np.abs(gains[hit].astype(np.float64) / gref[hit] - 1)
    print("%s: worst |g / g_ref - 1| = %.3g of %.3g" % (name, rel.max() if rel.size else 0.0, sa.GAIN_REL))
    assert np.all(rel < sa.GAIN_REL), (name, float(rel.max()))
    for k in np.nonzero(hit)[0]:
        vs = c["valid"][k]
        err = np.abs(got[k, :, :vs].astype(np.float64) - ref[k, :, :vs])
        assert np.all(err <= sa.cell_bound(got[k, :, :vs], gn[k, :, :vs])), (name, int(k), float(err.max()))


def test_the_gain_sets_the_ratio_of_mean_powers():
    """The point of it all: after the call, 10 log10 of (the signal's mean power over Vs) / (the added part's over Vn) is snr_db --
    also for the window whose noise ends inside it --, and with +inf, index -1, an empty signal, no live noise, an all-zero noise
    and an all-zero signal nothing is added and the gain is +0.0."""
    for name in ("T65_rows3", "T4095_rows2", "snr_range", "zero_energy"):
        c = ac.case(name)
        x, n = ac.data(c)
        got, gains = ac.simulated(name, sa.CT)
        for k, vs in enumerate(c["valid"]):
            j = c["index"][k]
            vn = min(c["noise_valid"][j], vs) if j >= 0 else 0
            dead = j < 0 or vs == 0 or vn == 0 or math.isinf(c["snr"][k]) or (c["kind"] == "zeros" and k < 2)
            if dead:
                assert gains[k].view(np.uint32) == 0, (name, k)
                continue
            ps = float((x[k, :, :vs].astype(np.float64) ** 2).sum()) / vs
            pn = float(gains[k]) ** 2 * float((n[j, :, :vn].astype(np.float64) ** 2).sum()) / vn
            assert abs(10 * math.log10(ps / pn) - c["snr"][k]) < 1e-5, (name, k, ps, pn)
            if abs(c["snr"][k]) < 50:                        # (what was added is the noise times the gain, to the cells' rounding)
                d = got[k, :, :vn].astype(np.float64) - x[k, :, :vn] - float(gains[k]) * n[j, :, :vn].astype(np.float64)
                assert np.all(np.abs(d) <= 2.0 ** -24 * np.abs(got[k, :, :vn]) + 2.0 ** -149), (name, k)
    assert any(c["valid"][k] > min(c["noise_valid"][j], c["valid"][k]) > 0 for c in ac.MATRIX for k, j in enumerate(c["index"]) if j >= 0)


def test_two_windows_share_one_noise_window_with_their_own_live_parts():
    c = ac.case("T65_rows3")
    assert c["index"][0] == c["index"][2] == 0 and c["valid"][0] != c["valid"][2] and c["noise_valid"][0] > c["valid"][2]
    x, n = ac.data(c)
    got, gains = ac.simulated("T65_rows3", sa.TC)
    one, g1 = sa.restate(x[2:3], c["valid"][2:3], n, c["noise_valid"], [0], c["snr"][2:3])
    assert ac.same_words(got[2:3], one) and gains[2] == g1[0] != gains[0]


def test_fma32_is_libm_fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(5)
    n = (rng.standard_normal(4000) * 10.0 ** rng.integers(-42, 3, 4000)).astype(np.float32)
    x = (rng.standard_normal(4000) * 10.0 ** rng.integers(-42, 3, 4000)).astype(np.float32)
    x[::7] = -(np.float32(0.37) * n[::7])                    # (cancellation: the result is the product's own rounding error)
    g = np.float32(0.37)
    want = np.array([m.fmaf(float(g), float(a), float(b)) for a, b in zip(n, x)], dtype=np.float32)
    assert ac.same_words(sa.fma32(g, n, x), want)


def test_a_gain_beyond_float32_is_inf_and_stays_in_its_window():
    """Nothing is clamped (claxon_hip.h, `range`): a loud signal over subnormal noise at -200 dB rounds to g = +inf, the cells are
    IEEE's -- inf where the noise is not zero, NaN where it is --, and the window beside it is what it is alone."""
    x = np.full((2, 1, 8), 1e30, dtype=np.float32)
    x[1] = np.float32(0.5)
    n = np.full((2, 1, 8), 1e-44, dtype=np.float32)
    n[0, 0, 3] = 0.0
    n[1] = np.float32(0.25)
    want, wg = sa.restate(x, [8, 8], n, [8, 8], [0, 1], [-200.0, 0.0])
    g = np.zeros(2, dtype=np.float32)
    got = x.copy()
    assert sa.add_windows(got, [8, 8], n, [8, 8], [0, 1], [-200.0, 0.0], sa.CT, g)
    assert ac.same_words(got, want) and ac.same_words(g, wg)
    assert np.isposinf(g[0]) and np.isnan(got[0, 0, 3]) and np.all(np.isposinf(np.delete(got[0, 0], 3)))
    assert g[1] == 2.0 and np.all(got[1] == 1.0)


def test_nothing_to_do_succeeds_and_launches_nothing():
    x = np.full((2, 2, 9), 7.0, dtype=np.float32)
    n = np.full((1, 2, 9), 3.0, dtype=np.float32)
    g = np.full(2, -1.0, dtype=np.float32)
    assert not sa.add_windows(x, [9, 9], n, [9], [-1, -1], [0.0, 0.0], sa.CT, g)       # every index -1
    assert np.all(x == 7.0) and np.all(g == -1.0)
    assert not sa.add_windows(None, None, None, None, None, None, sa.CT, shape=(0, 3, 5), n_noise=0)
    assert not sa.add_windows(None, None, None, None, None, None, sa.TC, shape=(4, 3, 0), n_noise=2)
    assert not sa.add_windows(None, [5], None, None, [-1], [1.0], sa.TC, shape=(1, 3, 5), n_noise=0)   # (no work: the device pointers may be null)
    assert sa.add_windows(x, [9, 9], n, [9], [0, 0], [INF, INF], sa.CT, g, reserved=0)    # +inf everywhere: launched, nothing added
    assert np.all(x == 7.0) and np.all(g.view(np.uint32) == 0)


REFUSALS = [
    (dict(reserved=1), "clx_add_windows: opts must be NULL or all zero"),
    (dict(layout=7), "clx_add_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
    (dict(rows=0), "clx_add_windows: rows must be 1..8"),
    (dict(rows=9), "clx_add_windows: rows must be 1..8"),
    (dict(valid=None), "clx_add_windows: null argument"),
    (dict(index=None), "clx_add_windows: null argument"),
    (dict(snr=None), "clx_add_windows: null argument"),
    (dict(data=None), "clx_add_windows: null argument"),
    (dict(noise=None), "clx_add_windows: null argument"),
    (dict(noise_valid=None), "clx_add_windows: null argument"),
    (dict(valid=[3, 6]), "clx_add_windows: valid[k] is larger than T"),
    (dict(noise_valid=[5, 6]), "clx_add_windows: noise_valid[j] is larger than T"),
    (dict(index=[0, 2]), "clx_add_windows: noise_index[k] must be -1 .. n_noise - 1"),
    (dict(index=[-2, 0]), "clx_add_windows: noise_index[k] must be -1 .. n_noise - 1"),
    (dict(snr=[0.0, float("nan")]), "clx_add_windows: snr_db[k] is NaN"),
    (dict(snr=[-INF, 0.0]), "clx_add_windows: snr_db[k] must be within -200 .. 200, or +inf"),
    (dict(snr=[200.5, 0.0]), "clx_add_windows: snr_db[k] must be within -200 .. 200, or +inf"),
    (dict(snr=[0.0, -201.0]), "clx_add_windows: snr_db[k] must be within -200 .. 200, or +inf"),
]


@pytest.mark.parametrize("change,text", REFUSALS)
def test_every_refusal_has_its_text_and_writes_nothing(change, text):
    a = dict(data=np.ones(2 * 3 * 5, dtype=np.float32), noise=np.ones(2 * 3 * 5, dtype=np.float32), rows=3, valid=[5, 2], noise_valid=[5, 1],
             index=[1, 0], snr=[0.0, 3.0], layout=sa.CT, reserved=None)
    a.update(change)
    before = None if a["data"] is None else a["data"].copy()
    with pytest.raises(cx.ClaxonError) as e:
        sa.add_windows(a["data"], a["valid"], a["noise"], a["noise_valid"], a["index"], a["snr"], a["layout"], shape=(2, a["rows"], 5), n_noise=2,
                       reserved=a["reserved"])
    assert text in str(e.value)
    assert before is None or np.array_equal(before, a["data"])


def test_the_stated_sizes_are_the_sources():
    L = sa.lib()
    assert (L.sim_add_chunk(), L.sim_add_strands(), L.sim_add_max_rows(), L.sim_add_table_bytes()) == (sa.CHUNK, sa.STRANDS, sa.MAX_ROWS, 20) \
        == (4096, 64, 8, 20)
    assert "clx_add_windows" in cx.EXPORTS


def test_add_is_a_plain_value():
    a = cx.Add([0, -1, 2], [5, 0, 7], 10)
    assert len(a) == 3 and a.source is None and a.snr_db.dtype == np.float32 and a.snr_db.tolist() == [10.0, 10.0, 10.0]
    assert a.stream_ids.tolist() == [0, -1, 2] and a.starts.tolist() == [5, 0, 7]
    b = cx.Add([0, 1], [0, 0], [INF, -200.0])
    assert b.snr_db.tolist() == [INF, -200.0] and "2 windows" in repr(b)
    assert len(cx.Add([], [], 3.0)) == 0
    cx.Add([-1], [-5], 0.0)                                  # (the start of a window without noise is not looked at)


@pytest.mark.parametrize("args", [([0, 1], [0], 0.0), ([0], [0], [1.0, 2.0]), ([-2], [0], 0.0), ([0], [-1], 0.0), ([0], [0], float("nan")),
                                  ([0], [0], -INF), ([0], [0], 200.5), ([0, 0], [0, 0], [0.0, -300.0]), ([0], [0], 0.0, "a set")])
def test_add_refuses(args):
    with pytest.raises(ValueError):
        cx.Add(*args)


def _bare_set(ctx, n_streams=2, channels=1):
    """A StreamSet as far as the refusals look at it: no device, no streams."""
    s = cx.StreamSet.__new__(cx.StreamSet)
    s.ctx, s._descs = ctx, np.zeros(0, dtype=cx.FRAME_DESC_DTYPE)
    s.problems, s.channels, s.sample_rates = [None] * n_streams, [channels] * n_streams, [16000] * n_streams
    s._lengths = np.full(n_streams, 100, dtype=np.int64)
    return s


def test_read_and_read_mel_refuse_a_bad_add_before_any_work():
    ctx, other = object(), object()
    s = _bare_set(ctx)
    for bad in ("noise", 3, dict(snr_db=0), cx.Norm()):
        with pytest.raises(ValueError, match="add must be an Add"):
            s.read([0], [0], 16, add=bad)
        with pytest.raises(ValueError, match="add must be an Add"):
            s.read_mel([0], [0], 4, None, add=bad)
    with pytest.raises(ValueError, match="add has 1 windows, the call 2"):
        s.read([0, 1], [0, 0], 16, add=cx.Add([0], [0], 0.0))
    with pytest.raises(ValueError, match="a stream its source does not have"):
        s.read([0, 1], [0, 0], 16, add=cx.Add([0, 2], [0, 0], 0.0))
    with pytest.raises(ValueError, match="another context"):
        s.read([0], [0], 16, add=cx.Add([0], [0], 0.0, source=_bare_set(other)))
    closed = _bare_set(ctx)
    closed.close()
    with pytest.raises(ValueError, match="source is closed"):
        s.read([0], [0], 16, add=cx.Add([0], [0], 0.0, source=closed))
    with pytest.raises(ValueError, match="noise stream 1 has 2 channels, the windows 1"):
        s.read([0], [0], 16, add=cx.Add([1], [0], 0.0, source=_bare_set(ctx, channels=2)))


@pytest.mark.parametrize("kw,text", [
    (dict(valid=[1]), "valid has 1 entries for 2 windows"), (dict(noise_index=[0]), "noise_index has 1 entries"),
    (dict(snr_db=[1.0, 2.0, 3.0]), "snr_db has 3 entries"), (dict(noise_valid=[1, 1]), "noise_valid has 2 entries for 1 windows")])
def test_add_windows_refuses_lengths_that_do_not_match(kw, text):
    c = cx.Context.__new__(cx.Context)
    a = dict(valid=[4, 4], noise_valid=[4], noise_index=[0, -1], snr_db=0.0)
    a.update(kw)
    with pytest.raises(ValueError, match=text):
        c.add_windows((0, 2, 1, 4), a["valid"], (0, 1), a["noise_valid"], a["noise_index"], a["snr_db"], cx.WINDOW_CT)
