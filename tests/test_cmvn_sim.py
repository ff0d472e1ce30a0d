"""Global and sliding-window CMVN (clx_cmvn.hip, unmodified) under the wave simulator, on the CPU: over the cases of cmvn_cases.py the
production kernels equal the numpy restatements of claxon_hip.h word for word in both layouts, guard words included; every cell
lies within DESIGN.md 4.22's bound of the exact reference; the statistics window obeys its rule for every (t, V); a centred window
that covers the utterance is clx_norm_windows' mean removal within both bounds; the global step is (x + shift) * scale in numpy
float32 and nothing is fused; padding is never read; clx_cmvn_from_stats is one float64 numpy line; every refusal has its own text
and launches nothing; and the Cmvn value checks what it is given."""
import math

import numpy as np
import pytest

import claxon_amd as cx
import cmvn_cases as cc
import simlib_cmvn as sc
import simlib_norm as sn

LAYOUTS = (sc.CT, sc.TC)


# ---- sliding ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.SLIDING_NAMES)
def test_sliding_is_the_restatement_word_for_word_in_both_layouts(name):
    want = cc.restated_sliding(name)
    ct, tc = cc.simulated_sliding(name, sc.CT), cc.simulated_sliding(name, sc.TC)
    assert cc.same_words(ct, want), (name, int(np.count_nonzero(ct.view(np.uint32) != want.view(np.uint32))))
    assert cc.same_words(tc, want), (name, int(np.count_nonzero(tc.view(np.uint32) != want.view(np.uint32))))
    assert cc.same_words(ct, tc)
    c = cc.sliding_case(name)
    for k, V in enumerate(c["valid"]):                       # padding is the pad, whatever the input held there
        assert np.all(ct[k, :, V:] == np.float32(c["pad"]))


@pytest.mark.parametrize("name", cc.FINITE_NAMES)
def test_sliding_lies_within_the_bound_of_the_exact_reference(name):
    """Log-mel-like cells: the reference's own variance stays far above the 1e-10 floor, so no bound is infinite."""
    c = cc.sliding_case(name)
    y, allow, vmin = sc.reference_sliding(cc.data(c), c["valid"], c["N"], c["M"], c["center"], c["norm_vars"], c["pad"])
    assert np.all(np.isfinite(allow)), (name, "a variance reaches the floor")
    got = cc.simulated_sliding(name, sc.CT).astype(np.float64)
    err = np.abs(got - y)
    worst = float(np.max(err / np.maximum(allow, 2.0 ** -149)))
    print("%s: worst |cell - reference| / bound %.3f, least variance %g" % (name, worst, vmin))
    assert np.all(err <= allow), (name, worst)


def test_the_wide_cases_show_the_order():
    """In the cases with cancelling pairs of magnitude 2^50 the double sums round where the float32 cell shows it: adding the same
    cells in plain ascending order gives other words, so the word-for-word tests above do hold the ORDER."""
    c = cc.sliding_case("wide_c1_v0")
    x = cc.data(c)
    want = cc.restated_sliding("wide_c1_v0")
    V = c["valid"][0]
    differs = 0
    for t in range(V):
        a, b = sc.window(t, V, c["N"], c["M"], c["center"])
        s = np.zeros(x.shape[1])
        for u in range(a, b):
            s = s + x[0, :, u].astype(np.float64)
        plain = (x[0, :, t].astype(np.float64) - s / np.float64(b - a)).astype(np.float32)
        differs += int(np.count_nonzero(plain.view(np.uint32) != want[0, :, t].view(np.uint32)))
    print("%d cells differ from the plain ascending sum" % differs)
    assert differs > 0


CONFIGS = [(N, M, center) for N in cc.WINDOWS for M in sorted({1, N, min(100, N)}) for center in (0, 1)]


@pytest.mark.parametrize("N,M,center", CONFIGS)
def test_the_window_rule_for_every_t_and_V(N, M, center):
    """Index only: the production rule (clx_cmvn::stat_window) is the stated one, and the stated one has the properties of Kaldi's."""
    Vs = sorted({v for v in (1, 2, 31, 32, 33, M - 1, M, M + 1, N - 1, N, N + 1, 2 * N, 256, 257, cc.T3) if 1 <= v <= 2100})
    for V in Vs:
        step = 1 if V <= 600 else 7
        for t in list(range(0, V, step)) + [V - 1]:
            a, b = sc.window(t, V, N, M, center)
            assert (a, b) == sc.sim_window(t, V, N, M, center), (t, V)
            assert 0 <= a <= t < b <= V and b - a <= N + 1, (t, V, a, b)
            if center and V >= N:
                assert b - a == N, (t, V, a, b)
            if not center and t >= N:
                assert (a, b) == (t - N, t + 1), (t, V, a, b)
            if not center and t + 1 < M <= V:
                assert b == M and a == 0, (t, V, a, b)
            if V <= min(N, M) or (center and V <= N):
                assert (a, b) == (0, V), (t, V, a, b)


def test_a_centred_window_over_the_utterance_is_mean_removal():
    """center, N >= 2 V, no variance: x - mean over [0, V), which is clx_norm_windows(mean, no var) -- in another order of the
    sum and with a float32 mean, so within the sum of both derived bounds and not word for word."""
    rng = np.random.default_rng(22)
    B, rows, T = 4, 5, 300
    valid = [300, 257, 33, 1]
    x = (rng.standard_normal((B, rows, T)) * 2.0 - 5.0).astype(np.float32)
    for k, V in enumerate(valid):
        x[k, :, V:] = 0.0
    o = sn.opts(1, 0, 0, 0.0, 0.0)
    for layout in LAYOUTS:
        src = cc.as_layout(x, layout)
        got = cc.from_layout(sc.sliding_windows(src, np.empty_like(src), valid, layout, 600, 1, 1, 0), layout)
        norm = cc.from_layout(sn.norm_windows(src.copy(), valid, layout, o), layout)
        y, allow, _ = sc.reference_sliding(x, valid, 600, 1, 1, 0)
        other = sn.bound(x, valid, o)
        err = np.abs(got.astype(np.float64) - norm.astype(np.float64))
        assert np.all(np.abs(got - y) <= allow)
        assert np.all(err <= allow + other), float(np.max(err - allow - other))
        assert float(np.max(err)) < 1e-5


def test_a_window_of_one_frame():
    """N = 1 centred: every window is the cell itself, so y = x - x = +0.0 (and with norm_vars n == 1 leaves it alone)."""
    x = np.array([[[1.5, -2.0, 3.25, 7.0]]], dtype=np.float32)
    for nv in (0, 1):
        got = sc.sliding_windows(x, np.empty_like(x), [3], sc.CT, 1, 1, 1, nv, pad=9.0)
        assert got.tolist() == [[[0.0, 0.0, 0.0, 9.0]]]


# ---- global -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.GLOBAL_NAMES)
def test_global_is_numpy_float32_word_for_word_in_both_layouts(name):
    c = cc.global_case(name)
    x, shift, scale = cc.global_data(c)
    want = sc.restate_global(x, c["valid"], shift, scale, c["pad"])
    with np.errstate(invalid="ignore"):                   # (the padding holds signalling NaNs)
        plain = (x + shift[None, :, None]) * scale[None, :, None]        # numpy float32, the whole batch at once
    for k, V in enumerate(c["valid"]):
        assert cc.same_words(want[k, :, :V], plain[k, :, :V])
        assert np.all(want[k, :, V:].view(np.uint32) == np.float32(c["pad"]).view(np.uint32))   # not the signalling patterns
    ct, tc = cc.simulated_global(name, sc.CT), cc.simulated_global(name, sc.TC)
    assert cc.same_words(ct, want), (name, int(np.count_nonzero(ct.view(np.uint32) != want.view(np.uint32))))
    assert cc.same_words(tc, want), (name, int(np.count_nonzero(tc.view(np.uint32) != want.view(np.uint32))))


def test_global_is_two_roundings_and_not_one_fused():
    """fmaf(x, scale, shift * scale) and the exactly rounded (x + shift) * scale differ from the two-step result in many cells."""
    c = cc.global_case("g_rows3")
    x, shift, scale = cc.global_data(c)
    V = c["valid"][0]
    got = cc.simulated_global("g_rows3", sc.CT)[0, :, :V]
    x64, sh, scl = x[0, :, :V].astype(np.float64), shift[:, None].astype(np.float64), scale[:, None].astype(np.float64)
    fused_a = ((x64 + sh) * scl).astype(np.float32)                      # one rounding of the exact value (the product is exact in double)
    fused_b = (x64 * scl + (shift * scale)[:, None].astype(np.float64)).astype(np.float32)    # fmaf(x, scale, fl32(shift * scale))
    assert np.count_nonzero(got != fused_a) > 0 and np.count_nonzero(got != fused_b) > 0
    assert np.max(np.abs(got - fused_a)) <= 2.0 ** -22 * np.max(np.abs(fused_a))


# ---- the accumulator --------------------------------------------------------------------------------------------------------------

def _stats(rows, seed=5, count=12345.0):
    rng = np.random.default_rng(seed)
    mean, std = rng.uniform(-8, 3, rows), rng.uniform(0.5, 4, rows)
    st = np.zeros((2, rows + 1))
    st[0, :rows], st[0, rows], st[1, :rows] = mean * count, count, (std * std + mean * mean) * count
    return st


@pytest.mark.parametrize("norm_vars", (True, False))
def test_from_stats_is_one_float64_line(norm_vars):
    st = _stats(80)
    st[1, 3] = 0.0                                           # a row whose variance comes out negative: the 1e-20 floor
    shift, scale = sc.from_stats(st, norm_vars)
    want_shift, want_scale = sc.from_stats64(st, norm_vars)
    assert cc.same_words(shift, want_shift) and cc.same_words(scale, want_scale)
    c = cx.Cmvn.from_kaldi_stats(st, norm_vars=norm_vars, pad=2.0)
    assert c.rows == 80 and c.pad == 2.0 and cc.same_words(c.shift, want_shift) and cc.same_words(c.scale, want_scale)
    if norm_vars:
        assert scale[3] == np.float32(1e10)
    else:
        assert np.all(scale == 1.0)


def test_from_stats_refuses_a_count_that_is_not_above_zero():
    for count in (0.0, -1.0, math.nan):
        st = _stats(4, count=1.0)
        st[0, 4] = count
        with pytest.raises(cx.ClaxonError, match="clx_cmvn_from_stats: the count must be above 0"):
            sc.from_stats(st)
        with pytest.raises(ValueError, match="count above 0"):
            cx.Cmvn.from_kaldi_stats(st)
    assert cx.lib().clx_cmvn_from_stats(None, 4, 1, None, None) == cx.API_ERROR


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _g(**kw):
    """A legal global call with one thing changed."""
    a = dict(data=np.zeros((2, 3, 8), dtype=np.float32), valid=[8, 2], layout=sc.CT, shift=np.zeros(3, np.float32), scale=np.ones(3, np.float32),
             pad=0.0, shape=None, opts=True, reserved=0)
    a.update(kw)
    return sc.global_windows(a["data"], a["valid"], a["layout"], a["shift"], a["scale"], a["pad"], a["shape"], a["opts"], a["reserved"])


def _s(**kw):
    """A legal sliding call with one thing changed."""
    x = np.zeros((2, 3, 8), dtype=np.float32)
    a = dict(data=x, out=np.zeros_like(x), valid=[8, 2], layout=sc.CT, window=4, min_window=2, center=0, norm_vars=0, pad=0.0, shape=None, opts=True,
             reserved=0)
    a.update(kw)
    return sc.sliding_windows(a["data"], a["out"], a["valid"], a["layout"], a["window"], a["min_window"], a["center"], a["norm_vars"], a["pad"],
                              a["shape"], a["opts"], a["reserved"])


_X = np.zeros((2, 3, 8), dtype=np.float32)
_BIG = np.zeros(1 << 23, dtype=np.uint32)                    # valid[] of the call with too many tiles (all zero: V = 0)
GLOBAL_REFUSALS = [
    (dict(opts=False), "clx_cmvn_global_windows: null options"),
    (dict(reserved=1), "clx_cmvn_global_windows: reserved must be 0"),
    (dict(pad=math.inf), "clx_cmvn_global_windows: pad must be finite"),
    (dict(pad=math.nan), "clx_cmvn_global_windows: pad must be finite"),
    (dict(layout=7), "clx_cmvn_global_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
    (dict(shape=(2, 0, 8)), "clx_cmvn_global_windows: rows must be 1..8192"),
    (dict(shape=(2, 8193, 8)), "clx_cmvn_global_windows: rows must be 1..8192"),
    (dict(shape=(2, 3, 1 << 31)), "clx_cmvn_global_windows: T must be below 2\\^31"),
    (dict(shift=None), "clx_cmvn_global_windows: null shift"),
    (dict(scale=None), "clx_cmvn_global_windows: null scale"),
    (dict(shift=np.array([0, math.nan, 0], np.float32)), "clx_cmvn_global_windows: shift must be finite"),
    (dict(scale=np.array([1, 1, math.inf], np.float32)), "clx_cmvn_global_windows: scale must be finite"),
    (dict(data=None, shape=(2, 3, 8)), "clx_cmvn_global_windows: null argument"),
    (dict(valid=None), "clx_cmvn_global_windows: null argument"),
    (dict(valid=[8, 9]), "clx_cmvn_global_windows: valid\\[k\\] is larger than T"),
    (dict(valid=_BIG, shape=(1 << 23, 8192, 129), shift=np.zeros(8192, np.float32), scale=np.ones(8192, np.float32)),
     "clx_cmvn_global_windows: too many tiles in one call"),
]
SLIDING_REFUSALS = [
    (dict(opts=False), "clx_cmvn_sliding_windows: null options"),
    (dict(reserved=1), "clx_cmvn_sliding_windows: reserved must be 0"),
    (dict(pad=-math.inf), "clx_cmvn_sliding_windows: pad must be finite"),
    (dict(layout=7), "clx_cmvn_sliding_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
    (dict(shape=(2, 0, 8)), "clx_cmvn_sliding_windows: rows must be 1..8192"),
    (dict(shape=(2, 8193, 8)), "clx_cmvn_sliding_windows: rows must be 1..8192"),
    (dict(shape=(2, 3, 1 << 31)), "clx_cmvn_sliding_windows: T must be below 2\\^31"),
    (dict(window=0), "clx_cmvn_sliding_windows: window must be 1..1024"),
    (dict(window=1025), "clx_cmvn_sliding_windows: window must be 1..1024"),
    (dict(min_window=0), "clx_cmvn_sliding_windows: min_window must be 1..window"),
    (dict(min_window=5), "clx_cmvn_sliding_windows: min_window must be 1..window"),
    (dict(center=2), "clx_cmvn_sliding_windows: center must be 0 or 1"),
    (dict(norm_vars=2), "clx_cmvn_sliding_windows: norm_vars must be 0 or 1"),
    (dict(data=None, shape=(2, 3, 8)), "clx_cmvn_sliding_windows: null argument"),
    (dict(out=None, shape=(2, 3, 8)), "clx_cmvn_sliding_windows: null argument"),
    (dict(valid=None), "clx_cmvn_sliding_windows: null argument"),
    (dict(data=_X, out=_X), "clx_cmvn_sliding_windows: d_out must not be d_in"),
    (dict(valid=[8, 9]), "clx_cmvn_sliding_windows: valid\\[k\\] is larger than T"),
    (dict(valid=_BIG, shape=(1 << 23, 3, 65537)), "clx_cmvn_sliding_windows: too many tiles in one call"),
]


@pytest.mark.parametrize("change,text", GLOBAL_REFUSALS, ids=[t.split(": ")[1][:28] + str(i) for i, (_, t) in enumerate(GLOBAL_REFUSALS)])
def test_every_global_refusal_has_its_own_text_and_launches_nothing(change, text):
    before = sc.launches()
    with pytest.raises(cx.ClaxonError, match="^.*" + text + "$"):
        _g(**change)
    assert sc.launches() == before


@pytest.mark.parametrize("change,text", SLIDING_REFUSALS, ids=[t.split(": ")[1][:28] + str(i) for i, (_, t) in enumerate(SLIDING_REFUSALS)])
def test_every_sliding_refusal_has_its_own_text_and_launches_nothing(change, text):
    before = sc.launches()
    with pytest.raises(cx.ClaxonError, match="^.*" + text + "$"):
        _s(**change)
    assert sc.launches() == before


def test_the_refusal_texts_differ_and_empty_calls_launch_nothing():
    assert len({t for _, t in GLOBAL_REFUSALS}) == 13 and len({t for _, t in SLIDING_REFUSALS}) == 14
    before = sc.launches()
    _g(data=None, valid=None, shape=(0, 3, 8))
    _g(data=None, valid=None, shape=(2, 3, 0))
    _s(data=None, out=None, valid=None, shape=(0, 3, 8))
    _s(data=None, out=None, valid=None, shape=(2, 3, 0))
    _s(center=1, min_window=0)                               # (min_window is only read when center == 0)
    assert sc.launches() == before + 1


# ---- the Python value -------------------------------------------------------------------------------------------------------------

def test_the_cmvn_value():
    g = cx.Cmvn.global_([1.0, 2.0], [0.5, 0.25], pad=-1.0)
    assert g.rows == 2 and g.pad == -1.0 and g.shift.tolist() == [1.0, 2.0] and g.scale.tolist() == [0.5, 0.25]
    assert g == cx.Cmvn.global_(np.array([1, 2]), np.array([0.5, 0.25], dtype=np.float32), pad=-1.0) and hash(g) == hash(cx.Cmvn.global_([1, 2], [0.5, 0.25], -1.0))
    assert g != cx.Cmvn.global_([1.0, 2.0], [0.5, 0.5], pad=-1.0) and g != cx.Cmvn.global_([1.0, 2.0], [0.5, 0.25]) and "2 rows" in repr(g)
    m = cx.Cmvn.from_mean_std([1.0, -2.0], [3.0, 0.1])
    assert m.shift.tolist() == [-1.0, 2.0] and cc.same_words(m.scale, (1.0 / np.array([3.0, 0.1])).astype(np.float32))
    s = cx.Cmvn.sliding()
    assert (s.rows, s.window, s.min_window, s.center, s.norm_vars, s.pad) == (None, 600, 100, False, False, 0.0) and s.shift is None
    x = cx.Cmvn.xvector()
    assert x == cx.Cmvn.sliding(300, 100, True, False) and hash(x) == hash(cx.Cmvn.sliding(300, 100, True)) and x != s and x != g
    assert "window=300" in repr(x) and "center=True" in repr(x)
    for bad in (lambda: cx.Cmvn.global_([1.0], [1.0, 2.0]), lambda: cx.Cmvn.global_([], []), lambda: cx.Cmvn.global_([math.nan], [1.0]),
                lambda: cx.Cmvn.global_([1.0], [1e39]), lambda: cx.Cmvn.global_(np.zeros(8193), np.ones(8193)), lambda: cx.Cmvn.global_("ab", [1.0, 2.0]),
                lambda: cx.Cmvn.global_([1.0], [1.0], pad=math.inf), lambda: cx.Cmvn.from_mean_std([0.0], [0.0]), lambda: cx.Cmvn.from_mean_std([0.0], [-1.0]),
                lambda: cx.Cmvn.from_kaldi_stats(np.zeros((3, 4))), lambda: cx.Cmvn.from_kaldi_stats(np.zeros((2, 1))), lambda: cx.Cmvn.from_kaldi_stats(np.zeros((2, 4))),
                lambda: cx.Cmvn.sliding(0), lambda: cx.Cmvn.sliding(1025), lambda: cx.Cmvn.sliding(50, 51), lambda: cx.Cmvn.sliding(50, 0),
                lambda: cx.Cmvn.sliding(50.0), lambda: cx.Cmvn.sliding(50, 10, center=2), lambda: cx.Cmvn.sliding(50, 10, norm_vars="yes"),
                lambda: cx.Cmvn.sliding(pad=math.nan), lambda: cx.Cmvn(), lambda: cx.Cmvn(shift=[1.0]), lambda: cx.Cmvn(shift=[1.0], scale=[1.0], window=5)):
        with pytest.raises(ValueError, match="^Cmvn: "):
            bad()
