"""clx_cmvn_stats_windows and clx_cmvn_grouped_windows under the wave simulator (CPU): the five kernels of clx_cmvn_stats.hip equal
a numpy restatement of claxon_hip.h's ORDER word for word, in both layouts, for a reset, for accumulating calls and for three
calls in a row; the chunk partials are clx_norm's; the sums lie within DESIGN.md 4.24's bound of exact arithmetic; padding is not
read; absent groups keep their words or become zeros; the solve is clx_cmvn_from_stats; the apply is clx_k_cmvn_global with one
group and numpy's float32 expression with several; every refusal has its own text."""
import ctypes as C
import math

import numpy as np
import pytest

import claxon_amd as cx
import cmvn_stats_cases as cc
import simlib_cmvn as sc
import simlib_cmvn_stats as ss
import simlib_norm as sn

CT, TC = ss.CT, ss.TC


def test_the_constants_are_the_sources():
    L = ss.lib()
    assert L.sim_cmvn_stats_threads() == ss.THREADS == 256 and L.sim_cmvn_stats_chunk() == ss.CHUNK == sn.CHUNK
    assert L.sim_cmvn_stats_strands() == ss.STRANDS == sn.STRANDS and L.sim_cmvn_stats_vecs() == ss.VECS
    assert L.sim_cmvn_stats_max_groups() == ss.MAX_GROUPS == cx.CMVN_MAX_GROUPS


@pytest.mark.parametrize("name", cc.NAMES)
def test_a_reset_call_is_the_restated_order_word_for_word_in_both_layouts(name):
    c = cc.case(name)
    want = cc.restated_stats(name)
    ct, tc = cc.simulated_stats(name, CT), cc.simulated_stats(name, TC)
    assert cc.same_words64(ct, tc), (name, "CT and TC differ")
    if c["kind"] == "nonfinite":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(ct), nan) and np.any(nan[0]) and not np.any(nan[1:]), name
        ct, want = np.where(nan, 0.0, ct), np.where(nan, 0.0, want)
    assert cc.same_words64(ct, want), (name, int(np.count_nonzero(ct.view(np.uint64) != want.view(np.uint64))))
    rows = c["rows"]
    groups = c["groups"] or [0] * len(c["valid"])
    for g in range(min(c["n_groups"], 8)):
        assert ct[g, 0, rows] == sum(v for v, gg in zip(c["valid"], groups) if gg == g), (name, g, "the count")
    assert np.all(ct[:, 1, rows].view(np.uint64) == 0), (name, "the unused word is +0.0 behind a reset")


@pytest.mark.parametrize("name", ["T65", "T4097", "unsorted", "rows80", "many_groups"])
def test_three_calls_in_a_row_accumulate_in_the_restated_order(name):
    want = cc.restated_stats(name, 3)
    for layout in cc.LAYOUTS:
        got = cc.simulated_stats(name, layout, 3)
        assert cc.same_words64(got, want), (name, layout)
    assert not cc.same_words64(want, cc.restated_stats(name, 1))


def test_an_accumulating_call_adds_to_what_is_there_and_absent_groups_keep_their_words():
    c = cc.case("unsorted")                                   # group 3 has no window, group 1 one without a live frame
    x = cc.data(c)
    rows = c["rows"]
    rng = np.random.default_rng(5)
    old = rng.uniform(-50, 50, cc.stats_shape(c))
    old[1] = -0.0                                            # (group 1 adds +0.0 to each word: -0.0 becomes +0.0, and that is in the ORDER)
    flat, body = cc.guarded64(old.size)
    body[:] = old.reshape(-1)
    ss.stats_windows(x, c["valid"], CT, c["groups"], c["n_groups"], body, accumulate=True)
    got = body.reshape(old.shape)
    assert cc.guards_intact64(flat, old.size)
    assert cc.same_words64(got[3], old[3]), "a group without a window changed"
    assert cc.same_words64(got[:, 1, rows], old[:, 1, rows]), "the unused word was written by an accumulating call"
    want = ss.restate_stats(x, c["valid"], c["groups"], c["n_groups"], old, True)
    assert cc.same_words64(got, want)
    assert np.all(got[1, :, :rows].view(np.uint64) == 0) and not np.any(got[0, :, :rows] == old[0, :, :rows])
    # a reset: the absent group and the group without a live frame become zeros
    ss.stats_windows(x, c["valid"], CT, c["groups"], c["n_groups"], body, accumulate=False)
    assert np.all(got[3].view(np.uint64) == 0) and np.all(got[1].view(np.uint64) == 0)
    # a reset over no window at all still zeroes, an accumulating call over none launches nothing and writes nothing
    body[:] = old.reshape(-1)
    n = ss.launches()
    ss.stats_windows(None, None, CT, None, c["n_groups"], body, accumulate=True, shape=(0, rows, 9))
    ss.stats_windows(x, c["valid"], CT, c["groups"], c["n_groups"], body, accumulate=True, shape=(len(c["valid"]), rows, 0))
    assert cc.same_words64(got, old) and ss.launches() == n
    ss.stats_windows(None, None, CT, None, c["n_groups"], body, accumulate=False, shape=(0, rows, 0))
    assert np.all(body.view(np.uint64) == 0) and ss.launches() == n and cc.guards_intact64(flat, old.size)


def test_every_window_of_group_minus_one_launches_nothing_and_changes_nothing():
    c = cc.case("T65")
    x = cc.data(c)
    flat, body = cc.guarded64(int(np.prod(cc.stats_shape(c))))
    body[:] = 1.5
    n = ss.launches()
    ss.stats_windows(x, c["valid"], CT, [-1] * len(c["valid"]), 1, body, accumulate=True)
    assert np.all(body == 1.5) and ss.launches() == n


def test_the_hosts_group_lists_are_a_stable_counting_sort():
    assert ss.table([5, 5, 5, 5, 5, 0], [2, 0, 2, -1, 0, 1], 4) == ([2, 0, 1], [0, 2, 4, 5], [0, 2, 1, 4, 5])
    assert ss.table([1, 1, 1], None, 1) == ([0], [0, 3], [0, 1, 2])
    assert ss.table([1, 1], [65535, 0], 65536) == ([65535, 0], [0, 1, 2], [0, 1])
    assert ss.table([1, 1], [-1, -1], 3) == ([], [0], [])


@pytest.mark.parametrize("layout", cc.LAYOUTS)
@pytest.mark.parametrize("name", ["T65", "T4097", "T8193", "rows80", "T64"])
def test_the_chunk_sums_are_clx_norms_own_partials_word_for_word(name, layout):
    c = cc.case(name)
    x = cc.data(c)
    mine, norms = ss.partials(cc.as_layout(x, layout), c["valid"], layout, shape=x.shape)
    written = ~np.isnan(norms[:, :, 0])
    assert np.any(written) and np.array_equal(written, ~np.isnan(mine[:, :, 0])) and np.array_equal(written, ~np.isnan(mine[:, :, 1]))
    assert np.all(np.isnan(norms[:, :, 1]))
    for k, V in enumerate(c["valid"]):                       # a chunk without a live cell is not written
        assert np.all(written[k] == (np.arange(mine.shape[3]) * ss.CHUNK < V)[None, :]), (name, k)
    assert np.array_equal(mine[:, :, 0][written].view(np.uint64), norms[:, :, 0][written].view(np.uint64))


def test_the_mean_clx_norm_reports_is_the_one_chunk_sum_divided():
    c = cc.case("T65")                                       # one chunk a row: clx_norm's m = (float)(S_0 / n), through simlib_norm
    x = cc.data(c)
    mine, _ = ss.partials(x, c["valid"], CT)
    B, rows, T = x.shape
    stats = np.zeros((B, rows, 2), dtype=np.float32)
    body = x.copy()
    for k, V in enumerate(c["valid"]):
        body[k, :, V:] = 0.0
    sn.norm_windows(body, c["valid"], CT, sn.opts(1, 0, 0, 0.0, 0.0), stats)
    for k, V in enumerate(c["valid"]):
        if V:
            assert np.array_equal(stats[k, :, 0].view(np.uint32), (mine[k, :, 0, 0] / np.float64(V)).astype(np.float32).view(np.uint32)), k


@pytest.mark.parametrize("name", cc.FINITE)
def test_the_sums_lie_within_the_derived_bound_of_exact_arithmetic(name):
    c = cc.case(name)
    if c["n_groups"] > 16:                                   # (the two groups that have windows; the others are zeros)
        c = dict(c, groups=[1, 0], n_groups=2)
        got = np.stack([cc.simulated_stats(name, CT)[0], cc.simulated_stats(name, CT)[65535]])
    else:
        got = cc.simulated_stats(name, CT)
    x = cc.data(c)
    E, A = ss.exact(x, c["valid"], c["groups"], c["n_groups"])
    groups = c["groups"] or [0] * len(c["valid"])
    n_added = [sum(1 for g in groups if g == j) for j in range(c["n_groups"])]       # N of DESIGN.md 4.24: the group's own windows
    allow = ss.bound(A, E, -(-c["T"] // ss.CHUNK), n_added)
    err = np.abs(got[:, :, :-1] - E[:, :, :-1])
    worst = float((err / np.maximum(allow, 1e-300)).max())
    print("%s: worst error / allowance %.3g, widest allowance %.3g" % (name, worst, float(allow.max())))
    assert np.all(err <= allow), (name, worst)
    assert np.array_equal(got[:, 0, -1], E[:, 0, -1]), (name, "the count is exact")


def test_padding_cells_are_never_read():
    c = cc.case("T4097")
    x = cc.data(c)
    y = x.copy()
    for k, V in enumerate(c["valid"]):
        y[k, :, V:] = np.float32(1e30)                       # another padding: were one cell read, a sum would differ
    for layout in cc.LAYOUTS:
        acc = np.zeros(cc.stats_shape(c))
        ss.stats_windows(cc.as_layout(y, layout), c["valid"], layout, c["groups"], c["n_groups"], acc, accumulate=False, shape=x.shape)
        assert cc.same_words64(acc, cc.simulated_stats("T4097", layout)), layout
        assert not np.any(np.isnan(cc.simulated_stats("T4097", layout)))


@pytest.mark.parametrize("norm_vars", (0, 1))
def test_the_solve_is_clx_cmvn_from_stats_word_for_word(norm_vars):
    L = cx.lib()
    for name in ("T65", "rows80", "T4097", "rows560"):
        st = cc.simulated_stats(name, CT).copy()
        rows = st.shape[2] - 1
        st[:, 1, 0] = st[:, 0, 0] ** 2 / np.maximum(st[:, 0, rows], 1.0)       # a row whose variance is at the floor
        got = ss.solve(st, norm_vars)
        assert cc.same_words(got, ss.solve64(st, norm_vars)), name
        for g in range(st.shape[0]):
            if not st[g, 0, rows] > 0:
                assert np.all(got[g, 0].view(np.uint32) == 0) and np.all(got[g, 1] == 1.0), (name, g, "an empty group is (+0.0, 1.0)")
                continue
            shift, scale = np.zeros(rows, dtype=np.float32), np.zeros(rows, dtype=np.float32)
            one = np.ascontiguousarray(st[g])
            assert L.clx_cmvn_from_stats(one.ctypes.data, rows, norm_vars, shift.ctypes.data, scale.ctypes.data) == cx.OK
            assert cc.same_words(got[g, 0], shift) and cc.same_words(got[g, 1], scale), (name, g)
            s2, c2 = sc.from_stats(one, norm_vars)
            assert cc.same_words(got[g, 0], s2) and cc.same_words(got[g, 1], c2), (name, g)
    assert any(not cc.simulated_stats(n, CT)[g, 0, -1] > 0 for n in ("T4097",) for g in range(4))


def test_the_solve_of_statistics_that_are_not_finite_is_ieee_in_that_group_only():
    st = cc.simulated_stats("nonfinite", CT)
    got = ss.solve(st, 1)
    want = ss.solve64(st, 1)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.any(nan[0]) and not np.any(nan[1:])
    assert cc.same_words(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want))
    assert np.all(got[2, 0].view(np.uint32) == 0) and np.all(got[2, 1] == 1.0)


@pytest.mark.parametrize("layout", cc.LAYOUTS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_the_grouped_apply_is_numpys_float32_expression_word_for_word(name, layout):
    c = cc.case(name)
    cells, shsc = cc.simulated_grouped(name, layout)
    st = cc.simulated_stats(name, CT)
    want_ss = ss.solve64(st, c["norm_vars"])
    x = cc.data(c)
    if c["kind"] == "nonfinite":
        want = ss.restate_grouped(x, c["valid"], c["groups"], want_ss, c["pad"])
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(cells), nan) and np.any(nan[0]) and not np.any(nan[1:]), (name, "only the window of the group with the NaN")
        assert cc.same_words(np.where(nan, np.float32(0), cells), np.where(nan, np.float32(0), want))
        return
    assert cc.same_words(shsc, want_ss), name
    want = ss.restate_grouped(x, c["valid"], c["groups"], shsc, c["pad"])
    assert cc.same_words(cells, want), (name, layout, int(np.count_nonzero(cells.view(np.uint32) != want.view(np.uint32))))
    for k, g in enumerate(c["groups"] or []):
        if g < 0:
            V = c["valid"][k]
            assert V > 0 and cc.same_words(cells[k, :, :V], x[k, :, :V]), (name, "group -1 keeps its live words")
            assert np.all(cells[k, :, V:] == np.float32(c["pad"]))


@pytest.mark.parametrize("layout", cc.LAYOUTS)
@pytest.mark.parametrize("name", ["T1", "T65", "T4096", "rows560"])
def test_one_group_is_the_simulated_global_kernel_with_the_same_shift_and_scale(name, layout):
    c = cc.case(name)
    assert c["groups"] is None and c["n_groups"] == 1
    cells, shsc = cc.simulated_grouped(name, layout)
    x = cc.data(c)
    B, rows, T = x.shape
    flat, body = cc.guarded(x.size, c["offset"])
    body[...] = cc.as_layout(x, layout).reshape(-1)
    sc.global_windows(body, c["valid"], layout, shsc[0, 0], shsc[0, 1], c["pad"], shape=x.shape)
    want = cc.from_layout(body.reshape((B, T, rows) if layout == TC else (B, rows, T)).copy(), layout)
    assert cc.same_words(cells, want), (name, layout)


def _stats_call(**kw):
    c = cc.case("T65")
    x = cc.data(c)
    a = dict(data=x, valid=c["valid"], layout=CT, groups=None, n_groups=1, stats=np.zeros(cc.stats_shape(c)), accumulate=True, shape=None,
             opts=True, reserved=0)
    a.update(kw)
    return ss.stats_windows(a["data"], a["valid"], a["layout"], a["groups"], a["n_groups"], a["stats"], a["accumulate"], a["shape"], a["opts"],
                            a["reserved"])


def _grouped_call(**kw):
    c = cc.case("T65")
    x = cc.data(c)
    a = dict(data=x, valid=c["valid"], layout=CT, groups=None, n_groups=1, stats=np.zeros(cc.stats_shape(c)), ss=np.zeros(2 * c["rows"], np.float32),
             norm_vars=1, pad=0.0, shape=None, opts=True, reserved=0)
    a.update(kw)
    return ss.grouped_windows(a["data"], a["valid"], a["layout"], a["groups"], a["n_groups"], a["stats"], a["ss"], a["norm_vars"], a["pad"],
                              a["shape"], a["opts"], a["reserved"])


def test_every_refusal_has_its_own_text():
    B = len(cc.case("T65")["valid"])
    misaligned = np.zeros(64).ctypes.data + 4
    stats_refusals = [
        (dict(opts=False), "clx_cmvn_stats_windows: null options"),
        (dict(reserved=1), "clx_cmvn_stats_windows: reserved must be 0"),
        (dict(accumulate=2), "clx_cmvn_stats_windows: accumulate must be 0 or 1"),
        (dict(layout=7), "clx_cmvn_stats_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
        (dict(shape=(B, 0, 65)), "clx_cmvn_stats_windows: rows must be 1..8192"),
        (dict(shape=(B, 8193, 65)), "clx_cmvn_stats_windows: rows must be 1..8192"),
        (dict(n_groups=0), "clx_cmvn_stats_windows: n_groups must be 1..65536"),
        (dict(n_groups=65537), "clx_cmvn_stats_windows: n_groups must be 1..65536"),
        (dict(stats=None), "clx_cmvn_stats_windows: null d_stats"),
        (dict(stats=misaligned), "clx_cmvn_stats_windows: d_stats must be 8-byte aligned"),
        (dict(data=None, shape=(B, 16, 65)), "clx_cmvn_stats_windows: null d_data"),
        (dict(valid=None, shape=(B, 16, 65)), "clx_cmvn_stats_windows: null valid"),
        (dict(valid=[65, 66, 1, 0, 65]), "clx_cmvn_stats_windows: valid\\[k\\] is larger than T"),
        (dict(groups=[0, 0, 1, 0, 0]), "clx_cmvn_stats_windows: group\\[k\\] must be -1..n_groups - 1"),
        (dict(groups=[0, 0, -2, 0, 0]), "clx_cmvn_stats_windows: group\\[k\\] must be -1..n_groups - 1"),
        (dict(shape=(1 << 20, 8192, 65)), "clx_cmvn_stats_windows: too many blocks in one call"),
    ]
    grouped_refusals = [
        (dict(opts=False), "clx_cmvn_grouped_windows: null options"),
        (dict(reserved=1), "clx_cmvn_grouped_windows: reserved must be 0"),
        (dict(norm_vars=2), "clx_cmvn_grouped_windows: norm_vars must be 0 or 1"),
        (dict(pad=math.inf), "clx_cmvn_grouped_windows: pad must be finite"),
        (dict(pad=math.nan), "clx_cmvn_grouped_windows: pad must be finite"),
        (dict(layout=7), "clx_cmvn_grouped_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
        (dict(shape=(B, 0, 65)), "clx_cmvn_grouped_windows: rows must be 1..8192"),
        (dict(shape=(B, 16, 1 << 31)), "clx_cmvn_grouped_windows: T must be below 2\\^31"),
        (dict(n_groups=0), "clx_cmvn_grouped_windows: n_groups must be 1..65536"),
        (dict(stats=None), "clx_cmvn_grouped_windows: null d_stats"),
        (dict(stats=misaligned), "clx_cmvn_grouped_windows: d_stats must be 8-byte aligned"),
        (dict(ss=None), "clx_cmvn_grouped_windows: null d_shift_scale"),
        (dict(ss=misaligned - 2), "clx_cmvn_grouped_windows: d_shift_scale must be 4-byte aligned"),
        (dict(data=None, shape=(B, 16, 65)), "clx_cmvn_grouped_windows: null d_data"),
        (dict(valid=None, shape=(B, 16, 65)), "clx_cmvn_grouped_windows: null valid"),
        (dict(valid=[65, 66, 1, 0, 65]), "clx_cmvn_grouped_windows: valid\\[k\\] is larger than T"),
        (dict(groups=[0, 0, 1, 0, 0]), "clx_cmvn_grouped_windows: group\\[k\\] must be -1..n_groups - 1"),
        (dict(shape=(1 << 20, 8192, 1 << 20)), "clx_cmvn_grouped_windows: too many blocks in one call"),
    ]
    n = ss.launches()
    for kw, text in stats_refusals:
        if "shape" in kw and kw["shape"][0] > B:             # (refused before anything of the arrays is read past B .. by its count alone)
            kw = dict(kw, valid=np.zeros(kw["shape"][0], np.uint32))
        with pytest.raises(cx.ClaxonError, match=text):
            _stats_call(**kw)
    for kw, text in grouped_refusals:
        if "shape" in kw and kw["shape"][0] > B:
            kw = dict(kw, valid=np.zeros(kw["shape"][0], np.uint32))
        with pytest.raises(cx.ClaxonError, match=text):
            _grouped_call(**kw)
    assert ss.launches() == n
    assert len({t for _, t in stats_refusals}) == 13 and len({t for _, t in grouped_refusals}) == 17     # each its own text
    # n_windows == 0 and T == 0 succeed and launch nothing
    _grouped_call(data=None, valid=None, shape=(0, 16, 65))
    _grouped_call(shape=(B, 16, 0))
    assert ss.launches() == n
    assert C.sizeof(cx._CmvnStatsOpts) == 8 and C.sizeof(cx._CmvnGroupedOpts) == 12
