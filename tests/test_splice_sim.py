"""clx_splice_windows under the wave simulator (tests/wavesim/sim_splice.cpp runs the production kernel of clx_splice.hip and its
host side on the CPU): over the edge matrix of splice_cases.py the cells equal the float32 numpy restatement word for word in both
layouts, CT equals TC, and every cell lies within DESIGN.md 4.21's bound of the float64 reference; Splice.lfr is the index-level
restatement of FunASR's stacking; Splice.deltas is Kaldi's combined filters over the edge-repeated row, which differ from the
first-order filter applied twice in the two edge frames; every refusal has its text; and the Splice value checks its arguments.
The Kaldi and FunASR semantics are this project's reading, held by these restatements, not by a run of either toolkit."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_splice as sp
import splice_cases as sc


@pytest.mark.parametrize("layout", (sp.CT, sp.TC))
@pytest.mark.parametrize("name", sc.NAMES)
def test_the_simulator_is_the_restatement_word_for_word(name, layout):
    got, want = sc.simulated(name, layout), sc.restated(name)
    assert sc.same_words(got, want), (name, layout, int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))))


@pytest.mark.parametrize("name", sc.NAMES)
def test_ct_is_tc(name):
    assert sc.same_words(sc.simulated(name, sp.CT), sc.simulated(name, sp.TC))


def _coefs64(splice_name):
    """The exact coefficients a delta plan's float32 ones were rounded from; None: the plan's own float32 values are exact."""
    if splice_name in ("d1", "d2", "d4w4"):
        order, window = {"d1": (1, 2), "d2": (2, 2), "d4w4": (4, 4)}[splice_name]
        return [None] + sp.deltas64(order, window)
    return None


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_cell_is_within_the_derived_bound_of_float64(name):
    c = sc.case(name)
    x = sc.data(c)
    ref, allow = sp.reference(x, c["valid"], sc.plan(c), _coefs64(c["plan"]))
    got = sc.simulated(name, sp.CT).astype(np.float64)
    assert got.shape == ref.shape
    nan = np.isnan(ref)                                      # (only where a case plants NaN words under copy blocks)
    assert np.array_equal(nan, np.isnan(got)) and (not nan.any() or c["cells"])
    err = np.where(nan, 0.0, np.abs(got - ref))
    live = allow > 0
    print("%s: worst error %.3g, worst error / bound %.3g over %d computed cells of %d" % (
        name, err.max(initial=0.0), (err[live] / allow[live]).max(initial=0.0), int(live.sum()), err.size))
    assert np.all(err <= allow), (name, int(np.count_nonzero(err > allow)))


def test_padding_of_the_input_is_never_read_and_the_pad_is_the_word():
    """The input's padding is NaN in every case; a FIR cell that read one would be NaN.  Output frames from V_out on are the pad's word."""
    for name in sc.NAMES:
        c = sc.case(name)
        got, p = sc.simulated(name, sp.CT), sc.plan(c)
        for k, V in enumerate(c["valid"]):
            Vo = p.frames_out(V)
            assert np.all(got[k, :, Vo:].view(np.uint32) == np.float32(p.pad).view(np.uint32)), (name, k)
            if not c["cells"]:
                assert not np.isnan(got[k, :, :Vo]).any(), (name, k)


def test_a_copy_block_moves_words():
    c = sc.case("copy_words")
    x, got = sc.data(c), sc.simulated("copy_words", sp.TC)
    rows = c["rows"]
    for k, r, t, word in c["cells"]:
        for j, (off, _) in enumerate(sc.plan(c).blocks):      # block j of output frame t - off is input frame t
            u = t - off
            if 0 <= u < c["valid"][k]:
                assert got.view(np.uint32)[k, j * rows + r, u] == word == x.view(np.uint32)[k, r, t]
    assert got.view(np.uint32)[0, 0 * rows + 1, 0] == sc.NAN_A and got.view(np.uint32)[0, 4 * rows + 2, 29] == sc.NEG_ZERO   # the clamped edges too


def test_lfr_is_the_stacking_restated_index_by_index():
    for name in ("s6", "rows80_lfr", "lfr_Tout256", "lfr_Tout257"):
        c = sc.case(name)
        x, p = sc.data(c), sc.plan(c)
        got = sc.simulated(name, sp.TC)                       # [B, 7 * rows, T_out]
        for k, V in enumerate(c["valid"]):
            want = sp.apply_lfr(x[k, :, :V].T, 7, 6)          # [ceil(V / 6), 7 * rows]
            assert want.shape == (p.frames_out(V), 7 * c["rows"]) == (-(-V // 6), 7 * c["rows"])
            assert sc.same_words(np.ascontiguousarray(got[k, :, :want.shape[0]].T), want), (name, k)
    assert cx.Splice.lfr() == cx.Splice([(o, None) for o in range(-3, 4)], stride=6) and cx.Splice.lfr(5, 3).blocks[0] == (-2, None)
    assert [o for o, _ in cx.Splice.lfr(4, 2).blocks] == [-1, 0, 1, 2]


def _run(x, splice, valid=None):
    """x [B, rows, T] through the simulator in CT."""
    B, rows, T = x.shape
    out = np.empty((B, splice.n_out(rows), splice.frames_out(T)), dtype=np.float32)
    return sp.splice_windows(np.ascontiguousarray(x), out, [T] * B if valid is None else valid, sp.CT, splice)


def _padded_filter(row, c):
    """sum_d c[d] row[clamp(t + d)] by float32 fused steps in ascending d, over the edge-repeated row."""
    m = len(c) // 2
    padded = np.concatenate([np.repeat(row[:1], m), row, np.repeat(row[-1:], m)])
    acc = np.zeros(row.size, dtype=np.float32)
    for i in range(len(c)):
        acc = sp.sa.fma32(np.float32(c[i]), padded[i:i + row.size], acc)
    return acc


def test_deltas_are_kaldis_combined_filters_and_not_the_first_order_filter_twice():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 2, 11)).astype(np.float32)
    one, two = cx.Splice.deltas(1, 2), cx.Splice.deltas(2, 2)
    assert one.blocks == ((0, None), (0, tuple(float(np.float32(v / 10.0)) for v in (-2, -1, 0, 1, 2))))
    nine = np.convolve([-2, -1, 0, 1, 2], [-2, -1, 0, 1, 2])
    assert nine.tolist() == [4, 4, 1, -4, -10, -4, 1, 4, 4]
    assert two.blocks[:2] == one.blocks and two.blocks[2] == (0, tuple(float(np.float32(np.float64(v) / 100.0)) for v in nine))
    y1, y2 = _run(x, one), _run(x, two)
    for r in range(2):
        assert sc.same_words(y1[0, r], x[0, r]) and sc.same_words(y2[0, r], x[0, r])
        assert sc.same_words(y1[0, 2 + r], _padded_filter(x[0, r], one.blocks[1][1]))
        assert sc.same_words(y2[0, 2 + r], y1[0, 2 + r])
        assert sc.same_words(y2[0, 4 + r], _padded_filter(x[0, r], two.blocks[2][1]))
    # order 1 applied twice: the same cells up to rounding away from the edges, another answer in the two frames at either edge
    twice = _run(np.ascontiguousarray(y1[:, 2:4]), one)[:, 2:4]
    diff = np.abs(twice.astype(np.float64) - y2[:, 4:6])
    scale = np.abs(x).max()
    assert np.all(diff[..., 2:-2] <= 1e-5 * scale), diff
    assert np.all(diff[..., :2] > 1e-3 * scale) and np.all(diff[..., -2:] > 1e-3 * scale), diff
    # the C++ builder, in the simulator's host build and in the library, against whole numerators over whole denominators
    for order, window in ((0, 2), (1, 1), (1, 16), (2, 2), (3, 5), (4, 4), (2, 8)):
        blk, coefs = sp.deltas_tables(order, window)
        p = cx.Splice.deltas(order, window)
        assert blk[0].tolist() == [0, 0, 1, 0] and len(p.blocks) == order + 1 and p.blocks[0] == (0, None) and p.stride == 1
        for i, want in enumerate(sp.deltas64(order, window), start=1):
            off, m, copy, at = blk[i].tolist()
            assert (off, m, copy) == (0, i * window, 0)
            assert sc.same_words(coefs[at:at + 2 * m + 1], want.astype(np.float32))
            assert p.blocks[i] == (0, tuple(float(v) for v in want.astype(np.float32)))


def test_nothing_to_do_succeeds_and_touches_nothing():
    p = cx.Splice.lfr()
    x = np.zeros((0, 2, 9), dtype=np.float32)
    sp.splice_windows(x, np.zeros((0, 14, 2), dtype=np.float32), np.zeros(0, np.uint32), sp.CT, p)
    sp.splice_windows(None, None, None, sp.CT, p, shape=(0, 3, 5))
    sp.splice_windows(None, None, None, sp.TC, p, shape=(4, 3, 0))
    assert p.frames_out(0) == 0 and p.frames_out(1) == 1 and p.frames_out(6) == 1 and p.frames_out(7) == 2


def _blk(*rows):
    return np.array(rows, dtype=np.int32).reshape(-1, 4), np.ones(40, dtype=np.float32)


REFUSALS = [
    (dict(opts=False), "clx_splice_windows: null options"),
    (dict(reserved=1), "clx_splice_windows: reserved must be 0"),
    (dict(K=0), "clx_splice_windows: n_blocks must be 1..32"),
    (dict(K=33), "clx_splice_windows: n_blocks must be 1..32"),
    (dict(stride=0), "clx_splice_windows: stride must be 1..64"),
    (dict(stride=65), "clx_splice_windows: stride must be 1..64"),
    (dict(layout=7), "clx_splice_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
    (dict(rows=0), "clx_splice_windows: rows must be 1..256"),
    (dict(rows=257), "clx_splice_windows: rows must be 1..256"),
    (dict(T=1 << 31), "clx_splice_windows: T must be below 2^31"),
    (dict(blocks=False), "clx_splice_windows: null blocks"),
    (dict(raw=_blk((65, 0, 1, 0))), "clx_splice_windows: a block's offset must be -64..64"),
    (dict(raw=_blk((-65, 0, 1, 0))), "clx_splice_windows: a block's offset must be -64..64"),
    (dict(raw=_blk((0, 17, 0, 0))), "clx_splice_windows: a block's half-width must be 0..16"),
    (dict(raw=_blk((0, 0, 2, 0))), "clx_splice_windows: a block's copy mark must be 0 or 1"),
    (dict(raw=_blk((0, 1, 1, 0))), "clx_splice_windows: a copy block has half-width 0"),
    (dict(raw=_blk((0, 1, 0, 0)), coefs=False), "clx_splice_windows: null coefficients for a FIR block"),
    (dict(data=None), "clx_splice_windows: null argument"),
    (dict(out=None), "clx_splice_windows: null argument"),
    (dict(valid=None), "clx_splice_windows: null argument"),
    (dict(same=True), "clx_splice_windows: d_out must not be d_in"),
    (dict(valid=[3, 6]), "clx_splice_windows: valid[k] is larger than T"),
]


@pytest.mark.parametrize("change,text", REFUSALS)
def test_every_refusal_has_its_text_and_writes_nothing(change, text):
    a = dict(data=np.ones(2 * 3 * 5, dtype=np.float32), out=np.full(2 * 9 * 5, 7, dtype=np.float32), rows=3, T=5, valid=[5, 1], layout=sp.CT,
             opts=True, blocks=True, coefs=True, K=None, stride=None, reserved=0, raw=None, same=False)
    a.update(change)
    out = a["data"] if a["same"] else a["out"]
    before = None if out is None else out.copy()
    with pytest.raises(cx.ClaxonError) as e:
        sp.splice_windows(a["data"], out, a["valid"], a["layout"], cx.Splice.deltas(), shape=(2, a["rows"], a["T"]), opts=a["opts"],
                          blocks=a["blocks"], coefs=a["coefs"], K=a["K"], stride=a["stride"], reserved=a["reserved"], raw=a["raw"])
    assert str(e.value).endswith(text), (str(e.value), text)
    assert before is None or np.array_equal(before, out)
    assert len({t for _, t in REFUSALS}) == 16               # (a text of its own for every kind of refusal)
    # (K * rows above 8192 has no text of its own: 32 blocks of 256 rows are the most, and the case k32_rows256 runs them)
    assert cx.SPLICE_MAX_OUT_ROWS == 8192 == cx.SPLICE_MAX_BLOCKS * 256


def test_the_stated_sizes_are_the_sources():
    L = sp.lib()
    assert (L.sim_splice_tile(), L.sim_splice_threads(), L.sim_splice_stage_words()) == (sp.TILE, sp.THREADS, sp.STAGE_WORDS) == (256, 256, 8192)
    assert L.sim_splice_lds_bytes() == sp.LDS_BYTES == 8192 * 4 + 32 * 16 + 32 * 33 * 4
    assert "clx_splice_windows" in cx.EXPORTS and "clx_splice_deltas" in cx.EXPORTS
    assert (cx.SPLICE_MAX_BLOCKS, cx.SPLICE_MAX_STRIDE, cx.SPLICE_MAX_OFFSET, cx.SPLICE_MAX_HALF) == (32, 64, 64, 16)


def test_the_sub_tiles_are_the_ones_the_design_states():
    """(Fs, Rc) of the shapes DESIGN.md 4.21 names: deltas on 13 and 80 rows, LFR on 80 rows, and the two shapes that split."""
    def shape(rows, T, layout, p):
        x = np.zeros((1, rows, T) if layout == sp.CT else (1, T, rows), dtype=np.float32)
        o = np.zeros((1, p.n_out(rows), p.frames_out(T)) if layout == sp.CT else (1, p.frames_out(T), p.n_out(rows)), dtype=np.float32)
        sp.splice_windows(x, o, [T], layout, p)
        return sp.last_shape()
    d2, lfr = cx.Splice.deltas(), cx.Splice.lfr()
    assert shape(13, 8, sp.CT, d2) == (256, 13, 4) and shape(13, 8, sp.TC, d2) == (256, 13, 4)
    assert shape(80, 8, sp.CT, d2) == (256, 31, 4) and shape(80, 8, sp.TC, d2) == (94, 80, 4)
    assert shape(80, 8, sp.CT, lfr) == (256, 5, 3) and shape(80, 8, sp.TC, lfr) == (16, 80, 3)
    assert shape(2, 8, sp.CT, cx.Splice.subsample(64)) == (128, 1, 0) and shape(256, 8, sp.TC, sc.PLANS["m16"]) == (1, 248, 16)


def test_the_splice_value():
    S = cx.Splice
    a = S([(0, None), (1, [0.5, 0.25, 0.5])], stride=2, pad=1.5)
    assert a == S([(0, None), (1, (0.5, 0.25, 0.5))], 2, 1.5) and hash(a) == hash(S([(0, None), (1, [0.5, 0.25, 0.5])], 2, 1.5))
    assert a != S([(0, None), (1, [0.5, 0.25, 0.5])], 2) and a != S([(0, None), (1, [0.5, 0.25, 0.5])], 1, 1.5) and a != "a"
    assert a.n_out(13) == 26 and a.frames_out(5) == 3 and a.frames_out(np.array([0, 1, 2, 3])).tolist() == [0, 1, 1, 2]
    assert repr(a) == "Splice([(0, None), (1, [0.5, 0.25, 0.5])], stride=2, pad=1.5)" and eval(repr(a), {"Splice": S}) == a
    assert S.context(1, 2) == S([(-1, None), (0, None), (1, None), (2, None)]) and S.subsample(3) == S([(0, None)], 3)
    assert S.deltas(0).blocks == ((0, None),) and len({S.deltas(), S.deltas(2, 2), S.lfr()}) == 2
    blk, cf = a._tables()
    assert blk.tolist() == [[0, 0, 1, 0], [1, 1, 0, 0]] and cf.tolist() == [0.5, 0.25, 0.5]
    for bad in (lambda: S([]), lambda: S([(0, None)] * 33), lambda: S([(65, None)]), lambda: S([(0.5, None)]), lambda: S([(0, [1.0, 2.0])]),
                lambda: S([(0, [1.0] * 35)]), lambda: S([(0, [float("nan")])]), lambda: S([(0, [1e39])]), lambda: S([(0, None)], 0),
                lambda: S([(0, None)], 65), lambda: S([(0, None)], True), lambda: S([(0, None)], 1, float("inf")), lambda: S([(0, None, 1)]),
                lambda: S(7), lambda: S.deltas(5), lambda: S.deltas(2, 9), lambda: S.deltas(1, 0), lambda: S.deltas(-1), lambda: S.context(16, 16),
                lambda: S.context(-1, 0), lambda: S.subsample(0), lambda: S.subsample(65), lambda: S.lfr(33), lambda: S.lfr(7, 0)):
        with pytest.raises(ValueError, match="Splice"):
            bad()
