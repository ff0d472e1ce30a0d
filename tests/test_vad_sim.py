"""The energy VAD and the frame selection (clx_vad.hip, unmodified) under the wave simulator, on the CPU: over the cases of
vad_cases.py the production kernels equal the numpy restatements of claxon_hip.h word for word in both layouts, guards included
-- the mask, the thresholds, the counts and the selected batch; the `wide` thresholds are not a plain ascending sum's; every
threshold lies within DESIGN.md 4.23's bound of the exact reference and the decisions equal the exact reference's away from the
threshold; the context obeys its rule; padding and the other rows are never read; the selection leaves its source alone and
counts the mask's live bytes; every refusal has its own text and launches nothing; and the Vad value checks what it is given."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_vad as sv
import vad_cases as vc

LAYOUTS = (sv.CT, sv.TC)


# ---- the decision -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", vc.VAD_NAMES)
def test_the_decision_is_the_restatement_word_for_word_in_both_layouts(name):
    want_mask, want_thr = vc.restated_vad(name)
    c = vc.vad_case(name)
    for layout in LAYOUTS:
        mask, thr = vc.simulated_vad(name, layout)
        assert np.array_equal(mask, want_mask), (name, layout, int(np.count_nonzero(mask != want_mask)))
        assert vc.same_words(thr, want_thr), (name, layout, thr, want_thr)
    for k, V in enumerate(c["valid"]):                       # padding is 0, whatever the input held there
        assert not np.any(want_mask[k, V:])
    if c["c"] == 0 and c["kind"] in ("normal", "alternating", "runs"):                     # (a frame's own cell decides: both answers occur)
        live = np.concatenate([want_mask[k, :V] for k, V in enumerate(c["valid"])])
        assert 0 < np.count_nonzero(live) < live.size, (name, "the case decides nothing")


def test_the_plain_kinds_decide_what_their_names_say():
    for name in vc.ORDINARY_NAMES:
        c, (mask, _) = vc.vad_case(name), vc.restated_vad(name)
        for k, V in enumerate(c["valid"]):
            if c["kind"] == "all":
                assert np.all(mask[k, :V] == 1), name
            if c["kind"] == "none":
                assert not np.any(mask[k, :V]), name


def test_the_planted_cells_are_not_above():
    """A cell equal to thr is not above: with c = 0 the planted frames themselves would be 0; here the restatement and the kernel
    agree on every byte (the test above), and the thresholds are the planted values exactly."""
    for name, thr in (("planted", 5.5), ("planted_s", 8.0)):
        c = vc.vad_case(name)
        x = vc.vad_data(c)
        got = vc.simulated_vad(name, sv.CT)[1]
        for k, V in enumerate(c["valid"]):
            if V >= 2:
                assert got[k] == np.float32(thr), (name, k, got[k])
            if V >= 8:                                       # (every three pairs, or every third cell, holds a planted one)
                assert np.count_nonzero(x[k, c["row"], :V] == np.float32(thr)) > 0
        alone = sv.restate_vad(x, c["valid"], c["E"], c["s"], 0, 0.5, c["row"])[0]
        for k, V in enumerate(c["valid"]):
            e = x[k, c["row"], :V]
            assert not np.any(alone[k, :V][e == np.float32(thr)]) and np.all(alone[k, :V][e > np.float32(thr)] == 1)


@pytest.mark.parametrize("name", vc.WIDE_NAMES)
def test_the_wide_thresholds_show_the_order(name):
    """With cancelling pairs of magnitude 2^50 in the energy row the double sum rounds where the float32 threshold shows it: the same
    cells added in plain ascending order give other thresholds, so the word-for-word test above does hold the ORDER."""
    c = vc.vad_case(name)
    plain = sv.restate_vad(vc.vad_data(c), c["valid"], c["E"], c["s"], c["c"], c["p"], c["row"], plain=True)[1]
    want = vc.restated_vad(name)[1]
    differs = int(np.count_nonzero(plain.view(np.uint32) != want.view(np.uint32)))
    print("%s: %d of %d thresholds differ from the plain ascending sum's" % (name, differs, want.size))
    assert differs > 0


@pytest.mark.parametrize("name", vc.FINITE_NAMES)
def test_every_threshold_lies_within_the_bound_of_the_exact_reference(name):
    _, ref, bound, _ = vc.reference_vad(name)
    got = vc.simulated_vad(name, sv.CT)[1].astype(np.float64)
    err = np.abs(got - ref)
    print("%s: worst |thr - thr*| %.3g, bound there %.3g" % (name, float(err.max()), float(bound[int(err.argmax())])))
    assert np.all(err <= bound), (name, err, bound)


@pytest.mark.parametrize("name", vc.ORDINARY_NAMES)
def test_the_decisions_are_the_exact_references_away_from_the_threshold(name):
    """The ordinary cases are drawn so that the reference alone keeps the doubtful frames -- those whose context holds a cell within
    the bound of thr* -- to at most 0.1 % of the live frames; everywhere else the bytes must be equal."""
    c = vc.vad_case(name)
    want, _, _, doubt = vc.reference_vad(name)
    live = sum(c["valid"])
    assert np.count_nonzero(doubt) <= 0.001 * live, (name, int(np.count_nonzero(doubt)), live)
    got = vc.simulated_vad(name, sv.CT)[0]
    assert np.array_equal(got[~doubt], want[~doubt]), (name, int(np.count_nonzero(got[~doubt] != want[~doubt])))


@pytest.mark.parametrize("c", vc.CONTEXTS)
def test_the_window_rule(c):
    """Index only: the production rule (clx_vad::context) is the stated one, which has its invariants."""
    for V in [v for v in vc.valids(c, vc.T3) if v]:
        for t in range(V):
            lo, hi, den = sv.window_rule(t, V, c)
            assert (lo, hi) == sv.sim_context(t, V, c), (t, V, c)
            assert 0 <= lo <= t <= hi < V and den == hi - lo + 1, (t, V, c)
            if t >= c and t + c < V:
                assert den == 2 * c + 1, (t, V, c)
            else:
                assert den < 2 * c + 1, (t, V, c)


def test_the_decision_reads_neither_padding_nor_other_rows():
    """Signalling patterns in the padding and in the other rows: other words there change no byte and no threshold."""
    for name in ("c2_p0.12_s0.5", "c128_p0.5_s0.0", "rows560_last"):
        c = vc.vad_case(name)
        x = vc.vad_data(c)
        y = x.copy()
        other = np.ones(x.shape, dtype=bool)
        for k, V in enumerate(c["valid"]):
            other[k, c["row"], :V] = False
        assert np.all(x.view(np.uint32)[other] == vc.PAD_WORD)
        y.view(np.uint32)[other] = 0x7f800001                # a signalling NaN
        y[:, :, 1::2][other[:, :, 1::2]] = np.float32(1e30)
        for layout in LAYOUTS:
            mask, thr = sv.vad_windows(vc.as_layout(y, layout), c["valid"], layout, c["E"], c["s"], c["c"], c["p"], c["row"], shape=x.shape)
            want_mask, want_thr = vc.simulated_vad(name, layout)
            assert np.array_equal(mask, want_mask) and vc.same_words(thr, want_thr), (name, layout)


def test_no_sum_is_launched_without_a_mean_scale():
    c = vc.vad_case("c0_p0.12_s0.0")
    x = vc.vad_data(c)
    before = sv.launches()
    sv.vad_windows(x, c["valid"], sv.CT, c["E"], 0.0, c["c"], c["p"], c["row"])
    assert sv.launches() == before + 1 and sv.last_shape()[2] == 0 and sv.last_shape()[4] == 0
    sv.vad_windows(x, c["valid"], sv.CT, c["E"], 0.5, c["c"], c["p"], c["row"])
    assert sv.launches() == before + 3 and sv.last_shape()[:2] == (3, 1) and sv.last_shape()[4] == len(c["valid"])
    mask, thr = sv.vad_windows(x, c["valid"], sv.CT, c["E"], 0.0, c["c"], c["p"], c["row"], thresholds=False)   # (no thresholds asked for)
    assert thr is None and np.array_equal(mask, vc.simulated_vad("c0_p0.12_s0.0", sv.CT)[0])


# ---- the selection ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", vc.SELECT_NAMES)
def test_the_selection_is_the_restatement_word_for_word_in_both_layouts(name):
    want, want_counts = vc.restated_select(name)
    c = vc.select_case(name)
    x, mask = vc.select_data(c)
    for layout in LAYOUTS:
        got, counts = vc.simulated_select(name, layout)
        assert np.array_equal(counts, want_counts), (name, layout, counts, want_counts)
        assert vc.same_words(got, want), (name, layout, int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))))
    for k, V in enumerate(c["valid"]):                       # count is the mask's live popcount: the 0xff bytes from V on count nothing
        assert want_counts[k] == np.count_nonzero(mask[k, :V]) and np.all(mask[k, V:] == 0xff)
        assert np.all(want.view(np.uint32)[k, :, want_counts[k]:] == np.float32(c["pad"]).view(np.uint32))


def test_an_all_ones_mask_gives_the_live_frames_then_pad():
    for name in ("ones_rows1", "padding_counts_nothing"):
        c = vc.select_case(name)
        x, _ = vc.select_data(c)
        got, counts = vc.simulated_select(name, sv.TC)
        assert counts.tolist() == c["valid"]
        for k, V in enumerate(c["valid"]):
            assert vc.same_words(got[k, :, :V], x[k, :, :V]) and np.all(got[k, :, V:] == np.float32(c["pad"]))


def test_the_selection_without_counts_and_with_a_nan_pad():
    """counts == NULL changes nothing else; the pad is a word, any word."""
    c = vc.select_case("random_rows30")
    x, mask = vc.select_data(c)
    nan_pad = np.array([0x7fc00abc], dtype=np.uint32).view(np.float32)[0]
    out, counts = sv.select_windows(x, np.empty_like(x), c["valid"], mask, sv.CT, float(nan_pad), counts=False)
    assert counts is None
    want, want_counts = vc.restated_select("random_rows30")
    for k in range(x.shape[0]):
        n = int(want_counts[k])
        assert vc.same_words(out[k, :, :n], want[k, :, :n]) and np.all(np.isnan(out[k, :, n:]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def _refused(call, text):
    before = sv.launches()
    with pytest.raises(cx.ClaxonError) as e:
        call()
    assert text in str(e.value), (text, str(e.value))
    assert sv.launches() == before, text


def test_every_refusal_of_the_decision_has_its_own_text_and_launches_nothing():
    x = np.zeros((2, 3, 40), dtype=np.float32)
    v = [40, 7]
    ok = dict(E=5.0, s=0.5, c=2, p=0.5, row=0)
    texts = []

    def refuse(text, data=x, valid=v, layout=sv.CT, shape=None, **kw):
        _refused(lambda: sv.vad_windows(data, valid, layout, shape=shape, **{**ok, **kw}), text)
        texts.append(text)

    refuse("clx_vad_windows: null options", opts=False)
    refuse("clx_vad_windows: reserved must be 0", reserved=[0, 0, 1])
    refuse("clx_vad_windows: reserved must be 0", reserved=[7, 0, 0])
    refuse("clx_vad_windows: energy_threshold must be finite", E=float("inf"))
    refuse("clx_vad_windows: energy_threshold must be finite", E=float("nan"))
    refuse("clx_vad_windows: energy_mean_scale must be finite", s=float("-inf"))
    for p in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        refuse("clx_vad_windows: proportion_threshold must be above 0 and below 1", p=p)
    refuse("clx_vad_windows: frames_context must be 0..128", c=129)
    refuse("clx_vad_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT", layout=7, shape=(2, 3, 40))
    refuse("clx_vad_windows: rows must be 1..8192", shape=(2, 0, 40))
    refuse("clx_vad_windows: rows must be 1..8192", shape=(2, 8193, 40))
    refuse("clx_vad_windows: n_frames must be below 2^31", shape=(2, 3, 1 << 31))
    refuse("clx_vad_windows: row must be below rows", row=3)
    refuse("clx_vad_windows: null argument", data=None, shape=(2, 3, 40))
    refuse("clx_vad_windows: null argument", valid=None)
    refuse("clx_vad_windows: null argument", mask=False)
    refuse("clx_vad_windows: valid[k] is larger than n_frames", valid=[40, 41])
    assert len(set(texts)) == 12
    # nothing to do is fine, and launches nothing
    before = sv.launches()
    sv.vad_windows(np.zeros((0, 3, 40), dtype=np.float32), [], sv.CT, **ok)
    sv.vad_windows(np.zeros((2, 3, 0), dtype=np.float32), [0, 0], sv.CT, **ok)
    assert sv.launches() == before


def test_every_refusal_of_the_selection_has_its_own_text_and_launches_nothing():
    x = np.zeros((2, 3, 40), dtype=np.float32)
    out = np.empty_like(x)
    m = np.ones((2, 40), dtype=np.uint8)
    v = [40, 7]
    texts = []

    def refuse(text, data=x, dst=out, valid=v, mask=m, layout=sv.CT, shape=None, **kw):
        _refused(lambda: sv.select_windows(data, dst, valid, mask, layout, shape=shape, **kw), text)
        texts.append(text)

    refuse("clx_select_windows: null options", opts=False)
    refuse("clx_select_windows: reserved must be 0", reserved=[0, 2, 0])
    refuse("clx_select_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT", layout=2, shape=(2, 3, 40))
    refuse("clx_select_windows: rows must be 1..8192", shape=(2, 8193, 40))
    refuse("clx_select_windows: n_frames must be below 2^31", shape=(2, 3, 1 << 31))
    refuse("clx_select_windows: null argument", data=None, shape=(2, 3, 40))
    refuse("clx_select_windows: null argument", dst=None)
    refuse("clx_select_windows: null argument", valid=None)
    refuse("clx_select_windows: null argument", mask=None)
    refuse("clx_select_windows: valid[k] is larger than n_frames", valid=[41, 0])
    refuse("clx_select_windows: d_dst must not overlap d_src", dst=x)
    both = np.zeros(2 * x.size - 1, dtype=np.float32)        # dst starts inside src's last word but one
    refuse("clx_select_windows: d_dst must not overlap d_src", data=both[:x.size], dst=both[x.size - 1:], shape=(2, 3, 40))
    refuse("clx_select_windows: d_dst must not overlap d_src", data=both[x.size - 1:], dst=both[:x.size], shape=(2, 3, 40))
    assert len(set(texts)) == 8
    before = sv.launches()
    _, counts = sv.select_windows(np.zeros((2, 3, 0), dtype=np.float32), np.zeros((2, 3, 0), dtype=np.float32), [0, 0], np.zeros((2, 0), dtype=np.uint8), sv.CT)
    assert sv.launches() == before and counts.tolist() == [0, 0]
    touching = np.zeros(2 * x.size, dtype=np.float32)        # dst right behind src: no overlap
    sv.select_windows(touching[:x.size], touching[x.size:], v, m, sv.CT, shape=(2, 3, 40))
    assert sv.launches() == before + 3


# ---- the value type -----------------------------------------------------------------------------------------------------------------

def test_the_vad_value():
    v = cx.Vad()
    assert (v.energy_threshold, v.energy_mean_scale, v.frames_context, v.proportion_threshold, v.row, v.select, v.pad) == \
        (5.0, 0.5, 0, float(np.float32(0.6)), 0, True, 0.0)
    x = cx.Vad.voxceleb()
    assert (x.energy_threshold, x.energy_mean_scale, x.frames_context, x.proportion_threshold) == (5.5, 0.5, 2, float(np.float32(0.12)))
    assert x == cx.Vad(5.5, 0.5, 2, 0.12) and hash(x) == hash(cx.Vad(5.5, 0.5, 2, 0.12)) and x != v and x != cx.Vad.voxceleb(select=False)
    assert eval(repr(x), {"Vad": cx.Vad}) == x and repr(v).startswith("Vad(")
    assert len({v, cx.Vad(), x}) == 2
    for kw in (dict(energy_threshold=float("inf")), dict(energy_threshold="5"), dict(energy_mean_scale=float("nan")), dict(frames_context=129),
               dict(frames_context=-1), dict(frames_context=1.5), dict(frames_context=True), dict(proportion_threshold=0.0),
               dict(proportion_threshold=1.0), dict(proportion_threshold=float("nan")), dict(row=-1), dict(row=8192), dict(row=0.5),
               dict(select=2), dict(pad="0"), dict(energy_threshold=1e39)):
        with pytest.raises(ValueError, match="Vad: "):
            cx.Vad(**kw)
