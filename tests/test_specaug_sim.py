"""clx_specaug_windows under the wave simulator (tests/wavesim/sim_specaug.cpp runs the production kernels of clx_specaug.hip and
clx_norm.hip's sum kernels on host buffers): over the edge matrix of specaug_cases.py the simulator equals the numpy restatement
of claxon_hip.h's definition bit for bit -- cells and fills, in both layouts, which are therefore bit-equal to each other --, lies
inside the float64 reference's interval and inside the interval around torch's bicubic interpolate, leaves the guard
bands, the padding and the input alone; every refusal has its text; and the policy (SpecAugment, SpecAugmentPlan, augment=) draws
and refuses what it says."""
import numpy as np
import pytest
import torch  # noqa: F401  (the outside check needs it; the package does too)

import claxon_amd as cx
import simlib_specaug as ss
import specaug_cases as sc


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_simulator_is_the_restatement_word_for_word(name):
    c = sc.case(name)
    x = sc.data(c)
    want, wfills = ss.restate(x, c["valid"], c["warp"], c["fm"], c["tm"], c["fill"])
    for layout in (ss.CT, ss.TC):
        got, fills = sc.simulated(name, layout)
        assert sc.same_words(got, want), (name, layout, "cells", int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))))
        assert sc.same_words(fills, wfills), (name, layout, "fills")
    assert sc.same_words(sc.simulated(name, ss.CT)[0], sc.simulated(name, ss.TC)[0])
    for k, n in enumerate(c["valid"]):                       # (padding comes back as the words it held)
        assert np.all(want[k, :, n:].view(np.uint32) == sc.PAD_WORD)


@pytest.mark.parametrize("name", [c["name"] for c in sc.MATRIX if c["finite"] and c["warp"] is not None])
def test_the_simulator_lies_inside_the_reference_interval(name):
    c = sc.case(name)
    x = sc.data(c)
    ref, allow = ss.reference(np.where(np.isfinite(x), x, 0), c["valid"], c["warp"])
    got = sc.simulated(name, ss.CT)[0].astype(np.float64)
    worst = 0.0
    for k, V in enumerate(c["valid"]):
        free = ~ss.masked(V, c["rows"], None if c["fm"] is None else c["fm"][k], None if c["tm"] is None else c["tm"][k])
        err, a = np.abs(got[k, :, :V] - ref[k, :, :V])[free], allow[k, :, :V][free]
        assert np.all(err <= a), (name, k, float(np.max(err / np.maximum(a, 1e-300))))
        worst = max(worst, float(np.max(err / np.maximum(a, 1e-300), initial=0.0)))
    print("%s: worst error / allowance %.3g" % (name, worst))


def test_unmasked_warps_against_torch_bicubic():
    """The outside check: torch.nn.functional.interpolate(mode="bicubic", align_corners=False) on the CPU, applied to the two
    segments.  torch's coordinate goes through a float32 scale, so this is an interval, not equality."""
    rng = np.random.default_rng(20)
    rows, T = 80, 300
    valid = [300, 257, 45, 120, 3, 82]
    warp = np.array([(150, 190), (200, 120), (37, 8), (1, 119), (1, 2), (41, 40)])
    x = rng.standard_normal((len(valid), rows, T)).astype(np.float32)
    got = ss.specaug_windows(x, np.empty_like(x), valid, ss.CT, warp, fill=0.0).astype(np.float64)
    want, allow = ss.torch_warp(x, valid, warp)
    worst = 0.0
    for k, V in enumerate(valid):
        err = np.abs(got[k, :, :V] - want[k, :, :V])
        ratio = err / allow[k, :, :V].clip(1e-300)
        worst = max(worst, float(ratio.max()))
        print("window %d, V %d, warp %s: worst difference %.3g, worst difference / allowance %.3g" % (k, V, tuple(warp[k]), err.max(), ratio.max()))
        assert np.all(err <= allow[k, :, :V]), (k, float(ratio.max()))
    print("largest observed ratio to the bound: %.3g" % worst)


def test_a_nan_under_a_mask_does_not_leak_and_one_beside_a_warped_cell_leaks_where_the_taps_say():
    c = sc.case("nan_masked")
    got = sc.simulated("nan_masked", ss.CT)[0]
    assert not np.any(np.isnan(got[0])) and np.all(got[0, 1] == np.float32(0.25))
    at = np.argwhere(np.isnan(got[1]))
    V, (cc, w) = c["valid"][1], c["warp"][1]
    hit = set()
    for b, I, ob, O in ss.segments(V, int(cc), int(w)):
        ix, _, _ = ss.coordinates(I, O)
        for q in range(4):
            hit |= set((ob + np.nonzero(b + np.clip(ix - 1 + q, 0, I - 1) == 25)[0]).tolist())
    assert 1 <= len(hit) <= 8 and set(map(tuple, at.tolist())) == {(1, t) for t in hit}


def test_copies_are_words():
    for name in ("copy_words", "identity"):
        c = sc.case(name)
        x, got = sc.data(c), sc.simulated(name, ss.TC)[0]
        for k, V in enumerate(c["valid"]):
            free = ~ss.masked(V, c["rows"], None if c["fm"] is None else c["fm"][k], None if c["tm"] is None else c["tm"][k])
            assert np.array_equal(got[k, :, :V].view(np.uint32)[free], x[k, :, :V].view(np.uint32)[free]), (name, k)
    assert sc.same_words(sc.simulated("identity", ss.CT)[0], sc.data(sc.case("identity")))


def test_a_fully_masked_window_is_its_mean():
    c = sc.case("mean_all_masked")
    x = sc.data(c)
    got, fills = sc.simulated("mean_all_masked", ss.CT)
    for k in (0, 1):
        V = c["valid"][k]
        assert np.all(got[k, :, :V] == fills[k]) and abs(float(fills[k]) - float(x[k, :, :V].astype(np.float64).mean())) < 1e-5
    assert fills[2] == 0 and not np.signbit(fills[2])


def test_nothing_to_do_succeeds_and_touches_nothing():
    x = np.zeros((0, 2, 9), dtype=np.float32)
    ss.specaug_windows(x, x.copy(), np.zeros(0, np.uint32), ss.CT)
    ss.specaug_windows(None, None, None, ss.CT, shape=(0, 3, 5))
    ss.specaug_windows(None, None, None, ss.TC, shape=(4, 3, 0))


REFUSALS = [
    (dict(opts=False), "clx_specaug_windows: null options"),
    (dict(reserved=1), "clx_specaug_windows: reserved must be 0"),
    (dict(fill_mean=2), "clx_specaug_windows: fill_mean must be 0 or 1"),
    (dict(fill=float("inf")), "clx_specaug_windows: fill must be finite"),
    (dict(fill=float("nan")), "clx_specaug_windows: fill must be finite"),
    (dict(F=33), "clx_specaug_windows: more than 32 frequency masks"),
    (dict(M=33), "clx_specaug_windows: more than 32 time masks"),
    (dict(layout=7), "clx_specaug_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"),
    (dict(rows=0), "clx_specaug_windows: rows must be 1..256"),
    (dict(rows=257), "clx_specaug_windows: rows must be 1..256"),
    (dict(T=1 << 31), "clx_specaug_windows: T must be below 2^31"),
    (dict(data=None), "clx_specaug_windows: null argument"),
    (dict(out=None), "clx_specaug_windows: null argument"),
    (dict(valid=None), "clx_specaug_windows: null argument"),
    (dict(same=True), "clx_specaug_windows: d_out must not be d_in"),
    (dict(valid=[3, 6]), "clx_specaug_windows: valid[k] is larger than T"),
    (dict(warp=[(0, 1), (0, 0)]), "clx_specaug_windows: warp[k] must be (0, 0) or have c and w within 1 .. valid[k] - 1"),
    (dict(warp=[(1, 0), (0, 0)]), "clx_specaug_windows: warp[k] must be (0, 0) or have c and w within 1 .. valid[k] - 1"),
    (dict(warp=[(5, 1), (0, 0)]), "clx_specaug_windows: warp[k] must be (0, 0) or have c and w within 1 .. valid[k] - 1"),
    (dict(warp=[(1, 5), (0, 0)]), "clx_specaug_windows: warp[k] must be (0, 0) or have c and w within 1 .. valid[k] - 1"),
    (dict(warp=[(0, 0), (1, 1)]), "clx_specaug_windows: warp[k] must be (0, 0) or have c and w within 1 .. valid[k] - 1"),
]


@pytest.mark.parametrize("change,text", REFUSALS)
def test_every_refusal_has_its_text_and_writes_nothing(change, text):
    a = dict(data=np.ones(2 * 3 * 5, dtype=np.float32), out=np.full(2 * 3 * 5, 7, dtype=np.float32), rows=3, T=5, valid=[5, 1], layout=ss.CT,
             warp=None, fill=0.0, opts=True, F=None, M=None, reserved=0, fill_mean=None, same=False)
    a.update(change)
    out = a["data"] if a["same"] else a["out"]
    before = None if out is None else out.copy()
    with pytest.raises(cx.ClaxonError) as e:
        ss.specaug_windows(a["data"], out, a["valid"], a["layout"], a["warp"], fill=a["fill"], shape=(2, a["rows"], a["T"]), opts=a["opts"],
                           F=a["F"], M=a["M"], reserved=a["reserved"], fill_mean=a["fill_mean"])
    assert str(e.value).endswith(text) or text in str(e.value)
    assert before is None or np.array_equal(before, out)
    assert len({t for _, t in REFUSALS}) == 13               # (a text of its own for every kind of refusal)


def test_the_stated_sizes_are_the_sources():
    L = ss.lib()
    assert (L.sim_specaug_tile(), L.sim_specaug_threads(), L.sim_specaug_max_rows(), L.sim_specaug_max_masks()) == \
        (ss.TILE, ss.THREADS, ss.MAX_ROWS, ss.MAX_MASKS) == (256, 256, 256, 32)
    assert L.sim_specaug_max_t() == (1 << 31) - 1 and L.sim_specaug_lds_bytes() == ss.LDS_BYTES == 9248
    assert "clx_specaug_windows" in cx.EXPORTS and cx.SPECAUG_MAX_MASKS == 32


# ---- the policy ---------------------------------------------------------------------------------------------------------------------

VF = [0, 1, 2, 3, 161, 162, 163, 500, 3000, 1000]


def test_the_same_seed_gives_the_same_plan_and_another_seed_another():
    a, b, c = (cx.SpecAugment(seed=s).draw(VF, 80) for s in (7, 7, 8))
    assert a == b and a != c and len(a) == len(VF)
    assert a.warp.shape == (len(VF), 2) and a.freq_masks.shape == (len(VF), 2, 2) and a.time_masks.shape == (len(VF), 10, 2) and a.fill == "mean"
    pol = cx.SpecAugment(seed=7)
    assert pol.draw(VF, 80) == a and pol.draw(VF, 80) != a   # (a policy goes on drawing: the second batch is another one)
    # a window's draws do not depend on the windows in front of it being short or long
    assert np.array_equal(cx.SpecAugment(seed=7).draw([5] * 8 + [3000], 80).warp[8], cx.SpecAugment(seed=7).draw([900] * 8 + [3000], 80).warp[8])


def test_p_0_is_an_all_identity_plan_and_p_1_skips_nothing():
    p = cx.SpecAugment(p=0, seed=1).draw(VF, 80)
    assert not p.warp.any() and not p.freq_masks[..., 1].any() and not p.time_masks[..., 1].any()
    q = cx.SpecAugment(p=1, seed=1).draw([3000] * 6, 80)
    assert np.all(q.warp > 0) and q.freq_masks[..., 1].any() and q.time_masks[..., 1].any()


@pytest.mark.parametrize("rows", (1, 3, 80, 256))
@pytest.mark.parametrize("kw", [dict(), dict(time_warp=1, time_width=5000, max_time_fraction=1.0, freq_width=300, freq_masks=32, time_masks=32),
                                dict(time_warp=0, max_time_fraction=0.0), dict(time_warp=5, fill=0.0, time_masks=0, freq_masks=0)])
def test_the_plans_stay_inside_the_stated_ranges(kw, rows):
    pol = cx.SpecAugment(p=1.0, seed=3, **kw)
    W = pol.time_warp
    for _ in range(20):
        plan = pol.draw(VF, rows)
        for k, V in enumerate(VF):
            c, w = plan.warp[k]
            if W == 0 or V < 2 * W + 2:
                assert (c, w) == (0, 0)
            else:
                assert W + 1 <= c <= V - W - 1 and abs(int(w) - int(c)) <= W and 1 <= w <= V - 1
            for first, width in plan.freq_masks[k]:
                assert 0 <= width <= min(pol.freq_width, rows) and 0 <= first and first + width <= rows
            for first, width in plan.time_masks[k]:
                assert 0 <= width <= min(pol.time_width, V) and 0 <= first and first + width <= V
            assert plan.time_masks[k][:, 1].sum() <= int(pol.max_time_fraction * V)          # the cap on the masked frames
            assert ss.masked(V, 1, None, plan.time_masks[k]).sum() <= pol.max_time_fraction * V
    if rows == 1:                                            # what a plan says is what the library accepts
        x = np.zeros((len(VF), 1, 3000), dtype=np.float32)
        ss.specaug_windows(x, np.empty_like(x), VF, ss.CT, plan.warp, plan.freq_masks if plan.freq_masks.size else None,
                           plan.time_masks if plan.time_masks.size else None, fill=0.0)


@pytest.mark.parametrize("rows", (1, 3, 80, 256))
def test_every_drawn_plan_passes_the_fit_check_of_read_mel(rows):
    """read_mel(augment=policy) holds the drawn plan to the same check as a plan given by hand: no seed may draw one that it refuses
    (a mask of width 0 may start at `rows` or at V: it masks nothing)."""
    zero_at_the_end = 0
    for kw in (dict(), dict(p=1.0), dict(p=1.0, time_warp=1, freq_masks=32, time_masks=32, freq_width=300, time_width=5000, max_time_fraction=1.0),
               dict(p=1.0, freq_width=0, time_width=0), dict(p=1.0, max_time_fraction=0.0)):
        for seed in range(100):
            plan = cx.SpecAugment(seed=seed, **kw).draw(VF, rows)
            cx._specaug_fit(plan, VF, rows, max(VF), "read_mel")
            zero_at_the_end += int(np.count_nonzero(plan.freq_masks[..., 0] == rows))
    vf32 = [3000] * 32
    for seed in range(300):                                  # the default policy on a loader's batch
        cx._specaug_fit(cx.SpecAugment(seed=seed).draw(vf32, 80), vf32, 80, 3000, "read_mel")
    assert zero_at_the_end > 0                               # (the case is met: a width-0 mask that starts at `rows`)


def test_the_fit_check_refuses_what_does_not_fit_and_clips_what_runs_over():
    z = np.zeros((2, 1, 2), dtype=np.int64)
    P = cx.SpecAugmentPlan
    ok = [P(np.zeros((2, 2)), z + [[80, 0]], z + [[24, 0]]), P(np.zeros((2, 2)), z + [[500, 0]], z + [[500, 0]]),
          P(np.zeros((2, 2)), z + [[79, 1 << 31]], z + [[23, 900]]), P([(1, 9), (0, 0)], z, z), P(np.zeros((0, 2)), np.zeros((0, 1, 2)), np.zeros((0, 1, 2)))]
    for plan in ok:
        cx._specaug_fit(plan, [10, 0][:len(plan)], 80, 24, "read_mel")
    bad = [(P(np.zeros((3, 2)), np.zeros((3, 1, 2)), np.zeros((3, 1, 2))), "a plan of 3 windows for a batch of 2"),
           (P(np.zeros((2, 2)), z + [[80, 1]], z), "a frequency mask of augment starts behind the batch's 80 rows"),
           (P(np.zeros((2, 2)), z, z + [[24, 1]]), "a time mask of augment starts behind the batch's 24 frames"),
           (P([(10, 1), (0, 0)], z, z), "a warp of augment"), (P([(0, 1), (0, 0)], z, z), "a warp of augment"), (P([(0, 0), (1, 1)], z, z), "a warp of augment")]
    for plan, text in bad:
        with pytest.raises(ValueError, match=text):
            cx._specaug_fit(plan, [10, 0], 80, 24, "read_mel")


@pytest.mark.parametrize("kw", [dict(time_warp=-1), dict(time_warp=1.5), dict(freq_masks=33), dict(time_masks=33), dict(time_masks=True), dict(freq_width=-1),
                                dict(time_width=None), dict(max_time_fraction=1.5), dict(max_time_fraction=-0.1), dict(p=2), dict(p=float("nan")),
                                dict(fill="median"), dict(fill=float("inf")), dict(fill=None)])
def test_the_policy_refuses(kw):
    with pytest.raises(ValueError):
        cx.SpecAugment(**kw)


def test_draw_and_the_plan_refuse():
    pol = cx.SpecAugment(seed=0)
    for bad in (dict(valid_frames=[-1], rows=80), dict(valid_frames=[1.5], rows=80), dict(valid_frames=[5], rows=0), dict(valid_frames=[5], rows=257)):
        with pytest.raises(ValueError):
            pol.draw(**bad)
    with pytest.raises(ValueError):
        cx.SpecAugmentPlan([(0, 0)], np.zeros((1, 33, 2)), np.zeros((1, 0, 2)))
    with pytest.raises(ValueError):
        cx.SpecAugmentPlan([(0, -1)], np.zeros((1, 0, 2)), np.zeros((1, 0, 2)))
    with pytest.raises(ValueError):
        cx.SpecAugmentPlan([(0, 0)], np.zeros((1, 0, 2)), np.zeros((1, 0, 2)), fill="max")
    assert len(cx.SpecAugmentPlan(np.zeros((0, 2)), np.zeros((0, 2, 2)), np.zeros((0, 10, 2)))) == 0


@pytest.mark.parametrize("bad", ["specaug", True, 1, dict(p=1.0), (0, 0)])
def test_read_mel_refuses_an_augment_that_is_neither_a_policy_nor_a_plan(bad):
    """(The refusal comes before anything else is looked at: no device, no stream set's state.)"""
    s = cx.StreamSet.__new__(cx.StreamSet)
    with pytest.raises(ValueError, match="augment must be a SpecAugment"):
        s.read_mel([0], [0], 4, None, augment=bad)


def test_read_has_no_augment_argument():
    import inspect
    assert "augment" not in inspect.signature(cx.StreamSet.read).parameters and "augment" in inspect.signature(cx.StreamSet.read_mel).parameters


@pytest.mark.parametrize("kw", [dict(warp=[(0, 0, 0)]), dict(warp=[(-1, 0)]), dict(freq_masks=np.zeros((1, 33, 2), dtype=np.int64)),
                                dict(time_masks=np.zeros((2, 1, 2), dtype=np.int64)), dict(time_masks=[[(0.5, 1)]]), dict(fill="zero"),
                                dict(fill=float("nan")), dict(valid=[1, 2])])
def test_specaug_windows_refuses_before_anything_touches_a_device(kw):
    c = cx.Context.__new__(cx.Context)
    a = dict(valid=[5])
    a.update(kw)
    with pytest.raises(ValueError):
        c.specaug_windows((64, 1, 3, 5), a.pop("valid"), cx.WINDOW_CT, out=128, **a)
