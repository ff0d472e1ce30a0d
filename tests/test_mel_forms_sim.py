"""The case matrix of mel_form_cases.py under the wave simulator: what test_gpu_mel_forms.py holds the GPU to, word for word, is
itself held to the definition here.  clx_k_mel_c, clx_k_mel_f and clx_k_mel_q in power mode lie inside the derived bound of the
float64 reference (simlib_mel.reference on the host-padded batch, simlib_melk.reference, simlib_melq.reference_power) with the
dead frames the word 0, valid_frames the formula's and every word outside the output untouched; clx_k_mel_range over two and three
tiles equals float32 numpy on the unranged output at all four offsets from the 16-byte grid; in zero-pad mode no float from
valid[k] on is read; the energy row is the logarithm of the energy in the stated lane order.  The guards and the every-word-written
check are mel_form_cases._sim_call's."""
import numpy as np
import pytest

import mel_form_cases as mc
import simlib_mel as sm
from test_melc_sim import RANGES


@pytest.mark.parametrize("case,layout", **mc.with_layouts(mc.POWER_CASES))
def test_power_is_inside_the_float64_bound(case, layout):
    """Every centred, framed and cepstral case: valid_frames by the formula, dead frames the word 0, live cells within the bound.
    With the energy on, row 0 is not the cepstrum's: test_the_energy_row holds it."""
    got, vf = mc.sim(case, layout)
    assert np.array_equal(vf, mc.valid_frames(case)), (case, vf, mc.valid_frames(case))
    assert vf.min() == 0 and vf.max() == case.T
    worst, cells = mc.check_bound(got, case, (case, mc.LAYOUT_NAMES[layout]), first_row=1 if getattr(case, "energy", 0) else 0)
    print("%s %s: worst |error| / bound %.4f over %d live cells" % (case, mc.LAYOUT_NAMES[layout], worst, cells))


def test_the_layouts_give_the_same_words():
    """A cell's sum does not depend on the lane that computes it."""
    for case in mc.POWER_CASES:
        if len(case.layouts) == 2:
            mc.same_words(mc.sim(case, mc.CT)[0], mc.sim(case, mc.TC)[0], case, "the other layout")


@pytest.mark.parametrize("case", mc.TWO_PASS_400, ids=repr)
def test_the_cepstral_bound_is_narrow(case):
    """So that the power-mode cepstral bound cannot go vacuous: the median of dC / max(|C64|, tiny) over the live cells is below
    0.05 for the two 400-tap shapes (a condition on the reference alone)."""
    C64, dC = mc.reference(case)
    vf = mc.valid_frames(case)
    rel = np.concatenate([(dC[k, :vf[k]] / np.maximum(np.abs(C64[k, :vf[k]]), np.finfo(np.float64).tiny)).reshape(-1) for k in range(len(vf))])
    print("%s: median dC / |C64| %.4f over %d live cells" % (case, float(np.median(rel)), rel.size))
    assert np.median(rel) < 0.05


@pytest.mark.parametrize("ranged", RANGES, ids=lambda r: "D%g_%g_%g" % r)
@pytest.mark.parametrize("mode", (sm.LN, sm.LOG10), ids=("ln", "log10"))
@pytest.mark.parametrize("case", mc.RANGED, ids=repr)
def test_ranged_is_float32_numpy_on_the_unranged_output(case, mode, ranged):
    """Both (D, shift, scale), both layouts, the output 0, 1, 2 and 3 words behind a 16-byte boundary: the words of float32
    maximum(y, max_k - D), + shift, * scale on the simulator's unranged output with the dead frames set to finish(0); wmax is that
    maximum.  The launches have two or three tiles per window (the frame-boundary case: one)."""
    assert case.boundaries or ((case.n_mels * case.T + 6) // 4 + 1023) // 1024 >= 2
    u, vf = mc.sim_unranged(case, mode)
    assert np.array_equal(vf, mc.valid_frames(case, mc.batch(case)[1]))
    y0 = sm.finish(mode, mc.FLOOR, [0.0])[0]
    assert np.all(u[-1].view(np.uint32) == y0.view(np.uint32)), "a computed frame of zeros is not the silence value"
    for k in range(u.shape[0]):
        assert np.all(u[k, vf[k]:].view(np.uint32) == 0)
    if not case.boundaries:
        assert vf[0] == case.T and 0 < vf[2] < case.T and vf[3] == 0 and vf[4] == case.T
        v = u.copy()
        v[3] = y0
        assert np.argmax(v[0].max(axis=1)) >= 32 * ((case.T - 1) // 32) and np.argmax(v[1].max(axis=1)) < 32
    want, mx = mc.ranged_want(u, vf, y0, ranged)
    for layout, offset, got, vf_lib, wmax in mc.sim_ranged(case, mode, ranged):
        what = (case, mode, ranged, mc.LAYOUT_NAMES[layout], offset)
        assert np.array_equal(vf_lib, vf) and np.array_equal(wmax.view(np.uint32), mx.view(np.uint32)), (what, wmax, mx)
        mc.same_words(got, want, what, "float32 numpy")


@pytest.mark.parametrize("case", mc.ZERO_PAD_CASES, ids=repr)
def test_zero_pad_mode_reads_nothing_from_valid_on(case):
    """The floats from valid[k] on are NaN: the words of the batch with zeros there, so none of them is loaded."""
    layout = mc.TC
    mc.same_words(mc.sim(case, layout, nan_tail=True)[0], mc.sim(case, layout)[0], case, "the zero-tailed batch")


@pytest.mark.parametrize("case,layout", **mc.with_layouts(mc.ENERGY_CASES))
def test_the_energy_row(case, layout):
    """Power mode with a lifter: row 0 within LOG_ULPS of log_energy64(energy32(..)) in the live frames and the word 0 in the dead
    ones, rows 1.. the words of the same spec without energy."""
    got, vf = mc.sim(case, layout)
    rest = mc.sim(mc.without_energy(case), layout)[0]
    mc.same_words(got[:, :, 1:], rest[:, :, 1:], (case, "rows 1.."), "the spec without energy")
    for k in range(got.shape[0]):
        assert np.all(got[k, vf[k]:, 0].view(np.uint32) == 0)
    ulps = mc.energy_ulps(got, case)
    print("%s %s: worst energy error %.3f ulp over %d frames" % (case, mc.LAYOUT_NAMES[layout], float(ulps.max()), ulps.size))
    assert ulps.size and np.all(ulps <= sm.LOG_ULPS), float(ulps.max())
