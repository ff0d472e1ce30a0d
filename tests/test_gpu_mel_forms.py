"""The newer mel kernels on the GPU against the wave simulator, word for word, over the case matrix of mel_form_cases.py: clx_k_mel_c
(centred), clx_k_mel_f (framed) and clx_k_mel_q (cepstral) in power mode write the same 32-bit words as the same source built by
g++ and run on host arrays (simlib_melc, simlib_melk, simlib_melq) -- every sum is a chain of explicit fmaf in a fixed order and
every conditioning step is rounded once, so a difference is a miscompile, a race the simulator's fixed schedule hides, a table that
differs between the two host compilers, or a contraction.  The float64 definition under its derived bound stays beside the equality
(test_mel_forms_sim.py holds the simulator to it as well).  The log modes of the multi-pass cases are held to LOG_ULPS of the
float64 log of the same call's power words; clx_k_mel_range over two and three tiles to float32 numpy on the GPU's own unranged
output at all four offsets from the 16-byte grid; zero-pad mode to reading nothing from valid[k] on; the energy row to the logarithm
of the energy in the stated lane order.

Every output is a guarded slice (gpu_guarded.py) that starts off the 16-byte grid: the guards stay and every word is written."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import mel_form_cases as mc
import simlib_mel as sm
from gpu_guarded import DEV, device_out, written
from test_melc_sim import RANGES

pytestmark = pytest.mark.gpu
MODE_NAMES = {sm.POWER: "power", sm.LN: "ln", sm.LOG10: "log10"}


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _same_table(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)))


def _spec(ctx, case, mode, ranged=None):
    """The case's spec on the device; its tables are, word for word, the arrays the simulator gets."""
    t = mc.tables(case)
    if case.form in ("centred", "ranged"):
        kw = dict(top=ranged[0], shift=ranged[1], scale=ranged[2]) if ranged is not None else {}
        spec = cx.MelSpec(ctx, mc.SR, n_fft=case.N, hop=case.H, n_mels=case.n_mels, mode=MODE_NAMES[mode], floor=mc.FLOOR, center=bool(case.center),
                          pad_mode=mc.PADS[case.pad], **kw)
    else:
        kw = {}
        if case.form == "cepstral":
            kw = dict(dct=t[2], lifter=t[3], energy=bool(case.energy), energy_scale=mc.ENERGY_SCALE if case.energy else 1.0)
        spec = cx.MelSpec.framed(ctx, case.rate, case.N, case.Nw, case.H, t[0], t[1], mode=MODE_NAMES[mode], floor=mc.FLOOR, remove_dc=bool(case.dc),
                                 preemph=case.c, whole_frames=bool(case.whole), **kw)
        assert np.float32(spec.preemph) == np.float32(case.c)
    assert _same_table(spec.window, t[0]) and _same_table(spec.fbank, t[1]), (case, "the spec's window or filterbank is not the simulator's")
    if case.form == "cepstral":
        assert _same_table(spec.dct, t[2]) and _same_table(spec.lifter, t[3]), (case, "the spec's dct or lifter is not the simulator's")
    assert spec.n_out == case.rows and spec.valid_frames(mc.batch(case)[1], case.T).tolist() == mc.valid_frames(case, mc.batch(case)[1]).tolist()
    return spec


def _gpu(ctx, spec, case, audio, layout, offset=1):
    """One call on the GPU; the output as [B, T, rows] float32 after the guard and fill checks."""
    B, rows, T = audio.shape[0], case.rows, case.T
    n = B * rows * T
    flat, out = device_out(n, offset_words=offset)
    shape = (B, rows, T) if layout == mc.CT else (B, T, rows)
    dev = torch.from_numpy(np.array(audio)).to(DEV)                # (a copy: the shared batch is read-only)
    torch.cuda.synchronize()                                 # (the fill first: on torch's default stream the launch goes to the context's own)
    ctx.mel_windows(spec, dev, mc.batch(case)[1], T, layout, out.view(shape))
    torch.cuda.synchronize()
    got = written(flat, n, (case, mc.LAYOUT_NAMES[layout], offset), offset_words=offset).view(np.float32).reshape(shape)
    return np.ascontiguousarray(got.transpose(0, 2, 1)) if layout == mc.CT else got


def _power(ctx, case, layout):
    spec = _spec(ctx, case, sm.POWER)
    try:
        return _gpu(ctx, spec, case, mc.batch(case)[0], layout)
    finally:
        spec.close()


@pytest.mark.parametrize("case,layout", **mc.with_layouts(mc.CENTRED))
def test_centred_power_is_the_simulators_word_for_word(ctx, case, layout):
    _check_power(ctx, case, layout)


@pytest.mark.parametrize("case,layout", **mc.with_layouts(mc.FRAMED))
def test_framed_power_is_the_simulators_word_for_word(ctx, case, layout):
    _check_power(ctx, case, layout)


@pytest.mark.parametrize("case,layout", **mc.with_layouts(mc.CEPSTRAL))
def test_cepstral_power_is_the_simulators_word_for_word(ctx, case, layout):
    """With the energy on, rows 1.. are the simulator's words and inside the bound; row 0 is within LOG_ULPS of the logarithm of the
    energy emulated in the stated lane order, and the word 0 in a dead frame."""
    _check_power(ctx, case, layout)


def _check_power(ctx, case, layout):
    what = (case, mc.LAYOUT_NAMES[layout])
    got = _power(ctx, case, layout)
    want, vf = mc.sim(case, layout)
    first = 1 if getattr(case, "energy", 0) else 0
    cells = mc.same_words(got[:, :, first:], want[:, :, first:], what)
    worst, live = mc.check_bound(got, case, what, first_row=first)
    print("%s %s: worst |error| / bound %.4f over %d live cells; %d cells word for word, 0 differ" % (case, mc.LAYOUT_NAMES[layout], worst, live, cells))
    if first:
        for k in range(got.shape[0]):
            assert np.all(got[k, vf[k]:, 0].view(np.uint32) == 0), (what, k)
        ulps = mc.energy_ulps(got, case)
        print("%s %s: worst energy error %.3f ulp over %d frames" % (case, mc.LAYOUT_NAMES[layout], float(ulps.max()), ulps.size))
        assert ulps.size and np.all(ulps <= sm.LOG_ULPS), (what, float(ulps.max()))


@pytest.mark.parametrize("case", mc.LOG_CASES, ids=repr)
def test_log_modes_within_log_ulps(ctx, case):
    """ln and log10 of the multi-pass centred and framed cases in the [B, n_frames, n_mels] layout against float64
    log(max(float64(M), floor)), M the power words of the same call shape (the modes share M bitwise; that M is the simulator's)."""
    vf = mc.valid_frames(case)
    power = _power(ctx, case, mc.TC)
    mc.same_words(power, mc.sim(case, mc.TC)[0], (case, "power"))
    for mode in (sm.LN, sm.LOG10):
        spec = _spec(ctx, case, mode)
        got = _gpu(ctx, spec, case, mc.batch(case)[0], mc.TC)
        spec.close()
        for k in range(len(vf)):
            assert np.all(got[k, vf[k]:].view(np.uint32) == 0), (case, MODE_NAMES[mode], k, "a frame past valid_frames is not the word 0")
        ulps = np.concatenate([sm.log_ulps(got[k, :vf[k]], power[k, :vf[k]], mode, mc.FLOOR).reshape(-1) for k in range(len(vf))])
        print("%s %s: worst error %.3f ulp over %d cells" % (case, MODE_NAMES[mode], float(ulps.max()), ulps.size))
        assert np.all(ulps <= sm.LOG_ULPS), (case, MODE_NAMES[mode], float(ulps.max()))


@pytest.mark.parametrize("mode", (sm.LN, sm.LOG10), ids=("ln", "log10"))
@pytest.mark.parametrize("case", mc.RANGED, ids=repr)
def test_ranged_is_float32_numpy_on_the_unranged_output(ctx, case, mode):
    """Both (D, shift, scale), both layouts, the output 0, 1, 2 and 3 words behind a 16-byte boundary: the words of float32
    maximum(y, max_k - D), + shift, * scale on the GPU's own unranged output with the dead frames set to the device's finish(0),
    read from the window of zeros that is live to its end.  The range launches have two or three tiles per window (the frame-boundary
    case: one)."""
    a, valid = mc.batch(case)
    vf = mc.valid_frames(case, valid)
    plain = _spec(ctx, case, mode)
    unranged = {layout: _gpu(ctx, plain, case, a, layout) for layout in mc.LAYOUTS}
    plain.close()
    cells = 0
    for ranged in RANGES:
        spec = _spec(ctx, case, mode, ranged)
        for layout in mc.LAYOUTS:
            u = unranged[layout]
            y0 = u[-1, 0, 0]
            assert vf[-1] == case.T and np.all(u[-1].view(np.uint32) == y0.view(np.uint32)), "a computed frame of zeros is not one silence value"
            assert abs(float(y0) - (np.log(mc.FLOOR) if mode == sm.LN else -10.0)) < 1e-4
            for k in range(u.shape[0]):
                assert np.all(u[k, vf[k]:].view(np.uint32) == 0), (case, k)
            want, _ = mc.ranged_want(u, vf, y0, ranged)
            for offset in mc.OFFSETS:
                got = _gpu(ctx, spec, case, a, layout, offset)
                cells += mc.same_words(got, want, (case, MODE_NAMES[mode], ranged, mc.LAYOUT_NAMES[layout], offset), "float32 numpy on the unranged output")
        spec.close()
    print("%s %s: %d cells word for word, 0 differ" % (case, MODE_NAMES[mode], cells))


@pytest.mark.parametrize("case,layout", **mc.with_layouts(mc.ZERO_PAD_CASES))
def test_zero_pad_mode_reads_nothing_from_valid_on(ctx, case, layout):
    """The floats from valid[k] on are NaN: the words of the batch with zeros there."""
    spec = _spec(ctx, case, sm.POWER)
    try:
        got = _gpu(ctx, spec, case, mc.nan_tailed(case), layout)
        mc.same_words(got, _gpu(ctx, spec, case, mc.batch(case)[0], layout), (case, mc.LAYOUT_NAMES[layout]), "the zero-tailed batch")
    finally:
        spec.close()
