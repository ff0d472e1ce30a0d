"""The mel, fbank, MFCC and Whisper front ends against an implementation this project did not write, on the CPU: the fixtures of
tools/make_feature_goldens.py (tests/golden/features) are what the tool writes; MelSpec's tables are the outside tables, cell by
cell; the float64 references of simlib_mel / simlib_melk / simlib_melq and the Whisper range step are the outside features; and
clx_k_mel, clx_k_mel_c with clx_k_mel_range, clx_k_mel_f and clx_k_mel_q under the wave simulator give the recorded outside values
within the bounds of DESIGN.md 4.14 (outside_cases.py has the rules).  Only the first test and the sharp comparison need
transformers; everything else reads the fixtures and never skips."""
import importlib.util
import os

import numpy as np
import pytest

import outside_cases as oc
import simlib_mel as sm
import simlib_melc as sc
import simlib_melk as sk
import simlib_melq as sq

NAN_FILL = 0x7fc0dead
GUARD = 0xffc0beef
LAYOUTS = (sm.CT, sm.TC)
# The worst relative difference of the band powers between the outside spectrogram() fed this project's float32 tables and
# simlib_mel / simlib_melk's float64 definition with the transform rounded to complex64 as the outside keeps it, over all cases
# (measured on the CPU, printed by test_the_definitions_are_the_outside_mathematics): the same mathematics in float64 twice.
SHARP_MEASURED = 8.0e-16
SHARP_FACTOR = 1000.0


def _offline_transformers():
    os.environ["HF_HUB_OFFLINE"] = "1"
    os.environ["TRANSFORMERS_OFFLINE"] = "1"
    return pytest.importorskip("transformers")


def _tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_feature_goldens.py")
    spec = importlib.util.spec_from_file_location("make_feature_goldens", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- a. the fixtures are what the tool writes ---------------------------------------------------------------------------------------

def test_fixtures_are_what_the_tool_writes():
    """Every case regenerated in memory equals the committed file array by array, bit for bit -- provided the recorded versions of
    transformers, numpy and scipy are the installed ones; otherwise the outside code may have moved and the test skips, naming both."""
    _offline_transformers()
    pytest.importorskip("scipy")
    tool = _tool()
    assert tuple(tool.CASES) == oc.NAMES
    have = tool.installed_versions()
    for name in oc.NAMES:
        c = oc.case(name)
        if c.versions != have:
            pytest.skip("%s was recorded with %r, installed is %r" % (name, c.versions, have))
        made = tool.generate(name)
        assert sorted(made) == sorted(c.z), (name, sorted(made), sorted(c.z))
        for key in made:
            assert tool.same(made[key], c.z[key]), (name, key)
        assert os.path.getsize(os.path.join(oc.DIR, name + ".npz")) < 256 << 10, "a fixture file has grown large"


# ---- b. tables --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", oc.NAMES)
def test_tables_are_the_outside_tables(name):
    """fbank and window: every cell within one float32 ulp of the outside float64 value (both sides round a float64 value once; one
    ulp, not half, leaves room for another libm; measured 0.50) and zero in the same cells.  A Kaldi spec holds the first n_bins
    rows of the outside bank, whose other rows -- the Nyquist bin -- are all zero: that is why 256 of the 257 bins suffice.  Kaldi's
    window carries the int16-range scale 32768, a power of two.  dct and lifter: within one ulp, or 1e-15 where the exact value is
    0 (scipy gives about 1e-17 for cos(pi / 2))."""
    c = oc.case(name)
    s = c.tables
    bank = c.z["fbank"]
    assert bank.shape == (s.n_mels, s.n_fft // 2 + 1) and s.fbank.shape == (s.n_mels, s.n_bins)
    assert np.all(bank[:, s.n_bins:] == 0), "an outside row past n_bins is not all zero"
    assert (s.n_bins == s.n_fft // 2) == (c.kind in ("kaldi", "mfcc"))
    worst = {"fbank": oc.table_ulps(s.fbank, bank[:, :s.n_bins])}
    if c.kind in ("kaldi", "mfcc"):
        w = s.window / np.float32(32768.0)
        assert np.array_equal(w * np.float32(32768.0), s.window)
        worst["window"] = oc.table_ulps(w, c.z["window"])
    else:
        worst["window"] = oc.table_ulps(s.window, c.z["window"])
    if c.cepstral:
        worst["dct"] = oc.table_ulps(s.dct, c.z["dct"], zero_abs=1e-15)
        worst["lifter"] = oc.table_ulps(s.lifter, c.z["lifter"])
    print(name, " ".join("%s %.2f ulp" % kv for kv in worst.items()))
    for what, ulps in worst.items():
        assert ulps <= 1.0, (name, what, ulps)


# ---- c. definitions ---------------------------------------------------------------------------------------------------------------

def _outside_power(au, c, k):
    """The outside spectrogram() of window k with this project's float32 tables: band powers [frames, n_mels] in float64."""
    s = c.tables
    a, _ = c.batch()
    bank = np.zeros((s.n_fft // 2 + 1, s.n_mels), dtype=np.float64)
    bank[:s.n_bins] = s.fbank.T.astype(np.float64)
    kw = dict(preemphasis=float(s.preemph), remove_dc_offset=True) if c.kind in ("kaldi", "mfcc") else {}
    y = au.spectrogram(a[k].astype(np.float64), s.window.astype(np.float64), frame_length=s.win_length, hop_length=s.hop, fft_length=s.n_fft,
                       power=2.0, center=bool(s.center), pad_mode="reflect", mel_filters=bank, mel_floor=0.0, log_mel=None, **kw)
    return np.asarray(y, dtype=np.float64).T[:c.n_frames]


def test_the_definitions_are_the_outside_mathematics():
    """The sharp comparison: the outside spectrogram() evaluated a second time, with this project's float32 tables as its window
    and mel_filters and float32(0.97) as its pre-emphasis, against simlib_mel.reference / simlib_melk.reference in float64.  One
    difference of convention remains and is stated on our side for this test: the outside keeps its transform in complex64
    (np.empty(.., dtype=np.complex64) in spectrogram()), so re and im are rounded to float32 once before they are squared;
    reference(..., spectrum=np.float32) does the same.  Both sides are then the same mathematics in float64 and agree to float64
    noise: the tolerance is SHARP_FACTOR times the worst relative difference measured, and stays below 2^-24, so that this step
    adds nothing a float32 kernel could hide in.  (Without the spectrum rounding the two differ by up to 1.2e-7 -- 2^-23, two
    float32 roundings of a power --, which could not stay below 2^-24: DESIGN.md 4.14.)"""
    _offline_transformers()
    from transformers import audio_utils as au
    worst, unrounded = 0.0, 0.0
    for name in oc.NAMES:
        c = oc.case(name)
        ours, plain = oc.power(c, spectrum=np.float32)[0], oc.power(c)[0]
        for k in range(len(c.windows)):
            out = _outside_power(au, c, k)
            live = out > 0                                   # (a frame of the zeros behind the stream has no power, on either side)
            assert out.shape == ours[k].shape and np.all(live[:c.valid_frames()[k]]) and np.all(ours[k][~live] == 0), (name, k, out.shape)
            rel = float(np.max(np.abs(ours[k][live] - out[live]) / out[live]))
            unrounded = max(unrounded, float(np.max(np.abs(plain[k][live] - out[live]) / out[live])))
            print("%s window %d: worst relative difference of the band powers %.3g" % (name, k, rel))
            worst = max(worst, rel)
    print("all cases: %.3g (with the transform in float64 on our side: %.3g)" % (worst, unrounded))
    assert SHARP_FACTOR * SHARP_MEASURED < 2.0 ** -24
    assert worst <= SHARP_FACTOR * SHARP_MEASURED, worst


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_float64_definitions_give_the_recorded_outside_features(name):
    """simlib_mel.reference, simlib_melk.reference, simlib_melq.reference and the centred pad of simlib_melc.pad_batch followed by the
    range step in float64, each with the spec's float32 tables, against the recorded outside features: the slack is 4.14's table
    term alone (no kernel bound, no LOG_ULPS).  Frames past valid_frames are the outside's value for zero-padded audio in the Whisper
    cases and 0 in the others."""
    c = oc.case(name)
    oc.check(oc.definition(c), c, "definition", kernel=False)


# ---- d. the kernels under the simulator ---------------------------------------------------------------------------------------------

def _sim(c, layout):
    """The case's one call under the simulator: [B, n_frames, n_out] float32, with the guard word's and the fill's checks."""
    s = c.tables
    a, valid = c.batch()
    mode = sm.MODES[s.mode]
    if c.kind == "plain":
        mod, h, kern = sm, sm.create(s.n_fft, s.hop, s.window, s.fbank, s.n_mels, mode, s.floor), "clx_k_mel"
    elif c.whisper:
        opts = dict(center=1, pad=sc.PAD_REFLECT, range=1, range_width=s.top, shift=s.shift, scale=s.scale)
        mod, h, kern = sc, sc.create(s.n_fft, s.hop, s.window, s.fbank, s.n_mels, mode, s.floor, opts), "clx_k_mel_c"
    else:
        opts = dict(remove_dc=int(s.remove_dc), whole_frames=int(s.whole_frames), preemph=s.preemph)
        if c.cepstral:
            cep = dict(n_ceps=s.n_ceps, dct=s.dct, lifter=s.lifter, energy=int(s.energy), energy_scale=s.energy_scale, energy_floor=s.energy_floor)
            mod, h = sq, sq.create(s.n_fft, s.win_length, s.hop, s.window, s.fbank, s.n_bins, s.n_mels, mode, s.floor, opts, cep)
        else:
            mod, h = sk, sk.create(s.n_fft, s.win_length, s.hop, s.window, s.fbank, s.n_bins, s.n_mels, mode, s.floor, opts)
        kern = mod.kernel(h)
        assert kern == ("clx_k_mel_q" if c.cepstral else "clx_k_mel_f")
    B, T, rows = a.shape[0], c.n_frames, s.n_out
    n = B * rows * T
    raw = np.full(n + 8, NAN_FILL, dtype=np.uint32)
    buf = raw[3:3 + n + 1]
    buf[n] = GUARD
    try:
        if mod is sm:
            mod.mel_windows(h, a, valid, T, layout, buf)
            vf = c.valid_frames()
        else:
            vf = mod.mel_windows(h, a, valid, T, layout, buf, tables=True)[1]
    finally:
        mod.destroy(h)
    assert np.array_equal(np.asarray(vf, dtype=np.int64), c.valid_frames()), (c, vf)
    assert buf[n] == GUARD and np.all(raw[:3] == NAN_FILL), "a word outside the output was written"
    assert not np.any(buf[:n] == NAN_FILL), "an output word was not written"
    out = buf[:n].view(np.float32)
    return (out.reshape(B, rows, T).transpose(0, 2, 1) if layout == sm.CT else out.reshape(B, T, rows)), kern


@pytest.mark.parametrize("layout", LAYOUTS, ids=("ct", "tc"))
@pytest.mark.parametrize("name", oc.NAMES)
def test_the_kernels_give_the_recorded_outside_features(name, layout):
    """clx_k_mel (htk_ln, slaney_log10), clx_k_mel_c with clx_k_mel_range (whisper80, whisper128), clx_k_mel_f (kaldi*) and
    clx_k_mel_q (mfcc*) on each case's audio: every cell inside the interval around the recorded outside value -- the kernel's dM
    plus 4.14's table term through the logarithm with LOG_ULPS, the cepstra's dC carried through the DCT row's absolute sum --,
    the Whisper cells also inside the one around the extractor's own float32 output, frames past valid_frames the outside's value
    for zero-padded audio (Whisper) or exactly 0, and fewer than 5 % of a case's cells with an allowed error above 5 % of the
    band's power (0.05 in a ln cell), so that the bound cannot go vacuous."""
    c = oc.case(name)
    got, kern = _sim(c, layout)
    oc.check(got, c, kern, kernel=True)
