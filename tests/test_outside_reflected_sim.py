"""The reflected front ends against the recorded outside answers (tests/golden/features/reflected_*.npz; outside_reflected.py says
what is outside-held and what is not), on the CPU: the fixtures are what the tool records, numpy's symmetric pad is Kaldi's loop on
the fixture's signal, the project's float64 definition lies in outside_cases.py's definition interval around the outside values, and
clx_k_mel_fr / clx_k_mel_qr under the wave simulator, given the unreflected samples, lie in the kernel interval -- SHARE_CAP and LN_CAP
as they are."""
import numpy as np
import pytest

import outside_cases as oc
import outside_reflected as orf
import simlib_mel as sm
import simlib_melr as sr


@pytest.mark.parametrize("name", orf.NAMES)
def test_the_fixture_is_the_recipes(name):
    c = orf.case(name)
    p, s = c.p, c.tables
    assert p["samples"] % s.hop != 0 and p["red"] == 0.97 and p["sample_rate"] == 16000 and c.streams[0].shape == (p["samples"], 1)
    assert p["frames"] == (p["samples"] + s.hop // 2) // s.hop == c.z["features"].shape[0]
    assert p["pad_left"] == s.win_length // 2 - s.hop // 2 and p["pad_left"] + p["samples"] + p["pad_right"] == (p["frames"] - 1) * s.hop + s.win_length
    # numpy's symmetric pad, which the outside values were computed on, is Kaldi's loop
    x = c.mono(0)
    a, vp = c.batch()
    assert vp[0] == p["pad_left"] + p["samples"] + p["pad_right"]
    assert np.array_equal(a[0, :vp[0]], np.pad(x, (p["pad_left"], p["pad_right"]), mode="symmetric")) and not a[0, vp[0]:].any()
    # the tables of the reflected constructor are held to the outside tables as the sibling's are
    r = c.reflected_spec(None)
    assert r.reflect_edges and oc.table_ulps(r.window, c.z["window"] * 32768.0) <= 1.0 and oc.table_ulps(r.fbank, c.z["fbank"][:, :r.n_bins]) <= 1.0
    assert r.valid_frames(c.raw_batch()[1], c.n_frames).tolist() == c.valid_frames().tolist() == [p["frames"]]


@pytest.mark.parametrize("name", orf.NAMES)
def test_the_float64_definition_is_the_outside_answer(name):
    c = orf.case(name)
    oc.check(oc.definition(c), c, "float64 definition", kernel=False)


@pytest.mark.parametrize("name", orf.NAMES)
def test_the_reflected_kernels_give_the_outside_answer(name):
    c = orf.case(name)
    r = c.reflected_spec(None)
    a, valid = c.raw_batch()
    cep = None if r.n_ceps is None else dict(n_ceps=r.n_ceps, dct=r.dct, lifter=r.lifter, energy=int(r.energy), energy_scale=r.energy_scale)
    h = sr.create(r.n_fft, r.win_length, r.hop, r.window, r.fbank, r.n_bins, r.n_mels, sm.LN, r.floor, dict(remove_dc=1, preemph=r.preemph), cep)
    assert sr.kernel(h) == ("clx_k_mel_fr" if cep is None else "clx_k_mel_qr")
    T = c.n_frames
    for layout in (sm.CT, sm.TC):
        out = np.full((1, r.n_out, T) if layout == sm.CT else (1, T, r.n_out), np.nan, dtype=np.float32)
        sr.mel_windows(h, a, valid, T, layout, out)
        oc.check(out.transpose(0, 2, 1) if layout == sm.CT else out, c, "simulator layout %d" % layout)
    sr.destroy(h)
