"""The reflected front ends (MelSpec.kaldi_reflected, MelSpec.mfcc_reflected) against recorded outside answers:
tests/golden/features/reflected_*.npz from tools/make_reflected_goldens.py, where numpy's np.pad(mode="symmetric") reflects the signal
and transformers.audio_utils.spectrogram(center=False) and scipy.fft.dct do the rest in float64.  Shared by test_outside_reflected_sim.py
and test_gpu_outside_reflected.py; nothing here needs transformers.

outside_cases.py's rules are used as they are.  A reflected spec's cells are by definition the whole-frame spec's cells on the
explicitly reflected samples (claxon_hip.h), so a reflected case is an outside_cases.Case whose batch() is that reflected window --
built here with Kaldi's loop (simlib_melr.kaldi_index), not with numpy's pad -- and whose tables are the snipped sibling's, which the
reflected constructors share word for word: intervals(), definition() and check() then hold the reflected kernel's output, computed
from the unreflected samples (raw_batch()), to the outside values.  What this does not hold to anything outside: the frame count
(T + hop // 2) // hop and the origin hop // 2 - win_length // 2, which decide how far numpy was asked to pad."""
import numpy as np

import claxon_amd as cx
import outside_cases as oc
import simlib_melr as sr

NAMES = ("reflected_fbank16", "reflected_mfcc16")


class ReflectedCase(oc.Case):
    def reflected_spec(self, ctx=None):
        p = self.p
        if self.kind == "kaldi":
            return cx.MelSpec.kaldi_reflected(ctx, sample_rate=p["sample_rate"], n_mels=p["n_mels"], low_freq=p["low_freq"], high_freq=p["high_freq"])
        return cx.MelSpec.mfcc_reflected(ctx, sample_rate=p["sample_rate"], n_ceps=p["n_ceps"], n_mels=p["n_mels"], cepstral_lifter=p["cepstral_lifter"],
                                         use_energy=p["use_energy"], low_freq=p["low_freq"], high_freq=p["high_freq"])

    @property
    def windows(self):
        return [(0, 0)]

    def raw_batch(self):
        """(audio [1, L] float32, valid): the whole stream from sample 0 in a window a few samples longer, NaN from valid on -- what
        the reflected spec is given."""
        x = self.mono(0)
        a = np.full((1, x.size + 5), np.nan, dtype=np.float32)
        a[0, :x.size] = x
        return a, np.array([x.size], dtype=np.uint32)

    def batch(self):
        """The explicitly reflected window the whole-frame sibling would be given, and its valid samples."""
        a, valid = self.raw_batch()
        s = self.tables
        p, vp, T = sr.reflected_batch(a, valid, s.win_length, s.hop, self.n_frames)
        assert p.shape[1] == s.window_len(self.n_frames) and T[0] == self.z["features"].shape[0]
        return p, vp


def case(name):
    if name not in oc._CACHE:
        oc._CACHE[name] = ReflectedCase(name)
    return oc._CACHE[name]
