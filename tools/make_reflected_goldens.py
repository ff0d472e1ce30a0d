"""The outside answers of the reflected front ends (MelSpec.kaldi_reflected, MelSpec.mfcc_reflected), recorded as data:
tests/golden/features/reflected_fbank16.npz and reflected_mfcc16.npz.

The signal is make_feature_goldens.py's kaldi16 recipe (a 440 Hz tone plus red noise of coefficient 0.97, 16 bits) with a length
that is no multiple of the hop.  An utterance of T samples has (T + 80) // 160 frames, the first one starting at sample 80 - 200 =
-120: np.pad(x, (120, right), mode="symmetric") -- numpy's reflection with the edge sample repeated, which is Kaldi's -- continues the
signal as far as those frames reach, and transformers.audio_utils.spectrogram(center=False, ...) on the padded signal and, for the
MFCC, scipy.fft.dct do the rest exactly as make_feature_goldens.py's Kaldi route does.  So the reflection (numpy's) and everything
behind it are outside values; the frame count and the origin, which decide the two pad widths, are this project's reading of Kaldi's
feature-window.cc and are not.  The cepstral lifter is the project's own formula, as in make_feature_goldens.py ("own").

At recording time the tool asserts that the outside values alone keep each case within tests/outside_cases.py's SHARE_CAP and LN_CAP
(the check of tests/outside_reflected.py with the outside values in place of an output).

  python tools/make_reflected_goldens.py            writes both cases
  python tools/make_reflected_goldens.py --check    compares with the committed files, array by array, bit for bit"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_feature_goldens as mg  # noqa: E402  (sets the offline switches before transformers is imported)

CASES = {
    "reflected_fbank16": dict(kind="kaldi", red=0.97, sample_rate=16000, n_mels=80, low_freq=20.0, high_freq=0.0, samples=8077, extra=2, seed=1611),
    "reflected_mfcc16": dict(kind="mfcc", red=0.97, sample_rate=16000, n_mels=23, n_ceps=13, cepstral_lifter=22.0, use_energy=False, low_freq=20.0,
                             high_freq=0.0, samples=8077, extra=2, seed=1612),
}


def generate(name):
    import scipy
    import transformers
    from scipy.fft import dct
    from transformers import audio_utils as au
    p = dict(CASES[name])
    win, hop, n_fft = mg.kaldi_shape(p["sample_rate"])
    assert p["samples"] % hop != 0
    pcm = mg.signal(p["sample_rate"], p["samples"], 1, p["seed"], p["red"])
    bank = au.mel_filter_bank(n_fft // 2 + 1, p["n_mels"], p["low_freq"], 0.5 * p["sample_rate"] + p["high_freq"], p["sample_rate"], norm=None,
                              mel_scale="kaldi", triangularize_in_mel_space=True)
    window = au.window_function(win, "povey", periodic=False)
    x = mg.mono(pcm)
    frames = (x.size + hop // 2) // hop
    left = win // 2 - hop // 2
    right = (frames - 1) * hop + win - x.size - left
    assert left >= 0 and 0 <= right <= x.size
    padded = np.pad(x, (left, right), mode="symmetric")
    logmel = mg._kaldi_logmel(au, padded, p, window, bank)
    assert logmel.shape == (frames, p["n_mels"])
    out = dict(pcm=pcm, window=np.asarray(window, np.float64), fbank=np.ascontiguousarray(np.asarray(bank, np.float64).T))
    p = dict(p, pad_left=int(left), pad_right=int(right), frames=int(frames))
    if p["kind"] == "kaldi":
        out["features"] = logmel
    else:
        n_ceps, Q = p["n_ceps"], p["cepstral_lifter"]
        lifter = 1.0 + 0.5 * Q * np.sin(np.pi * np.arange(n_ceps) / Q)       # this project's formula, not an outside one
        feats = dct(logmel, type=2, norm="ortho", axis=-1)[:, :n_ceps] * lifter[None, :]
        out.update(logmel=logmel, features=np.ascontiguousarray(feats), lifter=lifter,
                   dct=np.ascontiguousarray(dct(np.eye(p["n_mels"]), type=2, norm="ortho", axis=0)[:n_ceps]))
        p = dict(p, own=["lifter"])
    out["params"] = np.array(json.dumps(p, sort_keys=True))
    out["versions"] = np.array(json.dumps(dict(transformers=transformers.__version__, numpy=np.__version__, scipy=scipy.__version__), sort_keys=True))
    return out


def within_the_caps(name):
    """outside_cases.check with the outside values in place of an output: asserts the share of cells whose allowed error is above
    LN_CAP stays below SHARE_CAP."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import outside_cases as oc
    import outside_reflected as orf
    oc._CACHE.pop(name, None)
    c = orf.case(name)
    got = np.zeros((1, c.n_frames, c.tables.n_out))
    got[0, :c.z["features"].shape[0]] = c.z["features"]
    return oc.check(got, c, "the outside values themselves")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=mg.OUT)
    ap.add_argument("--check", action="store_true", help="compare with the files in --out and write nothing")
    args = ap.parse_args()
    largest = max(os.path.getsize(os.path.join(mg.OUT, f)) for f in os.listdir(mg.OUT) if f.endswith(".npz") and not f.startswith("reflected_"))
    bad = 0
    for name in CASES:
        arrays = generate(name)
        path = os.path.join(args.out, name + ".npz")
        if args.check:
            with np.load(path) as z:
                ok = sorted(z.files) == sorted(arrays) and all(mg.same(z[k], arrays[k]) for k in arrays)
            print("%-18s %s" % (name, "same" if ok else "DIFFERS"))
            bad += not ok
        else:
            os.makedirs(args.out, exist_ok=True)
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            print("%-18s %7d bytes  %s" % (name, size, " ".join("%s%s" % (k, list(v.shape)) for k, v in sorted(arrays.items()))))
            assert size <= largest, "%s is larger than the largest fixture already there (%d bytes)" % (name, largest)
            if os.path.abspath(args.out) == os.path.abspath(mg.OUT):
                within_the_caps(name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
