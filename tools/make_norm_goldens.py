"""The outside answers of per-utterance normalisation, recorded as data: tests/golden/features/norm_<case>.npz.

claxon_amd.Norm is held by the suite to a float64 formula this project wrote itself (tests/simlib_norm.py).  This tool evaluates the
same step with implementations the project did not write -- the numpy code of transformers' feature extractors -- and writes what
they gave, with the library versions.  tests/norm_cases.py reads the files; no test needs transformers.  Every extractor is built
from constructor arguments: nothing is downloaded and no pretrained configuration is read.

  norm_wav2vec2   Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm on a seeded 16-bit mono signal of 8000 samples over 32768 as
                  float32, padded with zeros to 8200, with an attention mask of 8000 ones.  The outside arithmetic is float32.
  norm_cmvn       Speech2TextFeatureExtractor.utterance_cmvn on the recorded outside fbank of kaldi16.npz ([48, 80] float64, fed as
                  float64: fed float32 the outside sums its columns in float32 and differs from the definition by up to 2e-5),
                  input_length 41 of the 48 frames; means only, variances only and both.
  norm_seamless   SeamlessM4TFeatureExtractor on the same PCM as norm_wav2vec2 (int16 range): its unnormalised output
                  (do_normalize_per_mel_bins=False) as the input, its normalised output as the answer, both unstacked from
                  [T / 2, 160] to [T, 80].  The outside arithmetic is float32, the variance has ddof = 1 and eps 1e-7.

  python tools/make_norm_goldens.py            writes every case
  python tools/make_norm_goldens.py --check    compares with the committed files, array by array, bit for bit"""
import argparse
import os
import sys

os.environ["HF_HUB_OFFLINE"] = "1"                 # (before transformers is imported: it must never look for a network)
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import numpy as np  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OUT = os.path.join(ROOT, "tests", "golden", "features")
SEED, SAMPLES, PADDED, CMVN_LIVE = 2201, 8000, 8200, 41


def versions():
    import transformers
    return "numpy %s, transformers %s" % (np.__version__, transformers.__version__)


def pcm():
    """int16 [SAMPLES]: a 440 Hz tone of amplitude 6000 on an offset of 300 plus N(0, 800) (the offset gives the mean something to remove)."""
    rng = np.random.default_rng(SEED)
    t = np.arange(SAMPLES, dtype=np.float64) / 16000.0
    return np.clip(np.rint(300.0 + 6000.0 * np.sin(2 * np.pi * 440.0 * t) + rng.normal(0.0, 800.0, SAMPLES)), -32768, 32767).astype(np.int16)


def wav2vec2():
    from transformers import Wav2Vec2FeatureExtractor
    p = pcm()
    x = np.zeros(PADDED, dtype=np.float32)
    x[:SAMPLES] = p.astype(np.float32) / np.float32(32768.0)
    mask = np.zeros(PADDED, dtype=np.int32)
    mask[:SAMPLES] = 1
    y = Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm([x.copy()], [mask], padding_value=0.0)[0]
    assert y.dtype == np.float32
    return dict(pcm=p, input=x, valid=np.int64(SAMPLES), output=y, versions=versions())


def cmvn():
    from transformers import Speech2TextFeatureExtractor
    f = np.load(os.path.join(OUT, "kaldi16.npz"))["features"].astype(np.float64)          # [48, 80]
    out = dict(input=f, valid=np.int64(CMVN_LIVE), versions=versions())
    for name, m, v in (("means", True, False), ("vars", False, True), ("both", True, True)):
        y = Speech2TextFeatureExtractor.utterance_cmvn(f.copy(), CMVN_LIVE, normalize_means=m, normalize_vars=v, padding_value=0.0)
        out["output_" + name] = y                            # (float32: the extractor's own last step)
        out["output64_" + name] = _cmvn64(f, CMVN_LIVE, m, v)
    return out


def _cmvn64(f, n, m, v):
    """utterance_cmvn's lines without its float32 cast at the end (the outside's own operations, in float64)."""
    x = f.copy()
    if m:
        x = np.subtract(x, x[:n].mean(axis=0))
    if v:
        x = np.divide(x, x[:n].std(axis=0))
    x[n:] = 0.0
    return x


def seamless():
    from transformers import SeamlessM4TFeatureExtractor
    p = pcm().astype(np.float32) / np.float32(32768.0)
    fe = SeamlessM4TFeatureExtractor()
    raw = fe(p, sampling_rate=16000, return_tensors="np", do_normalize_per_mel_bins=False)["input_features"][0]
    nrm = fe(p, sampling_rate=16000, return_tensors="np", do_normalize_per_mel_bins=True)["input_features"][0]
    T = raw.shape[0] * 2
    return dict(input=np.ascontiguousarray(raw.reshape(T, 80)), valid=np.int64(T), output=np.ascontiguousarray(nrm.reshape(T, 80)),
                versions=versions())


CASES = {"norm_wav2vec2": wav2vec2, "norm_cmvn": cmvn, "norm_seamless": seamless}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    bad = 0
    for name, make in CASES.items():
        d = make()
        path = os.path.join(OUT, name + ".npz")
        if args.check:
            old = np.load(path)
            for k, v in d.items():
                same = str(old[k]) == str(v) if k == "versions" else (np.asarray(v).dtype == old[k].dtype and np.asarray(v).tobytes() == old[k].tobytes())
                if not same:
                    print("%s: %s differs" % (name, k))
                    bad += 1
        else:
            np.savez_compressed(path, **d)
            print("%s: %d bytes" % (path, os.path.getsize(path)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
