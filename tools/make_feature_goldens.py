"""The outside answers of the feature front ends, recorded as data: tests/golden/features/<case>.npz.

MelSpec (HTK / Slaney log-mel), MelSpec.whisper, MelSpec.kaldi and MelSpec.mfcc are held by the suite to float64 formulas that this
project wrote itself.  This tool evaluates the same definitions with an implementation the project did not write -- the numpy
float64 code of `transformers.audio_utils` (spectrogram, mel_filter_bank, window_function; its mel_scale="kaldi" with
triangularize_in_mel_space=True is the port of torchaudio's Kaldi compliance code), `WhisperFeatureExtractor` and `scipy.fft.dct` --
on seeded signals of its own, and writes per case one .npz with the int16 PCM [T, C], the case's parameters, the versions of the
three libraries, the outside tables in float64 and the outside features in float64 (for Whisper the extractor's own float32 output
as well).  tests/outside_cases.py reads the files; neither the CPU nor the GPU tests need transformers.  Every extractor is built
from constructor arguments: nothing is downloaded and no pretrained configuration is read.

What is not an outside value, and is marked so in the files ("own" in the parameters): the cepstral lifter 1 + 0.5 Q sin(pi i / Q),
one line of numpy below -- this project's formula, no implementation of it is at hand --, and the energy row of mfcc16_energy, ln
of the frame's energy after the mean's removal and before pre-emphasis and the window, in plain float64 numpy.

The signal is a 440 Hz tone of amplitude 6000 plus N(0, 800), rounded to int16, so that no band is empty and the derived bounds of
the tests stay narrow.  16-bit values over 32768 are exact in float32, and so is the mean of two of them: the outside input is
exactly what StreamSet.read(..., channels=1) produces.

  python tools/make_feature_goldens.py            writes every case
  python tools/make_feature_goldens.py --check    compares with the committed files, array by array, bit for bit"""
import argparse
import json
import os
import sys

os.environ["HF_HUB_OFFLINE"] = "1"                 # (before transformers is imported: it must never look for a network)
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import numpy as np  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OUT = os.path.join(ROOT, "tests", "golden", "features")
FLT_EPSILON = float(np.finfo(np.float32).eps)
PREEMPH = 0.97
WHISPER_LIVE = 5920                                # 0.37 s at 16 kHz: 39 of the 100 frames reach into it

# name: parameters.  samples is the stream's length (kaldi44: three frames exactly); extra is the frames asked for past the last one
# the stream holds; start2 a second window's first sample; red and sparse the kind of noise (signal()).
CASES = {
    "kaldi16": dict(kind="kaldi", red=0.97, sample_rate=16000, n_mels=80, low_freq=20.0, high_freq=0.0, samples=8000, extra=2, start2=777, seed=1601),
    "kaldi8": dict(kind="kaldi", sample_rate=8000, n_mels=23, low_freq=20.0, high_freq=0.0, samples=4000, extra=2, seed=801),
    "kaldi_edges": dict(kind="kaldi", red=0.97, sample_rate=16000, n_mels=40, low_freq=100.0, high_freq=-400.0, samples=8000, extra=2, seed=1602),
    "kaldi44": dict(kind="kaldi", red=0.97, sparse=20, sample_rate=44100, n_mels=80, low_freq=20.0, high_freq=0.0, samples=2 * 441 + 1102, extra=1, seed=4401),
    "mfcc8": dict(kind="mfcc", sample_rate=8000, n_mels=23, n_ceps=13, cepstral_lifter=22.0, use_energy=False, low_freq=20.0, high_freq=0.0,
                  samples=4000, extra=2, seed=802),
    "mfcc16": dict(kind="mfcc", sample_rate=16000, n_mels=23, n_ceps=13, cepstral_lifter=22.0, use_energy=False, low_freq=20.0, high_freq=0.0,
                   samples=8000, extra=2, seed=1603),
    "mfcc16_energy": dict(kind="mfcc", sample_rate=16000, n_mels=23, n_ceps=13, cepstral_lifter=22.0, use_energy=True, low_freq=20.0,
                          high_freq=0.0, samples=8000, extra=2, seed=1604),
    "whisper80": dict(kind="whisper", sample_rate=16000, n_mels=80, seed=1680),
    "whisper128": dict(kind="whisper", sample_rate=16000, n_mels=128, seed=1628),
    "htk_ln": dict(kind="plain", sample_rate=16000, n_fft=400, hop=160, n_mels=80, mel_scale="htk", norm=None, mode="ln", samples=8000,
                   extra=2, seed=1605),
    "slaney_log10": dict(kind="plain", sample_rate=16000, n_fft=400, hop=160, n_mels=80, mel_scale="slaney", norm="slaney", mode="log10",
                         samples=8000, extra=2, seed=1606),
}
# The frames of the full-second Whisper stream whose float64 values are kept (the float32 output is kept for all 100): both ends,
# where the crop is reflected, and either side of the kernel's 32-frame groups.  The short stream keeps all of its live frames.
WHISPER_F64_FRAMES = (0, 1, 2, 30, 31, 32, 33, 62, 63, 64, 65, 94, 95, 96, 97, 98, 99)


def signal(rate, samples, channels, seed, red=0.0, sparse=0):
    """int16 [samples, channels]: 6000 sin(2 pi 440 t) + noise per channel (the tone's phase moves with the channel).  The noise is
    N(0, 800), white; with red > 0 it is n[t] = red n[t - 1] + N(0, 800), which Kaldi's pre-emphasis of the same coefficient
    turns white again: with white noise the pre-emphasised bins below 250 Hz hold so little power beside the sum of the absolute
    terms of their transform that the float32 bound of those bands -- an eighth of an 80-band 16 kHz bank -- says nothing.  With
    sparse = K the noise is N(0, 8000) in one sample of K and N(0, 20) in the others: broadband all the same, but a frame's
    transform is a sum of Nw / K large terms and not of Nw, and the bound of a float32 sum grows with the square root of that
    count -- at 1102 taps dense noise alone puts it at 4 to 5 % of a band's power."""
    rng = np.random.default_rng(seed)
    t = np.arange(samples, dtype=np.float64) / rate
    cols = []
    for c in range(channels):
        n = rng.normal(0.0, 800.0, samples)
        if sparse:
            n = np.where(rng.random(samples) < 1.0 / sparse, rng.normal(0.0, 8000.0, samples), rng.normal(0.0, 20.0, samples))
        if red:
            for i in range(1, samples):
                n[i] += red * n[i - 1]
        cols.append(6000.0 * np.sin(2.0 * np.pi * 440.0 * t + 0.7 * c) + n)
    return np.clip(np.round(np.stack(cols, axis=1)), -32768, 32767).astype(np.int16)


def mono(pcm):
    """What read(..., channels=1) gives: the channels' mean of pcm / 32768, float32, exactly."""
    m = pcm.astype(np.float64).mean(axis=1) / 32768.0
    assert np.array_equal(m.astype(np.float32).astype(np.float64), m)
    return m.astype(np.float32)


def kaldi_shape(rate):
    win, hop = int(rate * 0.001 * 25.0), int(rate * 0.001 * 10.0)
    return win, hop, 1 << (win - 1).bit_length()


def _kaldi_logmel(au, x, p, window, bank):
    win, hop, n_fft = kaldi_shape(p["sample_rate"])
    y = au.spectrogram(x.astype(np.float64) * 32768.0, window, frame_length=win, hop_length=hop, fft_length=n_fft, power=2.0, center=False,
                       preemphasis=PREEMPH, mel_filters=bank, mel_floor=FLT_EPSILON, log_mel="log", remove_dc_offset=True, dtype=np.float64)
    return np.ascontiguousarray(y.T)                           # [frames, n_mels]


def make_kaldi(au, name, p):
    win, hop, n_fft = kaldi_shape(p["sample_rate"])
    pcm = signal(p["sample_rate"], p["samples"], 1, p["seed"], p.get("red", 0.0), p.get("sparse", 0))
    high = p["high_freq"] if p["high_freq"] > 0 else 0.5 * p["sample_rate"] + p["high_freq"]
    bank = au.mel_filter_bank(n_fft // 2 + 1, p["n_mels"], p["low_freq"], high, p["sample_rate"], norm=None, mel_scale="kaldi",
                              triangularize_in_mel_space=True)
    window = au.window_function(win, "povey", periodic=False)
    x = mono(pcm)
    out = dict(pcm=pcm, window=np.asarray(window, np.float64), fbank=np.ascontiguousarray(np.asarray(bank, np.float64).T))
    logmel = _kaldi_logmel(au, x, p, window, bank)
    if p["kind"] == "kaldi":
        out["features"] = logmel
        if "start2" in p:
            out["features2"] = _kaldi_logmel(au, x[p["start2"]:], p, window, bank)
    else:
        from scipy.fft import dct
        n_ceps, Q = p["n_ceps"], p["cepstral_lifter"]
        lifter = 1.0 + 0.5 * Q * np.sin(np.pi * np.arange(n_ceps) / Q)       # this project's formula, not an outside one
        feats = dct(logmel, type=2, norm="ortho", axis=-1)[:, :n_ceps] * lifter[None, :]
        if p["use_energy"]:                                     # own formula, not outside-checked: row 0 is the frame's log energy
            frames = (x.astype(np.float64) * 32768.0)[np.arange(logmel.shape[0])[:, None] * hop + np.arange(win)[None, :]]
            d = frames - frames.mean(axis=1, keepdims=True)
            feats[:, 0] = np.log(np.maximum((d * d).sum(axis=1), FLT_EPSILON))
        out.update(logmel=logmel, features=np.ascontiguousarray(feats), lifter=lifter,
                   dct=np.ascontiguousarray(dct(np.eye(p["n_mels"]), type=2, norm="ortho", axis=0)[:n_ceps]))
        p = dict(p, own=["lifter"] + (["features[:, 0]"] if p["use_energy"] else []))
    return out, p


def make_plain(au, name, p):
    N, H = p["n_fft"], p["hop"]
    pcm = signal(p["sample_rate"], p["samples"], 1, p["seed"])
    bank = au.mel_filter_bank(N // 2 + 1, p["n_mels"], 0.0, p["sample_rate"] / 2.0, p["sample_rate"], norm=p["norm"], mel_scale=p["mel_scale"])
    window = au.window_function(N, "hann", periodic=True)
    x = mono(pcm).astype(np.float64)
    live = -(-x.size // H)                                      # the frames that begin inside the stream: the last ones hang over zeros
    x = np.concatenate([x, np.zeros((live - 1) * H + N - x.size)])
    y = au.spectrogram(x, window, frame_length=N, hop_length=H, power=2.0, center=False, mel_filters=bank, mel_floor=1e-10,
                       log_mel={"ln": "log", "log10": "log10"}[p["mode"]], dtype=np.float64)
    assert y.shape[1] == live
    return dict(pcm=pcm, window=np.asarray(window, np.float64), fbank=np.ascontiguousarray(np.asarray(bank, np.float64).T),
                features=np.ascontiguousarray(y.T)), p


def make_whisper(au, name, p):
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=p["n_mels"], chunk_length=1)
    assert (fe.n_fft, fe.hop_length, fe.n_samples, fe.nb_max_frames, fe.sampling_rate) == (400, 160, 16000, 100, 16000)
    pcm0, pcm1 = signal(16000, WHISPER_LIVE, 1, p["seed"]), signal(16000, 16000, 2, p["seed"] + 1)
    window = au.window_function(400, "hann")
    batch = np.zeros((2, 16000), dtype=np.float32)              # the extractor's own zero padding to one second
    batch[0, :WHISPER_LIVE], batch[1] = mono(pcm0), mono(pcm1)
    f32 = fe._np_extract_fbank_features(batch, "cpu")           # [2, n_mels, 100] float32: the extractor itself
    assert f32.dtype == np.float32 and f32.shape == (2, p["n_mels"], 100)
    f64 = []
    for x in batch:                                             # the extractor's steps with dtype=float64
        y = au.spectrogram(x, window, frame_length=400, hop_length=160, power=2.0, mel_filters=fe.mel_filters, log_mel="log10",
                           dtype=np.float64)[:, :-1]
        y = np.maximum(y, y.max() - 8.0)
        f64.append(((y + 4.0) / 4.0).T)
    frames1 = np.array(WHISPER_F64_FRAMES, dtype=np.int64)
    live0 = -(-(WHISPER_LIVE + 200) // 160)
    assert np.all(f64[0][live0:] == f64[0][live0, 0]), "a frame past the short stream is not the silence value"
    return dict(pcm0=pcm0, pcm1=pcm1, window=np.asarray(window, np.float64),
                fbank=np.ascontiguousarray(np.asarray(fe.mel_filters, np.float64).T),
                features0=np.ascontiguousarray(f64[0][:live0 + 1]), features1=np.ascontiguousarray(f64[1][frames1]), frames1=frames1,
                features32=np.ascontiguousarray(f32.transpose(0, 2, 1))), dict(p, live0=int(live0))


def generate(name):
    """The arrays of one case, as they are written: {key: array}; "params" and "versions" are JSON texts."""
    import scipy
    import transformers
    from transformers import audio_utils as au
    p = dict(CASES[name])
    arrays, p = {"kaldi": make_kaldi, "mfcc": make_kaldi, "plain": make_plain, "whisper": make_whisper}[p["kind"]](au, name, p)
    arrays["params"] = np.array(json.dumps(p, sort_keys=True))
    arrays["versions"] = np.array(json.dumps(dict(transformers=transformers.__version__, numpy=np.__version__, scipy=scipy.__version__),
                                             sort_keys=True))
    return arrays


def installed_versions():
    import scipy
    import transformers
    return dict(transformers=transformers.__version__, numpy=np.__version__, scipy=scipy.__version__)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--check", action="store_true", help="compare with the files in --out and write nothing")
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    bad = 0
    for name in args.cases:
        arrays = generate(name)
        path = os.path.join(args.out, name + ".npz")
        if args.check:
            with np.load(path) as z:
                ok = sorted(z.files) == sorted(arrays) and all(same(z[k], arrays[k]) for k in arrays)
            print("%-14s %s" % (name, "same" if ok else "DIFFERS"))
            bad += not ok
        else:
            os.makedirs(args.out, exist_ok=True)
            np.savez_compressed(path, **arrays)
            print("%-14s %7d bytes  %s" % (name, os.path.getsize(path), " ".join("%s%s" % (k, list(v.shape)) for k, v in sorted(arrays.items()))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
