"""The feature front ends against an implementation this project did not write: the recorded answers of tools/make_feature_goldens.py
(tests/golden/features/*.npz: transformers.audio_utils, WhisperFeatureExtractor and scipy.fft.dct in float64 on seeded 16-bit
signals) and the rules by which a table, a float64 definition and a kernel's output are held to them.  Shared by the CPU tests
(test_outside_features_sim.py) and the GPU tests (test_gpu_outside_features.py); nothing here needs transformers.

A case gives its spec (MelSpec with ctx=None: the tables alone), its windows -- (stream, first sample) --, n_frames (a few more than
the stream holds, so that dead frames are asked for), the batch that read(..., channels=1) gives for them, and per window the
interval [lo, hi] of every cell around the outside value:

  D = dM + dT per band cell, dM the kernel's own bound (simlib_mel.reference / simlib_melk.reference, 4.10 / 4.12) and dT the
  table term: the window and the bank are float32 here and float64 outside, each entry within one float32 ulp (what the table tests
  assert: relative g(2)), the pre-emphasis coefficient is float32(0.97) here and the double 0.97 outside (g(1)), and the outside
  keeps its transform in complex64 (u per component).  The outside power M_s is recovered from the recorded logarithm, the kernel's
  band sum lies in M_s +- D, its logarithm in [log(max(M_s - D, floor)), log(max(M_s + D, floor))] widened by LOG_ULPS float32 ulps,
  and the steps behind the logarithm (Whisper's clamp, shift and scale; the DCT and the lifter) carry the interval on, every
  rounded operation widened by one ulp of the larger end.

kernel=False leaves dM, LOG_ULPS and the ulps out: the interval our own float64 definition must lie in."""
import json
import os

import numpy as np

import claxon_amd as cx
import simlib_mel as sm
import simlib_melc as sc
import simlib_melk as sk

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features")
NAMES = ("kaldi16", "kaldi8", "kaldi_edges", "kaldi44", "mfcc8", "mfcc16", "mfcc16_energy", "whisper80", "whisper128", "htk_ln", "slaney_log10")
KALDI_NAMES = tuple(n for n in NAMES if n.startswith(("kaldi", "mfcc")))
U, g = sm.U, sm.g
U64 = 2.0 ** -53
NOISE64 = 1e-12                  # float64 evaluation behind the band sums: a logarithm, at most 128 products of magnitude <= 40
SHARE_CAP = 0.05                 # at most this share of a case's cells may have an allowed error above 5 % of the band's power
LN_CAP = 0.05                    # .. which is 0.05 absolute in a ln cell
_CACHE = {}


def g64(k):
    return k * U64 / (1.0 - k * U64)


def _ulp(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


class Case:
    def __init__(self, name):
        self.name = name
        with np.load(os.path.join(DIR, name + ".npz")) as z:
            self.z = {k: z[k] for k in z.files}
        for a in self.z.values():
            a.setflags(write=False)
        self.p = json.loads(str(self.z["params"]))
        self.versions = json.loads(str(self.z["versions"]))
        self.kind = self.p["kind"]
        self.whisper, self.cepstral = self.kind == "whisper", self.kind == "mfcc"
        self.energy = bool(self.p.get("use_energy"))

    def __repr__(self):
        return self.name

    def spec(self, ctx=None):
        """The case's MelSpec by its constructor; ctx=None: the tables alone."""
        p = self.p
        if self.kind == "kaldi":
            return cx.MelSpec.kaldi(ctx, sample_rate=p["sample_rate"], n_mels=p["n_mels"], low_freq=p["low_freq"], high_freq=p["high_freq"])
        if self.kind == "mfcc":
            return cx.MelSpec.mfcc(ctx, sample_rate=p["sample_rate"], n_ceps=p["n_ceps"], n_mels=p["n_mels"], cepstral_lifter=p["cepstral_lifter"],
                                   use_energy=p["use_energy"], low_freq=p["low_freq"], high_freq=p["high_freq"])
        if self.kind == "whisper":
            return cx.MelSpec.whisper(ctx, n_mels=p["n_mels"])
        return cx.MelSpec(ctx, p["sample_rate"], n_fft=p["n_fft"], hop=p["hop"], n_mels=p["n_mels"], mel_scale=p["mel_scale"], norm=p["norm"],
                          mode=p["mode"])

    @property
    def tables(self):
        """The tables-only spec, built once."""
        if "_tables" not in self.__dict__:
            self.__dict__["_tables"] = self.spec(None)
        return self.__dict__["_tables"]

    @property
    def streams(self):
        """The PCM of the case's streams, each int16 [T, C]."""
        return [self.z["pcm0"], self.z["pcm1"]] if self.whisper else [self.z["pcm"]]

    @property
    def windows(self):
        """(stream, first sample) of every window of the case's one call."""
        if self.whisper:
            return [(0, 0), (1, 0)]
        return [(0, 0)] + ([(0, self.p["start2"])] if "start2" in self.p else [])

    @property
    def n_frames(self):
        return 100 if self.whisper else int(self.z["features"].shape[0]) + int(self.p["extra"])

    def mono(self, stream):
        """read(..., channels=1)'s samples of a stream: the channels' mean of pcm / 32768, exact in float32."""
        m = self.streams[stream].astype(np.float64).mean(axis=1) / 32768.0
        assert np.array_equal(m.astype(np.float32).astype(np.float64), m)
        return m.astype(np.float32)

    def batch(self):
        """(audio [B, L] float32, valid uint32): what read(ids, starts, L, "ct", channels=1) gives, zeros from valid[k] on."""
        L = self.tables.window_len(self.n_frames)
        a, valid = np.zeros((len(self.windows), L), dtype=np.float32), []
        for k, (s, st) in enumerate(self.windows):
            x = self.mono(s)[st:st + L]
            a[k, :x.size] = x
            valid.append(x.size)
        return a, np.array(valid, dtype=np.uint32)

    def valid_frames(self):
        return self.tables.valid_frames(self.batch()[1], self.n_frames)

    def outside(self, k, f32=False):
        """(frames, values [len(frames), n_out]) of window k: the recorded outside features and the frames they belong to.  f32: the
        Whisper extractor's own float32 output (all 100 frames)."""
        z = self.z
        if not self.whisper:
            O = z["features2" if k else "features"]
            return np.arange(O.shape[0]), O
        if f32:
            return np.arange(100), z["features32"][k].astype(np.float64)
        if k == 0:                                           # every frame past the short stream is the silence value of frame live0
            live0 = self.p["live0"]
            return np.arange(100), np.concatenate([z["features0"][:live0], np.repeat(z["features0"][live0:live0 + 1], 100 - live0, axis=0)])
        return z["frames1"], z["features1"]


def case(name):
    if name not in _CACHE:
        _CACHE[name] = Case(name)
    return _CACHE[name]


# ---- tables ---------------------------------------------------------------------------------------------------------------------------

def table_ulps(ours32, outside64, zero_abs=0.0):
    """The worst distance of the float32 table from the outside float64 value in float32 ulps of that value, after the check that
    both are zero in the same cells.  zero_abs: an outside value of at most this size counts as the exact 0 it stands for."""
    ours32, outside64 = np.asarray(ours32), np.asarray(outside64, dtype=np.float64)
    assert ours32.dtype == np.float32 and ours32.shape == outside64.shape, (ours32.dtype, ours32.shape, outside64.shape)
    zero = np.abs(outside64) <= zero_abs
    if zero_abs:
        assert np.all(np.abs(ours32[zero]) <= zero_abs), "a cell that is 0 outside is not 0 here"
    else:
        assert np.array_equal(ours32 != 0, ~zero), "the zero pattern differs in %d cells" % int(np.count_nonzero((ours32 != 0) == zero))
    live = ~zero
    if not live.any():
        return 0.0
    return float(np.max(np.abs(ours32[live].astype(np.float64) - outside64[live]) / _ulp(outside64[live])))


# ---- the definition in float64 and the terms of the bound -------------------------------------------------------------------------------

def _framing(c):
    """(Nw, N, H, n_bins, remove_dc, preemph, P) of the case's spec."""
    s = c.tables
    return s.win_length, s.n_fft, s.hop, s.n_bins, bool(s.remove_dc), float(s.preemph), (s.n_fft // 2 if s.center else 0)


def power(c, spectrum=None):
    """(M64, dM), each [B, n_frames, n_mels]: the project's float64 definition of the band sums on the case's batch with the spec's
    float32 tables, and the kernel's bound -- simlib_mel.reference (on the reflect-padded batch for a centred spec) or
    simlib_melk.reference.  spectrum: see those."""
    key = (c.name, "power", spectrum)
    if key not in _CACHE:
        s, (a, _) = c.tables, c.batch()
        Nw, N, H, n_bins, dc, pre, P = _framing(c)
        if c.kind in ("kaldi", "mfcc"):
            _CACHE[key] = sk.reference(a, s.window, s.fbank, N, H, c.n_frames, dc, pre, spectrum=spectrum)
        else:
            ap = sc.pad_batch(a, P, sc.PAD_REFLECT) if P else a
            _CACHE[key] = sm.reference(ap, s.window, s.fbank, N, H, c.n_frames, spectrum=spectrum)
    return _CACHE[key]


def table_term(c):
    """dT [B, n_frames, n_mels]: how far the outside band sum -- float64 tables, the double 0.97, the transform kept
    in complex64 -- can lie from this project's float64 definition with its float32 tables, from the sums of the absolute terms."""
    key = (c.name, "dT")
    if key in _CACHE:
        return _CACHE[key]
    s, (a, _) = c.tables, c.batch()
    Nw, N, H, n_bins, dc, pre, P = _framing(c)
    ap = sc.pad_batch(a, P, sc.PAD_REFLECT) if P else a
    X = sk.frames_of(np.asarray(ap, dtype=np.float64), Nw, H, c.n_frames)              # [B, T, Nw]
    mu = X.mean(axis=-1, keepdims=True) if dc else np.zeros(X.shape[:-1] + (1,))
    d = X - mu
    prev = np.concatenate([d[..., :1], d[..., :-1]], axis=-1)
    y = d - pre * prev
    Cb, Sb = sk.basis64(s.window, N, n_bins)
    fb = np.asarray(s.fbank, dtype=np.float64)
    t = g(2)                                                 # a table entry within one float32 ulp of the outside value
    noise = g64(4 * Nw + 64) * (1.0 + pre) * (np.abs(X) + np.abs(mu))                  # both float64 evaluations, transform included
    E = 0.0
    for B_ in (Cb, Sb):
        r = y @ B_.T
        dr = t * (np.abs(y) @ np.abs(B_).T) + g(1) * pre * (1.0 + t) * (np.abs(prev) @ np.abs(B_).T) + (1.0 + t) * (noise @ np.abs(B_).T)
        dr = dr + U * (np.abs(r) + dr)                       # the complex64 store of the outside transform
        E = E + 2.0 * np.abs(r) * dr + dr * dr
    Pw = power_bins(c)
    _CACHE[key] = E @ fb.T + (t + g64(n_bins + 2)) * ((Pw + E) @ fb.T)
    return _CACHE[key]


def power_bins(c):
    """P [B, n_frames, n_bins] of the float64 definition."""
    s, (a, _) = c.tables, c.batch()
    Nw, N, H, n_bins, dc, pre, P = _framing(c)
    ap = sc.pad_batch(a, P, sc.PAD_REFLECT) if P else a
    X = sk.frames_of(np.asarray(ap, dtype=np.float64), Nw, H, c.n_frames)
    d = X - (X.mean(axis=-1, keepdims=True) if dc else 0.0)
    y = d - pre * np.concatenate([d[..., :1], d[..., :-1]], axis=-1)
    Cb, Sb = sk.basis64(s.window, N, n_bins)
    return (y @ Cb.T) ** 2 + (y @ Sb.T) ** 2


def energy_terms(c):
    """(le64, dE / E handled inside): (E64, dE) [B, n_frames] of the frame energy times energy_scale -- the definition in float64
    and the bound of its float32 evaluation in any order: the mean within dmu = g(Nw + 1) mean|x|, d[n] = fl32(x[n] - mu) within
    dd = dmu + u (|d| + dmu), the Nw squares and their sum within g(Nw + 4) of the sum of the computed squares."""
    s, (a, _) = c.tables, c.batch()
    Nw, N, H, n_bins, dc, pre, P = _framing(c)
    X = sk.frames_of(np.asarray(a, dtype=np.float64), Nw, H, c.n_frames)
    mu = X.mean(axis=-1, keepdims=True)
    dmu = g(Nw + 1) * np.abs(X).mean(axis=-1, keepdims=True)
    d = X - mu
    dd = dmu + U * (np.abs(d) + dmu)
    e, sq = (d * d).sum(axis=-1), (2.0 * np.abs(d) * dd + dd * dd).sum(axis=-1)
    return e * s.energy_scale, (sq + g(Nw + 4) * (e + sq)) * s.energy_scale


def _log(c, m):
    return np.log10(m) if c.tables.mode == "log10" else np.log(m)


def _exp(c, y):
    return 10.0 ** y if c.tables.mode == "log10" else np.exp(y)


def _widen(lo, hi, kernel):
    if not kernel:
        return lo - NOISE64, hi + NOISE64
    u = np.maximum(_ulp(lo), _ulp(hi))
    return lo - u, hi + u


def intervals(c, k, kernel=True, f32=False):
    """(frames, O, lo, hi, cap) of window k: the recorded outside values O [len(frames), n_out] of the frames `frames`, the interval
    every such cell of the output must lie in, and per cell the allowed error that 5 % of the band's power comes to (the vacuity
    cap counts the cells whose interval reaches further).  kernel=False: the interval of the project's float64 definition.
    f32 (Whisper): around the extractor's own float32 output, one float32 ulp of the cell wider."""
    s = c.tables
    frames, O = c.outside(k, f32)
    D = table_term(c)[k] + (power(c)[1][k] if kernel else 0.0)                        # [n_frames, n_mels]
    vf = int(c.valid_frames()[k])
    floor = s.floor
    if c.whisper:
        # every frame's interval from the float32 output (all 100 frames are in it): the window's maximum needs them all
        _, O32 = c.outside(k, True)
        ys = O32 / s.scale - s.shift
        clamped = ys <= ys.max() - s.top + 1e-5              # the outside cell sits on the clamp: its own power is only known to be below
        slack = (_ulp(O32) / abs(s.scale))
        Ms = _exp(c, ys)
        lo = np.where(clamped, np.log10(floor), _log(c, np.maximum(Ms - D, floor)) - slack)
        hi = _log(c, np.maximum(Ms + D, floor)) + slack
        if not f32:                                          # the frames kept in float64: their own, sharper interval
            y64 = O / s.scale - s.shift
            M64 = _exp(c, y64)
            cl = clamped[frames]
            lo[frames] = np.where(cl, lo[frames], _log(c, np.maximum(M64 - D[frames], floor)))
            hi[frames] = np.where(cl, hi[frames], _log(c, np.maximum(M64 + D[frames], floor)))
        lo[vf:] = hi[vf:] = np.log10(floor)                  # a dead frame is finish(0)
        if kernel:
            lo, hi = lo - sm.LOG_ULPS * _ulp(lo), hi + sm.LOG_ULPS * _ulp(hi)
        else:
            lo, hi = lo - NOISE64, hi + NOISE64
        clo, chi = _widen(lo.max() - s.top, hi.max() - s.top, kernel)
        lo, hi = np.maximum(lo, clo), np.maximum(hi, chi)
        lo, hi = _widen(lo + s.shift, hi + s.shift, kernel)
        lo, hi = _widen(lo * s.scale, hi * s.scale, kernel)
        if f32:
            lo, hi = lo - _ulp(O32), hi + _ulp(O32)
        cap = np.full(O.shape, LN_CAP / np.log(10.0) * abs(s.scale))
        return frames, O, lo[frames], hi[frames], cap
    T = O.shape[0]
    assert T == vf, (c, k, T, vf)
    Ol = c.z["logmel"] if c.cepstral else O                  # the outside log-mel cells [T, n_mels]
    Ms = _exp(c, Ol)
    lo, hi = _log(c, np.maximum(Ms - D[:T], floor)), _log(c, np.maximum(Ms + D[:T], floor))
    if kernel:
        lo, hi = lo - sm.LOG_ULPS * _ulp(lo), hi + sm.LOG_ULPS * _ulp(hi)
    else:
        lo, hi = lo - NOISE64, hi + NOISE64
    if not c.cepstral:
        return frames, O, lo, hi, np.full(O.shape, LN_CAP / (np.log(10.0) if s.mode == "log10" else 1.0))
    # cepstra: the outside DCT (scipy's, float64) of the outside log-mel cells against the kernel's fmaf chain over its own cells with
    # the float32 DCT, each entry within one ulp of the outside one (or 1e-15 where that is 0), then the lifter, within one ulp too
    Dm = np.asarray(s.dct, dtype=np.float64)
    l = np.ones(s.n_ceps) if s.lifter is None else np.asarray(s.lifter, dtype=np.float64)
    aD = np.abs(Dm)
    dY = np.maximum(hi - Ol, Ol - lo)
    t = g(2)
    dC = dY @ aD.T + ((g(s.n_mels + 1) if kernel else g64(s.n_mels + 1)) + t) * ((np.abs(Ol) + dY) @ aD.T) + 1e-15 * np.abs(Ol).sum(axis=-1, keepdims=True)
    dC = dC * np.abs(l)[None, :] + t * np.abs(O)
    dC = dC + (_ulp(np.abs(O) + dC) if kernel else NOISE64)
    cap = LN_CAP * (np.abs(l) * aD.sum(axis=1))[None, :] * np.ones_like(O)
    lo_c, hi_c = O - dC, O + dC
    if c.energy:                                             # row 0: own formula, not outside-checked -- ln of the frame's energy
        E, dE = energy_terms(c)
        E, dE = E[k, :T], dE[k, :T] if kernel else 0.0
        eps = cx.FLT_EPSILON
        elo, ehi = np.log(np.maximum(E - dE, eps)), np.log(np.maximum(E + dE, eps))
        elo, ehi = (elo - sm.LOG_ULPS * _ulp(elo), ehi + sm.LOG_ULPS * _ulp(ehi)) if kernel else (elo - NOISE64, ehi + NOISE64)
        lo_c[:, 0], hi_c[:, 0], cap[:, 0] = elo, ehi, LN_CAP
    return frames, O, lo_c, hi_c, cap


def definition(c):
    """[B, n_frames, n_out] float64: the project's own float64 definition of the case's features on its batch -- the references of
    simlib_mel / simlib_melk / simlib_melq, and for Whisper the centred pad of simlib_melc.pad_batch followed by the range step in
    float64 (a dead frame is log10 of the floor)."""
    import simlib_melq as sq
    s, (a, _) = c.tables, c.batch()
    Nw, N, H, n_bins, dc, pre, P = _framing(c)
    vf = c.valid_frames()
    if c.cepstral:
        C64, _ = sq.reference(a, s.window, s.fbank, N, H, c.n_frames, dc, pre, s.floor, s.dct, s.lifter)
        if c.energy:
            C64 = C64.copy()
            C64[:, :, 0] = np.log(np.maximum(energy_terms(c)[0], cx.FLT_EPSILON))
        out = C64
    else:
        out = _log(c, np.maximum(power(c)[0], s.floor))
    out = out.copy()
    for k in range(out.shape[0]):
        out[k, vf[k]:] = np.log10(s.floor) if c.whisper else 0.0
    if c.whisper:
        out = (np.maximum(out, out.reshape(out.shape[0], -1).max(axis=1)[:, None, None] - s.top) + s.shift) * s.scale
    return out


def check(got, c, what, kernel=True):
    """got [B, n_frames, n_out] against the recorded outside values: every frame past valid_frames exactly 0 (Whisper: inside the
    silence value's interval, like any cell), every other cell inside its interval -- Whisper's also inside the one around the
    extractor's float32 output.  Prints and returns (worst |error| / allowed, the share of cells whose allowed error is above the
    cap, cells compared); the share is asserted to be below SHARE_CAP."""
    got = np.asarray(got)
    vf = c.valid_frames()
    worst, wide, cells = 0.0, 0, 0
    for k in range(len(c.windows)):
        g_k = got[k].astype(np.float64)
        if not c.whisper:
            assert np.all(np.ascontiguousarray(got[k, vf[k]:]) == 0) and not np.any(np.signbit(got[k, vf[k]:])), (what, k, "a frame past valid_frames is not +0.0")
        for f32 in (False, True) if c.whisper else (False,):
            frames, O, lo, hi, cap = intervals(c, k, kernel=kernel, f32=f32)
            v = g_k[frames]
            bad = np.argwhere(~((lo <= v) & (v <= hi)))
            assert bad.size == 0, (what, "window %d%s: %d cells outside; frame %d row %d: %r, outside value %r, interval [%r, %r]" % (
                k, " (float32 output)" if f32 else "", bad.shape[0], frames[bad[0][0]], bad[0][1], v[tuple(bad[0])], O[tuple(bad[0])],
                lo[tuple(bad[0])], hi[tuple(bad[0])]))
            allowed = np.maximum(hi - O, O - lo)
            worst = max(worst, float(np.max(np.abs(v - O) / allowed)))
            if not f32:
                wide += int(np.count_nonzero(allowed > cap))
                cells += O.size
    share = wide / cells
    print("%s %s: worst |error| / allowed %.4f, %d cells, %.2f %% of them wider than the cap" % (c.name, what, worst, cells, 100.0 * share))
    assert share < SHARE_CAP, (what, c, "the intervals are too wide to mean anything: %.1f %% of the cells" % (100.0 * share))
    return worst, share, cells
