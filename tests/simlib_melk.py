"""Loader for the wave simulator build of the framed mel specs (tests/wavesim/sim_melk.cpp): clx_mel.hip's framed table builder, its
argument checks, the valid_frames rules and clx_k_mel / clx_k_mel_f as clx_mel_create_framed / clx_mel_windows run them, on host
buffers; the conditioning of the definition (claxon_hip.h) in numpy float32, its float64 reference with the derived bound, and
Kaldi's window and filterbank by their formulas, written independently of claxon_amd's.  The simulator and the GPU tests share it."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib
import simlib_mel
from simlib_mel import CT, LN, LOG10, LOG_ULPS, POWER, TC, g, log_ulps, triangles  # noqa: F401

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_melk.so")


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_melk.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_mel.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: the conditioning's subtract, multiply and divide are each rounded once, as __fsub_rn and its kin are on the GPU
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_melk.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_melk_create.argtypes = [u32, u32, u32, vp, vp, u32, u32, u32, f32, C.c_int, u32, u32, f32]
        _lib.sim_melk_destroy.argtypes = [C.c_int]
        _lib.sim_melk_destroy.restype = None
        _lib.sim_melk_table_words.argtypes = [C.c_int, vp]
        _lib.sim_melk_table_words.restype = sz
        _lib.sim_melk_kernel.argtypes = [C.c_int]
        _lib.sim_melk_windows.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, vp, vp]
        _lib.sim_melk_guarded.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, C.c_int, vp]
        _lib.sim_melk_error.restype = C.c_char_p
        _lib.sim_melk_lds_bytes.restype = u32
    return _lib


def _check(st):
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_melk_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data


def create(n_fft, win_length, hop, window, fbank, n_bins, n_mels, mode, floor, opts=None):
    """clx_mel_create_framed under the simulator: the spec's number.  opts is None (a NULL pointer) or a dict with any of remove_dc,
    whole_frames, preemph (the rest zero)."""
    window = None if window is None else np.ascontiguousarray(window, dtype=np.float32)
    fbank = None if fbank is None else np.ascontiguousarray(fbank, dtype=np.float32)
    o = dict(remove_dc=0, whole_frames=0, preemph=0.0)
    o.update(opts or {})
    h = lib().sim_melk_create(n_fft, win_length, hop, _ptr(window), _ptr(fbank), n_bins, n_mels, mode, floor, 0 if opts is None else 1,
                              o["remove_dc"], o["whole_frames"], o["preemph"])
    if h < 0:
        _check(cx.API_ERROR)
    return h


def destroy(h):
    lib().sim_melk_destroy(h)


def table_words(h):
    """The spec's basis, filterbank and row ends as the builder left them, as one uint32 array."""
    n = lib().sim_melk_table_words(h, None)
    out = np.zeros(n, dtype=np.uint32)
    lib().sim_melk_table_words(h, out.ctypes.data)
    return out


def kernel(h):
    """The kernel clx_mel_windows launches for the spec: "clx_k_mel" or "clx_k_mel_f"."""
    return ("clx_k_mel", "clx_k_mel_f")[lib().sim_melk_kernel(h)]


def mel_windows(h, audio, valid, n_frames, layout, out, shape=None, tables=False):
    """clx_mel_windows under the simulator, `out` written in place.  tables=True: returns (out, valid_frames)."""
    B, L = shape if shape is not None else audio.shape
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    for a in (audio, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.itemsize == 4)
    vf = np.zeros(max(B, 1), np.uint32)
    _check(lib().sim_melk_windows(h, _ptr(audio), B, L, _ptr(valid), n_frames, layout, _ptr(out), vf.ctypes.data))
    return (out, vf[:B]) if tables else out


def mel_guarded(h, audio, valid, n_frames, layout, at_end, out):
    """The batch read from where an inaccessible page follows its last float (at_end) or precedes its first."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    valid = np.ascontiguousarray(valid, dtype=np.uint32)
    _check(lib().sim_melk_guarded(h, a.ctypes.data, a.shape[0], a.shape[1], valid.ctypes.data, n_frames, layout, 1 if at_end else 0,
                                  out.ctypes.data))
    return out


# ---- the definition, independently of the library ---------------------------------------------------------------------------------

def valid_frames(valid, Nw, H, n_frames, whole):
    """whole: 0 for valid < Nw, else min(n_frames, 1 + (valid - Nw) // H); otherwise min(n_frames, ceil(valid / H))."""
    v = np.asarray(valid, dtype=np.int64)
    if not whole:
        return np.minimum((v + H - 1) // H, n_frames)
    return np.where(v < Nw, 0, np.minimum(1 + np.maximum(v - Nw, 0) // H, n_frames))


def frames_of(a, Nw, H, n_frames):
    """[B, n_frames, Nw]: frame t of window k is a[k][t*H + n]."""
    return a[:, np.arange(n_frames)[:, None] * H + np.arange(Nw)[None, :]]


def condition32(x, remove_dc, c):
    """The conditioning in float32, every operation rounded once: x is [.., Nw] float32 whose sums are exact in float32 (the caller
    sees to it: samples on the 2^-15 grid), so that the order of the sum does not matter."""
    x = np.asarray(x, dtype=np.float32)
    Nw = x.shape[-1]
    d = x
    if remove_dc:
        S64 = x.astype(np.float64).sum(axis=-1)
        S = S64.astype(np.float32)
        assert np.array_equal(S.astype(np.float64), S64), "the frame sums are not exact in float32"
        mu = S / np.float32(Nw)
        assert mu.dtype == np.float32
        d = x - mu[..., None]
    if c > 0:
        c = np.float32(c)
        prev = np.concatenate([d[..., :1], d[..., :-1]], axis=-1)
        d = d - c * prev
    assert d.dtype == np.float32
    return np.ascontiguousarray(d)


def basis64(window, N, n_bins):
    """(cos [n_bins, Nw], sin [n_bins, Nw]) in double from the float32 window, the angle over N."""
    Nw = len(window)
    ang = 2.0 * np.pi * ((np.arange(n_bins, dtype=np.int64)[:, None] * np.arange(Nw, dtype=np.int64)[None, :]) % N) / N
    w = np.asarray(window, dtype=np.float64)[None, :]
    return w * np.cos(ang), -w * np.sin(ang)


def reference(audio, window, fbank, N, H, n_frames, remove_dc, c, spectrum=None):
    """(M64, dM), each [B, n_frames, n_mels] in float64: the band sums of the framed definition with the conditioning in exact
    arithmetic on the float32 samples, and the bound that holds for a float32 evaluation in any order (claxon_hip.h).
    spectrum=np.float32 rounds re and im once before they are squared, as an implementation that keeps its transform in complex64
    does (outside_cases.py)."""
    Nw, fb = len(window), np.asarray(fbank, dtype=np.float64)
    X = frames_of(np.asarray(audio, dtype=np.float64), Nw, H, n_frames)              # [B, T, Nw]
    aX = np.abs(X)
    c = float(np.float32(c))
    mu = X.mean(axis=-1, keepdims=True) if remove_dc else np.zeros(X.shape[:-1] + (1,))
    dmu = g(Nw + 1) * aX.mean(axis=-1, keepdims=True) if remove_dc else np.zeros_like(mu)
    d = X - mu
    prev = lambda v: np.concatenate([v[..., :1], v[..., :-1]], axis=-1)
    y = d - c * prev(d)
    dy = (1 + c) * dmu + g(3) * (aX + c * prev(aX) + (1 + c) * (np.abs(mu) + dmu))
    Cb, Sb = basis64(window, N, fb.shape[1])
    re, im = y @ Cb.T, y @ Sb.T
    if spectrum is not None:
        re, im = re.astype(spectrum).astype(np.float64), im.astype(spectrum).astype(np.float64)
    dre = g(Nw + 2) * ((np.abs(y) + dy) @ np.abs(Cb).T) + dy @ np.abs(Cb).T
    dim = g(Nw + 2) * ((np.abs(y) + dy) @ np.abs(Sb).T) + dy @ np.abs(Sb).T
    P = re * re + im * im
    E = 2 * np.abs(re) * dre + dre * dre + 2 * np.abs(im) * dim + dim * dim
    dP = E + g(3) * (P + E)
    nz = fb != 0
    Jm = np.where(nz.any(axis=1), fb.shape[1] - np.argmax(nz[:, ::-1], axis=1) - np.argmax(nz, axis=1), 0)
    M64 = P @ fb.T
    dM = dP @ fb.T + g(Jm + 1)[None, None, :] * ((P + dP) @ fb.T)
    return M64, dM


def kaldi_window(window_type, Nw):
    """The four symmetric windows in float64, point by point."""
    out = np.zeros(Nw, dtype=np.float64)
    for n in range(Nw):
        cosine = np.cos(2.0 * np.pi * n / (Nw - 1)) if Nw > 1 else 1.0
        out[n] = {"povey": lambda: (0.5 - 0.5 * cosine) ** 0.85, "hanning": lambda: 0.5 - 0.5 * cosine,
                  "hamming": lambda: 0.54 - 0.46 * cosine, "rectangular": lambda: 1.0}[window_type]()
    return out


def kaldi_fbank(sample_rate, N, n_mels, low_freq=20.0, high_freq=0.0):
    """[n_mels, N // 2] in float64, cell by cell: triangles that are linear in mel = 1127 ln(1 + f / 700)."""
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    hi = high_freq if high_freq > 0 else 0.5 * sample_rate + high_freq
    mel_lo, mel_hi = mel(low_freq), mel(hi)
    delta = (mel_hi - mel_lo) / (n_mels + 1)
    fb = np.zeros((n_mels, N // 2), dtype=np.float64)
    for b in range(n_mels):
        left = mel_lo + b * delta
        centre = left + delta
        right = centre + delta
        for i in range(N // 2):
            m = mel(i * float(sample_rate) / N)
            if left < m <= centre:
                fb[b, i] = (m - left) / (centre - left)
            elif centre < m < right:
                fb[b, i] = (right - m) / (right - centre)
    return fb
