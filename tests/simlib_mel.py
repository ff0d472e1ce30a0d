"""Loader for the wave simulator build of the mel feature kernel (tests/wavesim/sim_mel.cpp): clx_mel.hip's table builder, argument
checks and kernel as clx_mel_create / clx_mel_windows run them, on host buffers; and the float64 reference of the definition
(claxon_hip.h) with its derived error bound, which the simulator and the GPU tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_mel.so")

TC, CT = 0, 1
POWER, LN, LOG10 = 0, 1, 2
MODES = {"power": POWER, "ln": LN, "log10": LOG10}

# The log step's allowance, in units in the last place of the float32 result, against float64 log(max(float64(M), floor)): twice
# the worst error seen over the tests' own values, and at least 2.  Worst seen under the simulator (the host's libm; printed by
# test_mel_sim.py::test_the_log_step_and_its_ulps): logf 0.689 ulp, log10f 1.666 ulp.  Worst seen on an MI355X (printed by
# test_gpu_mel.py::test_mel_windows_on_native_audio): logf 2.061 ulp, log10f 2.123 ulp.  Twice the worst of the four.
LOG_ULPS = 4.25


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_mel.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_mel.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_mel.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        _lib.sim_mel_create.argtypes = [u32, u32, vp, vp, u32, u32, C.c_float]
        _lib.sim_mel_destroy.argtypes = [C.c_int]
        _lib.sim_mel_destroy.restype = None
        _lib.sim_mel_tables.argtypes = [C.c_int, vp, vp, vp]
        _lib.sim_mel_windows.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, vp]
        _lib.sim_mel_guarded.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, C.c_int, vp]
        _lib.sim_mel_finish.argtypes = [u32, C.c_float, vp, sz, vp]
        _lib.sim_mel_finish.restype = None
        _lib.sim_mel_error.restype = C.c_char_p
        _lib.sim_mel_lds_bytes.restype = u32
        _lib.sim_mel_group_frames.restype = u32
    return _lib


def _check(st):
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_mel_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data


def create(n_fft, hop, window, fbank, n_mels, mode, floor):
    """clx_mel_create under the simulator: the spec's number.  `window` and `fbank` are float32 arrays or None."""
    window = None if window is None else np.ascontiguousarray(window, dtype=np.float32)
    fbank = None if fbank is None else np.ascontiguousarray(fbank, dtype=np.float32)
    h = lib().sim_mel_create(n_fft, hop, _ptr(window), _ptr(fbank), n_mels, mode, floor)
    if h < 0:
        _check(cx.API_ERROR)
    return h


def destroy(h):
    lib().sim_mel_destroy(h)


def tables(h, n_fft, n_mels):
    """The library's basis, dense: (cos [J, N], sin [J, N], ends [n_mels, 2]); asserts that the padding of its table is zeros."""
    J = n_fft // 2 + 1
    c, s, e = np.zeros((J, n_fft), np.float32), np.zeros((J, n_fft), np.float32), np.zeros((n_mels, 2), np.uint32)
    st = lib().sim_mel_tables(h, c.ctypes.data, s.ctypes.data, e.ctypes.data)
    assert st == 0, "the basis table's padding is not all zeros" if st == 1 else "no such spec"
    return c, s, e


def mel_windows(h, audio, valid, n_frames, layout, out, shape=None):
    """clx_mel_windows under the simulator: `audio` [B, L] and `out` are host float32 / uint32 arrays (or None, with shape=(B, L)),
    `out` is written in place.  Raises ClaxonError(API_ERROR) with the library's text for what it refuses."""
    B, L = shape if shape is not None else audio.shape
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    for a in (audio, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.itemsize == 4)
    _check(lib().sim_mel_windows(h, _ptr(audio), B, L, _ptr(valid), n_frames, layout, _ptr(out)))
    return out


def mel_guarded(h, audio, valid, n_frames, layout, at_end, out):
    """The batch read from where an inaccessible page follows its last float (at_end) or precedes its first."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    valid = np.ascontiguousarray(valid, dtype=np.uint32)
    _check(lib().sim_mel_guarded(h, a.ctypes.data, a.shape[0], a.shape[1], valid.ctypes.data, n_frames, layout, 1 if at_end else 0,
                                 out.ctypes.data))
    return out


def finish(mode, floor, m):
    """The kernel's last step (the simulator's logf / log10f) on the float32 values m."""
    m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
    out = np.zeros_like(m)
    lib().sim_mel_finish(mode, floor, m.ctypes.data, m.size, out.ctypes.data)
    return out


# ---- the tables, built independently of claxon_amd's ------------------------------------------------------------------------------

def hann(N):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)


def mel_points(sample_rate, n_mels, f_min=0.0, f_max=None, scale="htk"):
    """The n_mels + 2 corner frequencies in Hz."""
    f_max = sample_rate / 2.0 if f_max is None else f_max
    if scale == "htk":
        to_mel, to_hz = (lambda f: 2595.0 * np.log10(1.0 + f / 700.0)), (lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0))
    else:
        step = np.log(6.4) / 27.0
        to_mel = lambda f: 3.0 * f / 200.0 if f < 1000.0 else 15.0 + np.log(f / 1000.0) / step
        to_hz = lambda m: np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp(step * (np.maximum(m, 15.0) - 15.0)))
    return to_hz(np.linspace(to_mel(float(f_min)), to_mel(float(f_max)), n_mels + 2))


def triangles(sample_rate, N, n_mels, f_min=0.0, f_max=None, scale="htk", slaney_norm=False):
    """[n_mels, J] float32: band m rises over [pts[m], pts[m+1]] and falls over [pts[m+1], pts[m+2]] (a loop over the bands)."""
    pts = mel_points(sample_rate, n_mels, f_min, f_max, scale)
    freqs = np.arange(N // 2 + 1, dtype=np.float64) * (float(sample_rate) / N)
    fb = np.zeros((n_mels, freqs.size), dtype=np.float64)
    for m in range(n_mels):
        lo, mid, hi = pts[m], pts[m + 1], pts[m + 2]
        up, down = (freqs - lo) / (mid - lo), (hi - freqs) / (hi - mid)
        fb[m] = np.maximum(0.0, np.minimum(up, down))
        if slaney_norm:
            fb[m] = fb[m] * (2.0 / (hi - lo))
    return fb.astype(np.float32)


# ---- the reference: the definition in float64, and the bound ----------------------------------------------------------------------

U = 2.0 ** -24


def g(k):
    return k * U / (1.0 - k * U)


def basis64(window, N):
    """(cos [J, N], sin [J, N]) in double from the float32 window: w[n] cos(2 pi ((j n) mod N) / N) and -w[n] sin(..)."""
    J = N // 2 + 1
    ang = 2.0 * np.pi * ((np.arange(J, dtype=np.int64)[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N) / N
    w = np.asarray(window, dtype=np.float64)[None, :]
    return w * np.cos(ang), -w * np.sin(ang)


def reference(audio, window, fbank, N, H, n_frames, spectrum=None):
    """(M64, dM), each [B, n_frames, n_mels] in float64, for audio [B, L] (float32, taken as float64): the band sums of the
    definition and the bound that holds for a float32 evaluation in any order (claxon_hip.h).  spectrum=np.float32 rounds re and im
    once before they are squared, as an implementation that keeps its transform in complex64 does (outside_cases.py)."""
    a = np.asarray(audio, dtype=np.float64)
    fb = np.asarray(fbank, dtype=np.float64)
    idx = np.arange(n_frames)[:, None] * H + np.arange(N)[None, :]
    X = a[:, idx]                                            # [B, T, N]
    Cb, Sb = basis64(window, N)
    re, im = X @ Cb.T, X @ Sb.T                              # [B, T, J]
    if spectrum is not None:
        re, im = re.astype(spectrum).astype(np.float64), im.astype(spectrum).astype(np.float64)
    A, Bm = np.abs(X) @ np.abs(Cb).T, np.abs(X) @ np.abs(Sb).T
    P = re * re + im * im
    dre, dim = g(N + 2) * A, g(N + 2) * Bm
    E = 2 * np.abs(re) * dre + dre * dre + 2 * np.abs(im) * dim + dim * dim
    dP = E + g(3) * (P + E)
    nz = fb != 0
    Jm = np.where(nz.any(axis=1), fb.shape[1] - np.argmax(nz[:, ::-1], axis=1) - np.argmax(nz, axis=1), 0)     # first .. last non-zero bin
    M64 = P @ fb.T
    dM = dP @ fb.T + g(Jm + 1)[None, None, :] * ((P + dP) @ fb.T)
    return M64, dM


def valid_frames(valid, H, n_frames):
    return np.minimum((np.asarray(valid, dtype=np.int64) + H - 1) // H, n_frames)


def log_ulps(got, m, mode, floor):
    """The error of the float32 log-mode outputs `got` against float64 log(max(float64(m), floor)), in ulps of the result."""
    x = np.maximum(np.asarray(m, dtype=np.float64), float(floor))
    ref = np.log(x) if mode == LN else np.log10(x)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / ulp
