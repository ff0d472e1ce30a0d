"""Loader for the wave simulator build of the cepstral mel specs (tests/wavesim/sim_melq.cpp): clx_mel.hip's cepstral table builder, its
argument checks and clx_k_mel_q as clx_mel_create_cepstral / clx_mel_windows run them, on host buffers; the definition's cepstrum as
one chain of the host libm's fmaf, its energy in the stated lane order, Kaldi's DCT and lifter by their formulas, written
independently of claxon_amd's, and the float64 interval of the MFCC formula.  The simulator and the GPU tests share it."""
import ctypes as C
import ctypes.util
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib
import simlib_melk as sk
from simlib_mel import CT, LN, LOG10, LOG_ULPS, POWER, TC, g  # noqa: F401

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_melq.so")
FLT_EPSILON = float(np.finfo(np.float32).eps)


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_melq.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_mel.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: the conditioning's steps, the energy's folds and the lifter product are each rounded once, as on the GPU
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_melq.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_melq_create.argtypes = [u32, u32, u32, vp, vp, u32, u32, u32, f32, C.c_int, u32, u32, f32, C.c_int, u32, vp, vp, u32, f32, f32]
        _lib.sim_melq_destroy.argtypes = [C.c_int]
        _lib.sim_melq_destroy.restype = None
        _lib.sim_melq_kernel.argtypes = [C.c_int]
        _lib.sim_melq_rows.argtypes = [C.c_int]
        _lib.sim_melq_rows.restype = u32
        _lib.sim_melq_logf.argtypes = [f32]
        _lib.sim_melq_logf.restype = f32
        _lib.sim_melq_windows.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, vp, vp]
        _lib.sim_melq_guarded.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, C.c_int, vp]
        _lib.sim_melq_error.restype = C.c_char_p
        _lib.sim_melq_lds_bytes.restype = u32
    return _lib


def _check(st):
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_melq_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data


FRAMED = "framed"


def create(n_fft, win_length, hop, window, fbank, n_bins, n_mels, mode, floor, opts=None, cep=None):
    """clx_mel_create_cepstral under the simulator: the spec's number.  opts is None (a NULL pointer) or a dict with any of
    remove_dc, whole_frames, preemph (the rest zero).  cep is None (a NULL pointer), a dict with any of n_ceps, dct, lifter, energy,
    energy_scale, energy_floor (the rest: n_ceps 1, no table, 0, 1.0, 0.0), or FRAMED: clx_mel_create_framed with the same tables."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    window, fbank = f32(window), f32(fbank)
    o = dict(remove_dc=0, whole_frames=0, preemph=0.0)
    o.update(opts or {})
    q = dict(n_ceps=1, dct=None, lifter=None, energy=0, energy_scale=1.0, energy_floor=0.0)
    q.update(cep if isinstance(cep, dict) else {})
    dct, lifter = f32(q["dct"]), f32(q["lifter"])
    h = lib().sim_melq_create(n_fft, win_length, hop, _ptr(window), _ptr(fbank), n_bins, n_mels, mode, floor, 0 if opts is None else 1,
                              o["remove_dc"], o["whole_frames"], o["preemph"], -1 if cep == FRAMED else 0 if cep is None else 1,
                              q["n_ceps"], _ptr(dct), _ptr(lifter), q["energy"], q["energy_scale"], q["energy_floor"])
    if h < 0:
        _check(cx.API_ERROR)
    return h


def destroy(h):
    lib().sim_melq_destroy(h)


def kernel(h):
    """The kernel clx_mel_windows launches for the spec."""
    return ("clx_k_mel", "clx_k_mel_f", "clx_k_mel_q")[lib().sim_melq_kernel(h)]


def rows(h):
    """The rows of the spec's output: n_ceps of a cepstral spec, else n_mels."""
    return int(lib().sim_melq_rows(h))


def logf(x):
    """logf as the simulator's libm computes it."""
    return np.float32(lib().sim_melq_logf(float(np.float32(x))))


def mel_windows(h, audio, valid, n_frames, layout, out, shape=None, tables=False):
    """clx_mel_windows under the simulator, `out` written in place.  tables=True: returns (out, valid_frames)."""
    B, L = shape if shape is not None else audio.shape
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    for a in (audio, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.itemsize == 4)
    vf = np.zeros(max(B, 1), np.uint32)
    _check(lib().sim_melq_windows(h, _ptr(audio), B, L, _ptr(valid), n_frames, layout, _ptr(out), vf.ctypes.data))
    return (out, vf[:B]) if tables else out


def mel_guarded(h, audio, valid, n_frames, layout, at_end, out):
    """The batch read from where an inaccessible page follows its last float (at_end) or precedes its first."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    valid = np.ascontiguousarray(valid, dtype=np.uint32)
    _check(lib().sim_melq_guarded(h, a.ctypes.data, a.shape[0], a.shape[1], valid.ctypes.data, n_frames, layout, 1 if at_end else 0,
                                  out.ctypes.data))
    return out


# ---- the definition, independently of the library ---------------------------------------------------------------------------------

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
_libm.fmaf.restype = C.c_float
_fmaf = _libm.fmaf


def dct_kaldi(n_ceps, n_mels):
    """Kaldi's ComputeDctMatrix, cell by cell in float64: the first n_ceps rows of the orthonormal DCT-II."""
    d = np.zeros((n_ceps, n_mels), dtype=np.float64)
    for k in range(n_ceps):
        for m in range(n_mels):
            d[k, m] = np.sqrt(1.0 / n_mels) if k == 0 else np.sqrt(2.0 / n_mels) * np.cos(np.pi / n_mels * (m + 0.5) * k)
    return d


def lifter_kaldi(n_ceps, Q=22.0):
    """1 + 0.5 Q sin(pi i / Q), point by point in float64."""
    return np.array([1.0 + 0.5 * Q * np.sin(np.pi * i / Q) for i in range(n_ceps)], dtype=np.float64)


def chain(dct, Y, lifter=None):
    """C[.., i] = sum_m dct[i][m] Y[.., m] as one chain of libm's fmaf, m ascending, from +0.0, for Y [.., n_mels] float32; then the
    lifter product in numpy float32.  [.., n_ceps] float32."""
    dct = np.ascontiguousarray(dct, dtype=np.float32)
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    flat = Y.reshape(-1, Y.shape[-1]).tolist()
    rows_ = dct.tolist()
    out = np.zeros((len(flat), len(rows_)), dtype=np.float32)
    for r, y in enumerate(flat):
        for i, d in enumerate(rows_):
            acc = 0.0
            for dm, ym in zip(d, y):
                acc = _fmaf(dm, ym, acc)
            out[r, i] = acc
    if lifter is not None:
        out = out * np.ascontiguousarray(lifter, dtype=np.float32)[None, :]
        assert out.dtype == np.float32
    return out.reshape(Y.shape[:-1] + (len(rows_),))


def energy32(X, remove_dc, energy_scale):
    """E of the definition for the frames X [.., Nw] float32, in the kernel's order: the mean as clx_k_mel_f sums it (8 partial sums
    over n = i, i+8, .. ascending, folded 4, 2, 1, one division), d = fl32(x - mu), e_i by libm's fmaf over n = i, i+8, ..,
    e = ((e0 + e4) + (e2 + e6)) + ((e1 + e5) + (e3 + e7)) in numpy float32, E = fl32(e * energy_scale).  [..] float32."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    Nw = X.shape[-1]
    flat = X.reshape(-1, Nw)
    out = np.zeros(flat.shape[0], dtype=np.float32)
    f32 = np.float32

    def fold(p):
        a = [f32(p[i] + p[i ^ 4]) for i in range(8)]
        b = [f32(a[i] + a[i ^ 2]) for i in range(8)]
        return f32(b[0] + b[1])

    for r in range(flat.shape[0]):
        x = flat[r]
        d = x
        if remove_dc:
            part = []
            for i in range(8):
                s = f32(0.0)
                for v in x[i::8]:
                    s = f32(s + v)
                part.append(s)
            mu = f32(fold(part) / f32(Nw))
            d = (x - mu).astype(np.float32)
        part = []
        for i in range(8):
            e = 0.0
            for v in d[i::8].tolist():
                e = _fmaf(v, v, e)
            part.append(f32(e))
        out[r] = f32(fold(part) * f32(energy_scale))
    return out.reshape(X.shape[:-1])


def log_energy64(E, energy_floor=0.0):
    """log(max(E, FLT_EPSILON)) in float64, raised to log(energy_floor) where that is larger."""
    le = np.log(np.maximum(np.asarray(E, dtype=np.float64), FLT_EPSILON))
    return np.maximum(le, np.log(energy_floor)) if energy_floor > 0 else le


def ulps_of(got, ref64):
    """|got - ref64| in float32 ulps of ref64."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


def _ulp(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def reference(audio, window, fbank, N, H, n_frames, remove_dc, c, floor, dct, lifter=None):
    """(C64, dC), each [B, n_frames, n_ceps] in float64: Kaldi's MFCC formula (mode ln) in exact arithmetic on the float32 samples
    and the half-width of the interval a float32 evaluation in any order lies in (claxon_hip.h): simlib_melk.reference's M64 +- dM
    through the logarithm, which is monotone, widened by LOG_ULPS ulps: Y64 +- dY; dC = sum_m |dct[i][m]| dY_m +
    g(n_mels + 1) sum_m |dct[i][m]| (|Y64_m| + dY_m) (the kernel's own |Y_m| is at most that); with a lifter both times |lifter[i]|
    and one float32 ulp of the larger end more."""
    M64, dM = sk.reference(audio, window, fbank, N, H, n_frames, remove_dc, c)
    Y64 = np.log(np.maximum(M64, floor))
    lo, hi = np.log(np.maximum(M64 - dM, floor)), np.log(np.maximum(M64 + dM, floor))
    lo, hi = lo - LOG_ULPS * _ulp(lo), hi + LOG_ULPS * _ulp(hi)
    dY = np.maximum(hi - Y64, Y64 - lo)
    D = np.asarray(np.asarray(dct, dtype=np.float32), dtype=np.float64)
    n_mels = D.shape[1]
    C64 = Y64 @ D.T
    dC = dY @ np.abs(D).T + g(n_mels + 1) * ((np.abs(Y64) + dY) @ np.abs(D).T)
    if lifter is not None:
        l = np.asarray(np.asarray(lifter, dtype=np.float32), dtype=np.float64)
        C64, dC = C64 * l[None, None, :], dC * np.abs(l)[None, None, :]
        dC = dC + _ulp(np.abs(C64) + dC)
    return C64, dC


def reference_power(audio, window, fbank, N, H, n_frames, remove_dc, c, dct, lifter=None):
    """(C64, dC), each [B, n_frames, n_ceps] in float64, for a cepstral spec in power mode, where the cells that enter the DCT are
    the band sums themselves: with (M64, dM) from simlib_melk.reference and D the float32 DCT, C64 = M64 @ D.T.  The kernel's cell
    Y_m is a float32 with |Y_m - M64_m| <= dM_m, and its chain of n_mels fmaf from +0.0 adds at most g(n_mels) sum_m |D[i][m]| |Y_m|
    in any order, so dC = dM @ |D|.T + g(n_mels + 1) ((M64 + dM) @ |D|.T) (M64 >= 0).  With a lifter both times |lifter[i]|, and one
    float32 ulp of the larger end for the product's one rounding."""
    M64, dM = sk.reference(audio, window, fbank, N, H, n_frames, remove_dc, c)
    D = np.asarray(np.asarray(dct, dtype=np.float32), dtype=np.float64)
    n_mels = D.shape[1]
    C64 = M64 @ D.T
    dC = dM @ np.abs(D).T + g(n_mels + 1) * ((M64 + dM) @ np.abs(D).T)
    if lifter is not None:
        l = np.asarray(np.asarray(lifter, dtype=np.float32), dtype=np.float64)
        C64, dC = C64 * l[None, None, :], dC * np.abs(l)[None, None, :]
        dC = dC + _ulp(np.abs(C64) + dC)
    return C64, dC
