"""Loader for the wave simulator build of the resampling window reader (tests/wavesim/sim_resample.cpp): clx_resample.hip's argument
checks, table builder and kernel as clx_resample_windows runs them, on host buffers; and the float64 reference of the resampler's
definition (claxon_hip.h), which the simulator and the GPU tests share."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_resample.so")

TC, CT = 0, 1


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_resample.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_resample.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_resample.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.sim_resample_windows.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_size_t, u32, u32, u32, u32, vp]
        _lib.sim_resample_guarded.argtypes = [vp, C.c_int64, u32, C.c_uint64, u32, u32, u32, u32, u32, u32, C.c_int, vp]
        _lib.sim_resample_error.restype = C.c_char_p
        _lib.sim_resample_cached_pairs.restype = C.c_size_t
        _lib.sim_resample_cached_floats.restype = C.c_size_t
    return _lib


def _check(st):
    if st != cx.OK:
        raise cx.ClaxonError(st, 0, lib().sim_resample_error().decode())


_TYPES = (np.uint64, np.int64, np.uint32, np.uint64, np.uint32, np.uint32)


def resample_windows(src, src_first, src_t0, src_n, out_t0, valid, src_rate, out_rate, window_len, channels, layout, out):
    """clx_resample_windows under the simulator: `src` and `out` are host float32 arrays (or None), the per-window arrays are
    sequences (or None), `out` is written in place.  Raises ClaxonError(API_ERROR) with the library's text for what it refuses."""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in zip((src_first, src_t0, src_n, out_t0, valid, src_rate), _TYPES)]
    n = max([a.size for a in arrs if a is not None] or [0])
    for a in (src, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.itemsize == 4)
    _check(lib().sim_resample_windows(None if src is None else src.ctypes.data, *[None if a is None else a.ctypes.data for a in arrs], n,
                                      out_rate, window_len, channels, layout, None if out is None else out.ctypes.data))
    return out


def resample_guarded(data, src_t0, src_n, out_t0, valid, src_rate, out_rate, window_len, channels, layout, at_end, out):
    """One window whose source span `data` (src_n * channels floats) is read from where an inaccessible page follows its last float
    (at_end) or precedes its first: an out-of-bounds load faults."""
    a = np.ascontiguousarray(data, dtype=np.float32)
    assert a.size == src_n * channels
    _check(lib().sim_resample_guarded(a.ctypes.data, src_t0, src_n, out_t0, valid, src_rate, out_rate, window_len, channels, layout,
                                      1 if at_end else 0, out.ctypes.data))
    return out


# ---- the reference: the definition in float64 ---------------------------------------------------------------------------------------

U = 2.0 ** -24


def pair(fs, R):
    """(o, n, W) of fs -> R."""
    g = math.gcd(fs, R)
    o, n = fs // g, R // g
    return o, n, int(math.ceil(6 * o / (min(o, n) * 0.99)))


def length_at(T, fs, R):
    o, n, _ = pair(fs, R)
    return -(-T * n // o)


def span(m0, m1, T, fs, R):
    """The source samples [lo, hi) that outputs m0 .. m1 reach."""
    o, n, W = pair(fs, R)
    return max(0, m0 * o // n - W + 1), min(T, m1 * o // n + W + 1)


def reference(x, fs, R, m, t0=0):
    """y64[m, c] and the tolerance's sum of |h_k x_k| for outputs `m` (an int array) of x [T, C] (float32, taken as float64) resampled
    from fs to R: every one of the 2W taps evaluated from the formula, x = 0 outside 0 <= s < T.  With t0, row 0 of x is stream
    sample t0 (x = 0 outside t0 <= s < t0 + T): a piece of a stream far from its start, without the zeros in front of it.  The
    positions are whole numbers throughout (int64: m * o is checked to fit), only the tap's distance s - m o / n becomes a double."""
    o, n, W = pair(fs, R)
    base = min(o, n) * 0.99
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    m = np.asarray(m, dtype=np.int64)
    assert m.size == 0 or (int(np.abs(m).max()) + 1) * o + 2 * W < 1 << 63, "m * o does not fit int64"
    fc = m * o // n
    s = fc[:, None] - W + 1 + np.arange(2 * W)[None, :]                          # [M, 2W]
    d = (s - fc[:, None]).astype(np.float64) - ((m * o) % n).astype(np.float64)[:, None] / n      # s - m o / n: the whole part in integers
    t = d * base / o
    h = np.where(np.abs(t) < 6.0, np.sinc(t) * np.cos(np.pi * t / 12.0) ** 2 * base / o, 0.0)
    s = s - int(t0)                                                              # (from here on: rows of x)
    inside = (s >= 0) & (s < T)
    xs = np.where(inside[:, :, None], x[np.clip(s, 0, max(T - 1, 0))], 0.0)      # [M, 2W, C]
    terms = h[:, :, None] * xs
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def bound(fs, R):
    """gamma of the N-term float32 dot product, N = 2W + 2."""
    N = 2 * pair(fs, R)[2] + 2
    return N * U / (1.0 - N * U)


def assert_close(got, x, fs, R, m, what="", t0=0):
    """got [M, C] (float32) against the reference for outputs m: |y - y64| <= gamma * sum |h_k x_k|, exactly 0 where no tap is.
    Returns the worst |error| / bound."""
    y, mag = reference(x, fs, R, m, t0)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == y.shape, (got.shape, y.shape, what)
    err, tol = np.abs(got - y), bound(fs, R) * mag
    bad = np.argwhere(err > tol)
    assert bad.size == 0, (what, "output %d channel %d: %r, expected %r, |error| %.3g > %.3g" % (
        int(m[bad[0][0]]), bad[0][1], got[tuple(bad[0])], y[tuple(bad[0])], err[tuple(bad[0])], tol[tuple(bad[0])]))
    worst = float(np.max(err / np.where(tol > 0, tol, 1.0))) if err.size else 0.0
    return worst
