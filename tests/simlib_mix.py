"""Loader for the wave simulator build of the channel-mixing window reader (tests/wavesim/sim_mix.cpp): clx_mix.hip's argument checks
and kernel as clx_mix_windows runs them, on host buffers; and the mix's definition (claxon_hip.h) evaluated with numpy float32
scalars in the stated order, which the simulator and the GPU tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_mix.so")

TC, CT = 0, 1


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_mix.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_mix.hip"),
            os.path.join(simlib._CSRC, "clx_resample.hip"), os.path.join(_DIR, "fake", "hip", "hip_runtime.h"),
            os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_mix.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.sim_mix_windows.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, u32, u32, u32, u32, vp]
        _lib.sim_mix_resample_windows.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_size_t, u32, u32, u32, u32, vp]
        _lib.sim_mix_guarded.argtypes = [vp, C.c_int64, u32, C.c_uint64, u32, u32, u32, u32, u32, u32, u32, C.c_int, vp]
        _lib.sim_mix_error.restype = C.c_char_p
        _lib.sim_mix_cached_pairs.restype = C.c_size_t
        _lib.sim_mix_cached_floats.restype = C.c_size_t
    return _lib


def _check(st):
    if st != cx.OK:
        raise cx.ClaxonError(st, 0, lib().sim_mix_error().decode())


_TYPES = (np.uint64, np.int64, np.uint32, np.uint64, np.uint32, np.uint32, np.uint8)


def _call(fn, src, arrs, types, tail, out):
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in zip(arrs, types)]
    n = max([a.size for a in arrs if a is not None] or [0])
    for a in (src, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.itemsize == 4)
    _check(fn(None if src is None else src.ctypes.data, *[None if a is None else a.ctypes.data for a in arrs], n, *tail,
              None if out is None else out.ctypes.data))
    return out


def mix_windows(src, src_first, src_t0, src_n, out_t0, valid, src_rate, src_channels, out_rate, window_len, out_channels, layout, out):
    """clx_mix_windows under the simulator: `src` and `out` are host float32 / uint32 arrays (or None), the per-window arrays are
    sequences (or None), `out` is written in place.  Raises ClaxonError(API_ERROR) with the library's text for what it refuses."""
    return _call(lib().sim_mix_windows, src, (src_first, src_t0, src_n, out_t0, valid, src_rate, src_channels), _TYPES,
                 (out_rate, window_len, out_channels, layout), out)


def resample_windows(src, src_first, src_t0, src_n, out_t0, valid, src_rate, out_rate, window_len, channels, layout, out):
    """clx_resample_windows on the coefficient cache that mix_windows uses."""
    return _call(lib().sim_mix_resample_windows, src, (src_first, src_t0, src_n, out_t0, valid, src_rate), _TYPES[:6],
                 (out_rate, window_len, channels, layout), out)


def mix_guarded(data, src_t0, src_n, out_t0, valid, src_rate, src_channels, out_rate, window_len, out_channels, layout, at_end, out):
    """One window whose source span `data` (src_n * src_channels floats) is read from where an inaccessible page follows its last
    float (at_end) or precedes its first: an out-of-bounds load faults."""
    a = np.ascontiguousarray(data, dtype=np.float32)
    assert a.size == src_n * src_channels
    _check(lib().sim_mix_guarded(a.ctypes.data, src_t0, src_n, out_t0, valid, src_rate, src_channels, out_rate, window_len, out_channels,
                                 layout, 1 if at_end else 0, out.ctypes.data))
    return out


def mix(x, K):
    """x [T, Cs] (float32) brought to K channels by the definition: [T, K] float32.  The reduce adds the channels in ascending order,
    each add a float32 add, then multiplies by the float32 nearest to 1 / Cs."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    Cs = x.shape[1]
    if Cs == K:
        return x
    if Cs == 1:
        return np.repeat(x, K, axis=1)
    assert K == 1, (Cs, K)
    with np.errstate(invalid="ignore", over="ignore"):
        s = x[:, 0].copy()
        for c in range(1, Cs):
            s = s + x[:, c]                                  # (float32 + float32: one rounding)
        s = s * np.float32(1.0 / Cs)                         # (1 / Cs in double, rounded once: the float32 nearest to it)
    assert s.dtype == np.float32
    return s.reshape(-1, 1)
