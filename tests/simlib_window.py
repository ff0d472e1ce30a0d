"""Loader for the wave simulator build of the window gather (tests/wavesim/sim_window.cpp): clx_window.hip's argument checks and
kernel as clx_gather_windows runs them, on host buffers."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_window.so")

TC, CT = 0, 1


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_window.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_window.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_window.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.sim_gather_windows.argtypes = [vp, vp, vp, C.c_size_t, u32, u32, u32, vp]
        _lib.sim_window_guarded.argtypes = [vp, u32, u32, u32, u32, C.c_int, vp]
        _lib.sim_window_error.restype = C.c_char_p
    return _lib


def _check(st):
    if st != cx.OK:
        raise cx.ClaxonError(st, 0, lib().sim_window_error().decode())


def gather_windows(src, src_first, valid, window_len, channels, layout, out):
    """clx_gather_windows under the simulator: `src` and `out` are host uint32 / float32 arrays (or None), `out` is written in place.
    Raises ClaxonError(API_ERROR) with the library's text for the combinations it refuses."""
    src_first = None if src_first is None else np.ascontiguousarray(src_first, dtype=np.uint64)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    n = src_first.size if src_first is not None else valid.size if valid is not None else 0
    for a in (src, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.itemsize == 4)
    _check(lib().sim_gather_windows(None if src is None else src.ctypes.data, None if src_first is None else src_first.ctypes.data,
                                    None if valid is None else valid.ctypes.data, n, window_len, channels, layout,
                                    None if out is None else out.ctypes.data))
    return out


def window_guarded(data, valid, window_len, channels, layout, at_end, out):
    """One window of valid * channels words `data` gathered from where an inaccessible page follows its last word (at_end) or
    precedes its first: an out-of-bounds load faults."""
    a = np.ascontiguousarray(data, dtype=np.uint32)
    assert a.size == valid * channels
    _check(lib().sim_window_guarded(a.ctypes.data, valid, window_len, channels, layout, 1 if at_end else 0, out.ctypes.data))
    return out
