"""Loader for the wave simulator build of the stream MD5 (tests/wavesim/sim_md5.cpp): clx_md5.hip's plan and kernel as
clx_md5_streams runs them, on host buffers."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_md5.so")


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_md5.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_md5.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_md5.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp = C.c_void_p
        _lib.sim_md5_streams.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_size_t, vp]
        _lib.sim_md5_guarded.argtypes = [vp, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint8, C.c_int, vp]
        _lib.sim_md5_error.restype = C.c_char_p
    return _lib


def md5_streams(samples, sample_format, first, counts, bps):
    """Context.md5_streams under the simulator: `samples` a host array (any dtype, read as bytes); uint8 [n, 16] digests.  Raises
    ClaxonError(API_ERROR) with the library's text for the combinations it refuses."""
    buf = np.ascontiguousarray(samples).view(np.uint8).reshape(-1) if samples is not None else None
    first = np.ascontiguousarray(first, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    bps = np.ascontiguousarray(bps, dtype=np.uint8)
    assert first.size == counts.size == bps.size
    out = np.zeros((first.size, 16), dtype=np.uint8)
    st = lib().sim_md5_streams(buf.ctypes.data if buf is not None else None, sample_format, first.ctypes.data, counts.ctypes.data,
                               bps.ctypes.data, first.size, out.ctypes.data)
    if st != cx.OK:
        raise cx.ClaxonError(st, 0, lib().sim_md5_error().decode())
    return out


def md5_guarded(data, sample_format, n, bps, at_end):
    """One stream of bytes `data` hashed where an inaccessible page follows (at_end) or precedes it: an out-of-bounds load faults."""
    a = np.ascontiguousarray(data, dtype=np.uint8)
    out = np.zeros(16, dtype=np.uint8)
    st = lib().sim_md5_guarded(a.ctypes.data, a.size, sample_format, n, bps, 1 if at_end else 0, out.ctypes.data)
    if st != cx.OK:
        raise cx.ClaxonError(st, 0, lib().sim_md5_error().decode())
    return out
