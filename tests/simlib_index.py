"""Loader for the wave simulator build of the segmented frame indexer (tests/wavesim/sim_index.cpp): clx_index.hip's kernels and host
steps as clx_index_streams_device runs them, on host buffers."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_index.so")


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_index.cpp", "wavesim.h")] + \
           [os.path.join(simlib._CSRC, f) for f in ("clx_index.hip", "clx_kernels.hip", "clx_device.h", "clx_crct.h")] + \
           [os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_index.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, sz = C.c_void_p, C.c_size_t
        for f in (_lib.sim_index_streams, _lib.sim_index_guarded):
            f.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, sz, vp, vp, C.POINTER(sz), vp]
        _lib.sim_index_error.restype = C.c_char_p
    return _lib


def aligned(arena, pad=32):
    """A 16-byte aligned copy of `arena` (uint8) with round16(size) + `pad` readable bytes, the padding filled with 0xff."""
    n = arena.size
    buf = np.full(((n + 15) // 16) * 16 + pad + 16, 0xff, dtype=np.uint8)
    base = (-buf.ctypes.data) % 16
    al = buf[base:base + ((n + 15) // 16) * 16 + pad]
    al[:n] = arena
    return al


def index_streams_raw(arena_ptr, arena_len, offs, lens, starts, n, descs_ptr, hdrs_ptr, cap, first_ptr, stops_ptr, guarded=False, null_found=False):
    """The C entry as it is (pointers may be None; null_found: n_found itself is NULL): (status, n_found, error text)."""
    found = C.c_size_t(0)
    parse = C.cast(cx.lib().clx_parse_frame_header, C.c_void_p)
    f = lib().sim_index_guarded if guarded else lib().sim_index_streams
    st = f(arena_ptr, arena_len, offs, lens, starts, n, descs_ptr, hdrs_ptr, cap, first_ptr, stops_ptr, None if null_found else C.byref(found), parse)
    return st, int(found.value), lib().sim_index_error().decode() if st != cx.OK else ""


def index_streams(arena, offs, lens, starts=None, cap=None, guarded=False):
    """Context.index_streams under the simulator: (descs, headers, first_frame, stop_offs); `cap` None grows as the binding does.
    Raises ClaxonError(API_ERROR) with the library's text."""
    a = np.ascontiguousarray(arena, dtype=np.uint8)
    al = a if guarded else aligned(a)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    starts = None if starts is None else np.ascontiguousarray(starts, dtype=np.uint64)
    n = offs.size
    first = np.zeros(n + 1, dtype=np.uint64)
    stops = np.zeros(n, dtype=np.uint64)
    grow = cap is None
    cap = int(lens.sum()) // 512 + 4 * n + 64 if grow else int(cap)
    while True:
        descs = np.zeros(max(cap, 1), dtype=cx.FRAME_DESC_DTYPE)
        hdrs = np.zeros(max(cap, 1), dtype=cx.FRAME_HEADER_DTYPE)
        st, found, err = index_streams_raw(al.ctypes.data, a.size, offs.ctypes.data, lens.ctypes.data,
                                           None if starts is None else starts.ctypes.data, n, descs.ctypes.data, hdrs.ctypes.data, cap,
                                           first.ctypes.data, stops.ctypes.data, guarded)
        if st == cx.API_ERROR and found > cap and grow:
            cap = found
            continue
        if st != cx.OK:
            e = cx.ClaxonError(st, 0, err)
            e.n_found = found
            raise e
        return descs[:found].copy(), hdrs[:found].copy(), first, stops
