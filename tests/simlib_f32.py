"""Loader for the wave simulator build of the float output (tests/wavesim/sim_f32.cpp): the lane path's kernels as the library
launches them for a CLX_OUT_F32 batch."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_f32.so")


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_f32.cpp", "sim_lib.cpp", "wavesim.h")] + \
           [os.path.join(simlib._CSRC, f) for f in ("clx_kernels.hip", "clx_lanes.hip", "clx_lean.hip", "clx_device.h", "clx_crct.h", "clx_plan.h")] + \
           [os.path.join(_DIR, "fake", "clx_intrin.h"), os.path.join(_DIR, "fake", "clx_k2_dot2.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_f32.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        _lib.sim_decode_frames_f32.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_uint32, C.c_void_p]
        _lib.sim_general_sure.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32]
        _lib.sim_general_sure.restype = C.c_uint64
    return _lib


def _aligned(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    buf = np.zeros(a.size + 64, dtype=np.uint8)          # (16-byte aligned base, padded allocation: as the GPU reads it)
    base = (-buf.ctypes.data) % 16
    al = buf[base:base + a.size]
    al[:] = a
    return buf, al


def _out_buffer(total, fill):
    """A float output of `total` samples on 256 bytes, as a device allocation is (the tiers take blocks that start on 32 bytes)."""
    buf = np.full(total + 72, fill, dtype=np.float32)
    k = ((-buf.ctypes.data) % 256) // 4
    return buf[k:k + total]


def decode_runs(arenas, arena_len, descs, out_offs, verify_crc=False, fill=np.nan, path=0):
    """Consecutive runs of ONE planned CLX_OUT_F32 batch on one set of scratch.  Returns ([(out float32, results), ...], tier_groups):
    tier_groups = (groups the 16-bit tier took, groups both tiers took), summed over the runs."""
    descs = np.ascontiguousarray(descs, dtype=cx.FRAME_DESC_DTYPE)
    out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
    n = descs.size
    total = int((out_offs + descs["n_channels"].astype(np.uint64) * descs["block_size"].astype(np.uint64)).max()) if n else 0
    keep = [_aligned(a) for a in arenas]
    outs = [_out_buffer(total, fill) for _ in arenas]
    ress = [np.zeros(n, dtype=cx.FRAME_RESULT_DTYPE) for _ in arenas]
    tiers = (C.c_uint64 * 2)()
    VP = C.c_void_p * len(arenas)
    flags = (cx.VERIFY_CRC16 if verify_crc else 0) | cx.OUT_F32 | path
    st = lib().sim_decode_frames_f32(VP(*[al.ctypes.data for _, al in keep]), arena_len, len(arenas), descs.ctypes.data, n,
                                     VP(*[o.ctypes.data for o in outs]), out_offs.ctypes.data, VP(*[r.ctypes.data for r in ress]), flags, tiers)
    if st != 0:
        raise cx.ClaxonError(cx.API_ERROR, 0, "the simulator rejects this combination of flags (0x%x)" % flags)
    return list(zip(outs, ress)), (int(tiers[0]), int(tiers[1]))


def general_sure(descs, out_offs, flags):
    descs = np.ascontiguousarray(descs, dtype=cx.FRAME_DESC_DTYPE)
    out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
    return int(lib().sim_general_sure(descs.ctypes.data, descs.size, out_offs.ctypes.data, flags))


class SimF32Backend:
    """parity_util's backend contract for the float output under simulation: decode() returns (float32 output, results)."""
    name = "wavesim-f32"

    def __init__(self, path=0):
        self.path = path          # extra flags next to CLX_OUT_F32 (CLX_COMPOSE / CLX_NO_COMPOSE ...)

    def decode(self, arena, arena_len, descs, out_offs, verify_crc, fill=np.nan):
        (r,), _ = decode_runs([arena], arena_len, descs, out_offs, verify_crc=verify_crc, fill=fill, path=self.path)
        return r
