"""Loader for the wave simulator build of the noise mixer (tests/wavesim/sim_add.cpp): clx_add.hip's argument checks, its table and
its kernels as clx_add_windows runs them, on host buffers.  Also the definition of claxon_hip.h twice over: restate(), numpy in the
stated order of the sums and with the stated roundings, which the simulator and the GPU equal bit for bit, and reference(), the
same in float64 with exact sums (math.fsum) and no float32 rounding, with the bounds DESIGN.md 4.17 derives around it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib
import simlib_norm as sn

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_add.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
CHUNK, STRANDS, MAX_ROWS = sn.CHUNK, sn.STRANDS, 8
GAIN_REL = 2.0 ** -23                    # |g / g_ref - 1| stays below this for sums of up to 2^24 terms


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_add.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_norm.hip"),
            os.path.join(simlib._CSRC, "clx_add.hip"), os.path.join(_DIR, "fake", "hip", "hip_runtime.h"),
            os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: every add, multiply and divide is rounded once; fmaf is the one fused operation, and it is asked for by name
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_add.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        _lib.sim_add_windows.argtypes = [vp, sz, u32, u32, vp, vp, sz, vp, vp, vp, u32, C.c_int, u32, vp, C.POINTER(C.c_int)]
        _lib.sim_add_error.restype = C.c_char_p
        for f in ("chunk", "strands", "max_rows", "table_bytes"):
            getattr(_lib, "sim_add_" + f).restype = u32
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def add_windows(data, valid, noise, noise_valid, noise_index, snr_db, layout, gains=None, shape=None, n_noise=None, reserved=None):
    """clx_add_windows under the simulator: `data` (a float32 array, [B, rows, T] for CT and [B, T, rows] for TC, or any float32
    buffer with shape=(B, rows, T)) mixed in place with `noise` ([N, ...] alike, or a buffer with n_noise=N); reserved None: opts
    NULL, else opts->reserved.  Returns whether the kernels were launched."""
    if shape is None:
        B = data.shape[0]
        rows, T = (data.shape[2], data.shape[1]) if layout == TC else (data.shape[1], data.shape[2])
    else:
        B, rows, T = shape
    if n_noise is None:
        n_noise = 0 if noise is None else noise.shape[0]
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    noise_valid = None if noise_valid is None else np.ascontiguousarray(noise_valid, dtype=np.uint32)
    noise_index = None if noise_index is None else np.ascontiguousarray(noise_index, dtype=np.int32)
    snr_db = None if snr_db is None else np.ascontiguousarray(snr_db, dtype=np.float32)
    for a in (data, noise, gains):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.dtype == np.float32)
    launched = C.c_int(0)
    st = lib().sim_add_windows(_ptr(data), B, rows, T, _ptr(valid), _ptr(noise), n_noise, _ptr(noise_valid), _ptr(noise_index), _ptr(snr_db),
                               layout, 0 if reserved is None else 1, reserved or 0, _ptr(gains), C.byref(launched))
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_add_error().decode())
    return bool(launched.value)


def fma32(g, n, x):
    """fmaf(g, n, x) of a float32 g and float32 arrays, one rounding: the product is exact in float64, the float64 sum is brought
    to round-to-odd with the error of the addition (TwoSum), and an odd-rounded float64 rounds to float32 as the exact value does."""
    p = np.float64(np.float32(g)) * np.asarray(n, dtype=np.float32).astype(np.float64)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + x
        bb = s - p
        err = (p - (s - bb)) + (x - bb)
        even = (s.view(np.int64) & 1) == 0
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        s = np.where((err != 0) & even & np.isfinite(s), odd, s)
        return s.astype(np.float32)


def ratio(snr_db):
    """q of the definition: the host's pow in double, 0 for +inf."""
    s = float(np.float32(snr_db))
    return 0.0 if math.isinf(s) else math.pow(10.0, -s / 10.0)


def _energy(cells, n):
    """Es / En: the rows' ordered sums of squares over t < n, added in ascending row order from +0.0."""
    c = cells[:, :n].astype(np.float64)
    e = np.float64(0.0)
    for rs in sn.ordered_sum(c * c):
        e = e + rs
    return e


def restate(x, valid, noise, noise_valid, noise_index, snr_db):
    """The definition in numpy, in the stated order and with the stated roundings: x [B, rows, T] and noise [N, rows, T] float32
    (CT).  Returns (y, gains); cells that the definition leaves alone keep x's words."""
    x = np.asarray(x, dtype=np.float32)
    B = x.shape[0]
    y = x.copy()
    gains = np.zeros(B, dtype=np.float32)
    snr = np.broadcast_to(np.asarray(snr_db, dtype=np.float32), (B,))
    with np.errstate(all="ignore"):
        for k in range(B):
            j, vs = int(noise_index[k]), int(valid[k])
            if j < 0:
                continue
            vn, q = min(int(noise_valid[j]), vs), ratio(snr[k])
            if vs == 0 or vn == 0 or q == 0.0:
                continue
            es, en = _energy(x[k], vs), _energy(noise[j], vn)
            if es == 0.0 or en == 0.0:
                continue
            g = np.float32(np.sqrt((es * np.float64(vn) * np.float64(q)) / (en * np.float64(vs))))
            gains[k] = g
            if g != 0:
                y[k, :, :vn] = fma32(g, noise[j, :, :vn], x[k, :, :vn])
    return y, gains


def reference(x, valid, noise, noise_valid, noise_index, snr_db):
    """The definition in float64 with exact sums (math.fsum of squares that are exact in float64) and no rounding to float32.
    Returns (y [B, rows, T] float64 -- live cells only, the rest copied --, g [B] float64, gn [B, rows, T]: |g n| per cell, 0 where
    nothing is added)."""
    x64 = np.asarray(x, dtype=np.float64)
    B = x64.shape[0]
    y, g, gn = x64.copy(), np.zeros(B), np.zeros(x64.shape)
    snr = np.broadcast_to(np.asarray(snr_db, dtype=np.float32), (B,))
    for k in range(B):
        j, vs = int(noise_index[k]), int(valid[k])
        if j < 0:
            continue
        vn, q = min(int(noise_valid[j]), vs), ratio(snr[k])
        if vs == 0 or vn == 0 or q == 0.0:
            continue
        s, n = x64[k, :, :vs].reshape(-1), np.asarray(noise[j], dtype=np.float64)[:, :vn]
        es, en = math.fsum(s * s), math.fsum(n.reshape(-1) ** 2)
        if es == 0.0 or en == 0.0:
            continue
        g[k] = math.sqrt((es / vs) / (en / vn) * q)
        y[k, :, :vn] = x64[k, :, :vn] + g[k] * n
        gn[k, :, :vn] = np.abs(g[k] * n)
    return y, g, gn


def cell_bound(out, gn):
    """|out - reference| <= 2^-24 |out| (the fma's one rounding) + 2^-23 |g n| (the gain) + 2^-149 (a result in the
    subnormal range)."""
    return sn.U32 * np.abs(np.asarray(out, dtype=np.float64)) + GAIN_REL * gn + 2.0 ** -149
