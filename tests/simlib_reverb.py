"""Loader for the wave simulator build of the reverberator (tests/wavesim/sim_reverb.cpp): clx_reverb.hip's argument checks, its
table and its kernels -- with clx_add's sum kernels between them -- as clx_reverb_windows runs them, on host buffers.  Also the
definition of claxon_hip.h twice over: restate(), numpy in the stated order of the chain and of the sums and with the stated
roundings, which the simulator and the GPU equal bit for bit, and reference(), the same in float64 with exact power sums
(math.fsum) and no float32 rounding, with the bounds DESIGN.md 4.18 derives around it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib
import simlib_add as sa
import simlib_norm as sn

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_reverb.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
U = 2.0 ** -24                           # float32's unit roundoff


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_reverb.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, f) for f in ("clx_norm.hip", "clx_add.hip", "clx_reverb.hip")] \
        + [os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: every add, multiply and divide is rounded once; fmaf is the one fused operation, and it is asked for by name
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_reverb.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        _lib.sim_reverb_windows.argtypes = [vp, sz, u32, u32, vp, vp, sz, u32, vp, vp, u32, C.c_int, u32, u32, vp, vp, C.POINTER(C.c_int)]
        _lib.sim_reverb_error.restype = C.c_char_p
        for f in ("tile", "chunk", "group", "max_rows", "max_taps", "lds_bytes", "table_bytes"):
            getattr(_lib, "sim_reverb_" + f).restype = u32
    return _lib


TILE, CHUNK, GROUP = (getattr(lib(), "sim_reverb_" + f)() for f in ("tile", "chunk", "group"))   # the kernel's own constants


def _ptr(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def reverb_windows(data, valid, ir, ir_len, ir_index, layout, out, keep_power=None, gains=None, shape=None, n_ir=None, K=None, reserved=0):
    """clx_reverb_windows under the simulator: `data` (a float32 array, [B, rows, T] for CT and [B, T, rows] for TC, or any float32
    buffer with shape=(B, rows, T)) convolved into `out` with the rows of `ir` ([N, K], or a buffer with n_ir=N and K=K);
    keep_power None: opts NULL, else opts = { keep_power, reserved }.  Returns whether the kernels were launched."""
    if shape is None:
        B = data.shape[0]
        rows, T = (data.shape[2], data.shape[1]) if layout == TC else (data.shape[1], data.shape[2])
    else:
        B, rows, T = shape
    if n_ir is None:
        n_ir = 0 if ir is None else ir.shape[0]
    if K is None:
        K = 1 if ir is None else ir.shape[1]
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    ir_len = None if ir_len is None else np.ascontiguousarray(ir_len, dtype=np.uint32)
    ir_index = None if ir_index is None else np.ascontiguousarray(ir_index, dtype=np.int32)
    for a in (data, ir, out, gains):
        assert a is None or isinstance(a, int) or (a.flags["C_CONTIGUOUS"] and a.dtype == np.float32)
    launched = C.c_int(0)
    st = lib().sim_reverb_windows(_ptr(data), B, rows, T, _ptr(valid), _ptr(ir), n_ir, K, _ptr(ir_len), _ptr(ir_index), layout,
                                  0 if keep_power is None else 1, int(keep_power or 0), reserved, _ptr(out), _ptr(gains), C.byref(launched))
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_reverb_error().decode())
    return bool(launched.value)


def _energy(cells, n):
    """Ex / Ey: the rows' ordered sums of squares over t < n, added in ascending row order from +0.0 (simlib_add's Es)."""
    return sa._energy(cells, n)


def chain(h, x):
    """One row's cells: y[t] = the ascending-k chain acc = fmaf(h[k], x[t - k], acc) from +0.0 over k <= min(t, len(h) - 1); taps
    with k > t are skipped.  h and x float32; the chain runs over every t at once, tap by tap."""
    x = np.asarray(x, dtype=np.float32)
    acc = np.zeros(x.size, dtype=np.float32)
    for k in range(min(len(h), x.size)):
        acc[k:] = sa.fma32(h[k], x[:x.size - k], acc[k:])
    return acc


def restate(x, valid, ir, ir_len, ir_index, keep_power):
    """The definition in numpy, in the stated order and with the stated roundings: x [B, rows, T] float32 (CT), ir [N, K].  Returns
    (y, gains)."""
    x = np.asarray(x, dtype=np.float32)
    B, rows, T = x.shape
    y = np.zeros_like(x)
    gains = np.ones(B, dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(B):
            j, v = int(ir_index[k]), int(valid[k])
            L = int(ir_len[j]) if j >= 0 else 0
            if L == 0:
                y[k, :, :v] = x[k, :, :v]
                continue
            for r in range(rows):
                y[k, r, :v] = chain(ir[j, :min(L, v)], x[k, r, :v])
            if not keep_power or v == 0:
                continue
            ex, ey = _energy(x[k], v), _energy(y[k], v)
            if ex == 0.0 or ey == 0.0:
                continue
            g = np.float32(np.sqrt(ex / ey))
            gains[k] = g
            if g != 1:
                y[k, :, :v] = y[k, :, :v] * g
    return y, gains


def reference(x, valid, ir, ir_len, ir_index, keep_power):
    """The definition in float64: np.convolve of the live samples with the live taps, exact power sums (math.fsum of squares that
    are exact in float64 for x; of the float64 y for Ey), no float32 rounding.  Returns (y [B, rows, T] float64 -- the unscaled
    convolution --, mag [B, rows, T]: the sum of |h[k] x[t - k]| per cell, N [B, T]: the taps of a cell's chain, g [B] float64)."""
    x64 = np.asarray(x, dtype=np.float64)
    B, rows, T = x64.shape
    y, mag, N, g = np.zeros(x64.shape), np.zeros(x64.shape), np.zeros((B, T)), np.ones(B)
    for k in range(B):
        j, v = int(ir_index[k]), int(valid[k])
        L = int(ir_len[j]) if j >= 0 else 0
        if L == 0 or v == 0:
            y[k, :, :v] = x64[k, :, :v]
            mag[k, :, :v] = np.abs(x64[k, :, :v])
            continue
        h = np.asarray(ir[j, :L], dtype=np.float64)
        for r in range(rows):
            y[k, r, :v] = np.convolve(x64[k, r, :v], h)[:v]
            mag[k, r, :v] = np.convolve(np.abs(x64[k, r, :v]), np.abs(h))[:v]
        N[k, :v] = np.minimum(np.arange(v) + 1, L)
        if keep_power:
            ex, ey = math.fsum((x64[k, :, :v] ** 2).reshape(-1)), math.fsum((y[k, :, :v] ** 2).reshape(-1))
            if ex != 0.0 and ey != 0.0:
                g[k] = math.sqrt(ex / ey)
    return y, mag, N, g


def gamma(n):
    """Higham's gamma_n for float32: n u / (1 - n u)."""
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def cell_bound(mag, N):
    """|y - y64| <= gamma_N sum |h[k] x[t - k]| (+ 2^-149 per step for results in the subnormal range) for the
    unscaled cell."""
    return gamma(N)[:, None, :] * mag + N[:, None, :] * 2.0 ** -149


def gain_rel(y64, mag, N, valid):
    """a bound on |g / g64 - 1| per window.  Ey is taken of the computed cells y + e, |e| <= cell_bound, so it
    lies within d = sum(2 |y| |e| + e^2) / Ey of the reference's, and sqrt(Ex / Ey) moves by at most d / (2 (1 - d)); the double
    sums, the division and the square root add less than 2^-40 between them for fewer than 2^13 terms a chunk fold, and the
    rounding to float32 adds 2^-24."""
    e = cell_bound(mag, N)
    rel = np.zeros(y64.shape[0])
    for k, v in enumerate(valid):
        ey = math.fsum((y64[k, :, :v] ** 2).reshape(-1))
        d = math.fsum((2 * np.abs(y64[k, :, :v]) * e[k, :, :v] + e[k, :, :v] ** 2).reshape(-1)) / ey if ey > 0 else 0.0
        assert d < 0.5, d
        rel[k] = (1 + U) * (1 + 2.0 ** -40) * (1 + d / (2 * (1 - d))) - 1 + U
    return rel


def scaled_bound(out, y64, g64, mag, N, g_rel):
    """DESIGN.md 4.18, keep_power: out = fl(y' g') with y' = y + e and g' = g (1 + r), |r| <= g_rel, so
    |out - g y| <= g (1 + g_rel) |e| + g_rel g |y| + 2^-24 |out| (the multiplication) + 2^-149."""
    g, r = g64[:, None, None], g_rel[:, None, None]
    return g * (1 + r) * cell_bound(mag, N) + r * np.abs(g * y64) + U * np.abs(np.asarray(out, dtype=np.float64)) + 2.0 ** -149
