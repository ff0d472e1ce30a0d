"""Loader for the wave simulator build of the per-window normalisation (tests/wavesim/sim_norm.cpp): clx_norm.hip's argument checks
and its kernels as clx_norm_windows runs them, on host buffers.  Also the definition of claxon_hip.h twice over: restate(), numpy
in the stated order of the sums, which the simulator and the GPU equal bit for bit, and reference(), the same in float64 without
the float32 roundings, with bound(), the per-cell interval around it that DESIGN.md 4.15 derives."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_norm.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
CHUNK, STRANDS, MAX_ROWS = 4096, 64, 256
U32 = 2.0 ** -24                         # the unit roundoff of float32
U64 = 2.0 ** -53                         # ... and of float64


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_norm.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_norm.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: every subtract, add, multiply and divide is rounded once, as __fsub_rn and its kin are on the GPU
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_norm.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_norm_windows.argtypes = [vp, sz, u32, u32, vp, u32, C.c_int, u32, u32, u32, f32, f32, vp]
        _lib.sim_norm_error.restype = C.c_char_p
        for f in ("chunk", "strands", "max_rows", "tc_lds_bytes", "apply_lds_bytes"):
            getattr(_lib, "sim_norm_" + f).restype = u32
    return _lib


def opts(mean=1, var=1, ddof=0, eps=0.0, pad=0.0):
    return dict(mean=mean, var=var, ddof=ddof, eps=eps, pad=pad)


def of_norm(norm):
    """The options of a claxon_amd.Norm."""
    return opts(int(norm.mean), int(norm.var), norm.ddof, norm.eps, norm.pad)


def norm_windows(data, valid, layout, o, stats=None, shape=None):
    """clx_norm_windows under the simulator, `data` (a float32 array, [B, rows, T] for CT and [B, T, rows] for TC, or any float32
    buffer with shape=(B, rows, T)) normalised in place; o is opts(...) or None (a NULL pointer).  Returns data."""
    if shape is None:
        B = data.shape[0]
        rows, T = (data.shape[2], data.shape[1]) if layout == TC else (data.shape[1], data.shape[2])
    else:
        B, rows, T = shape
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    for a in (data, stats):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.dtype == np.float32)
    q = o or opts()
    st = lib().sim_norm_windows(None if data is None else data.ctypes.data, B, rows, T, None if valid is None else valid.ctypes.data, layout,
                                0 if o is None else 1, q["mean"], q["var"], q["ddof"], q["eps"], q["pad"],
                                None if stats is None else stats.ctypes.data)
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_norm_error().decode())
    return data


def ordered_sum(terms):
    """The sum of float64 `terms` [..., n] along the last axis in the order of claxon_hip.h: chunks of 4096, 64 strands a chunk, the xor
    fold, the chunks' partials ascending.  (A strand that is short of a term adds +0.0, which changes no sum that started at +0.0.)"""
    terms = np.asarray(terms, dtype=np.float64)
    n = terms.shape[-1]
    total = np.zeros(terms.shape[:-1], dtype=np.float64)
    idx = np.arange(STRANDS)
    for c0 in range(0, n, CHUNK):
        seg = terms[..., c0:c0 + CHUNK]
        rounds = -(-seg.shape[-1] // STRANDS)
        a = np.zeros(terms.shape[:-1] + (rounds * STRANDS,), dtype=np.float64)
        a[..., :seg.shape[-1]] = seg
        a = a.reshape(terms.shape[:-1] + (rounds, STRANDS))
        acc = np.zeros(terms.shape[:-1] + (STRANDS,), dtype=np.float64)
        for j in range(rounds):
            acc = acc + a[..., j, :]
        for d in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[..., idx ^ d]
        total = total + acc[..., 0]
    return total


def restate(x, valid, o):
    """The definition in numpy, in the stated order and with the stated roundings: x is float32 [B, rows, T] (CT).  Returns (y, stats)."""
    x = np.asarray(x, dtype=np.float32)
    B, rows, T = x.shape
    y = np.full_like(x, np.float32(o["pad"]))
    stats = np.zeros((B, rows, 2), dtype=np.float32)
    eps = np.float32(o["eps"])
    with np.errstate(all="ignore"):
        for k in range(B):
            n = int(valid[k])
            xs = x[k, :, :n]
            m = (ordered_sum(xs.astype(np.float64)) / n).astype(np.float32) if n else np.zeros(rows, np.float32)
            d = xs - m[:, None]                              # (float32 - float32: one rounding)
            s = np.ones(rows, dtype=np.float32)
            if o["var"]:
                d64 = d.astype(np.float64)
                v = (ordered_sum(d64 * d64) / (n - o["ddof"])).astype(np.float32) if n > o["ddof"] else np.zeros(rows, np.float32)
                s = np.sqrt(v + eps)                         # (float32 throughout)
            out = d if o["mean"] else xs
            if o["var"]:
                out = out / s[:, None]
            y[k, :, :n] = out
            stats[k, :, 0], stats[k, :, 1] = m, s
    return y, stats


def reference(x, valid, o):
    """The definition in float64 with no float32 rounding anywhere (the sums by math.fsum: exact, rounded once): x is [B, rows, T] of
    any float type.  Returns (y, mean, scale), float64; padding is o['pad']."""
    x = np.asarray(x, dtype=np.float64)
    B, rows, T = x.shape
    y = np.full(x.shape, float(np.float32(o["pad"])), dtype=np.float64)
    mu, sc = np.zeros((B, rows)), np.ones((B, rows))
    eps = float(np.float32(o["eps"]))
    with np.errstate(all="ignore"):
        for k in range(B):
            n = int(valid[k])
            for r in range(rows):
                xs = x[k, r, :n]
                m = math.fsum(xs) / n if n else 0.0
                d = xs - m
                s = 1.0
                if o["var"]:
                    v = math.fsum(d * d) / (n - o["ddof"]) if n > o["ddof"] else 0.0
                    s = math.sqrt(v + eps)
                out = d if o["mean"] else xs
                if o["var"]:
                    out = out / s if s > 0 else np.where(out == 0, np.nan, np.copysign(np.inf, out))
                y[k, r, :n] = out
                mu[k, r], sc[k, r] = m, s
    return y, mu, sc


def bound(x, valid, o, sum_rel=None, u=U32, sq_rounded=False, dx=None):
    """DESIGN.md 4.15's interval: |cell - reference cell| <= bound, per cell, for an implementation of the definition whose sums are
    within sum_rel (default n * 2^-53: ours) of exact relative to the sum of the magnitudes of their terms, and whose m, v, v + eps,
    sqrt, x - m and y / s are each one rounding of unit roundoff u (default float32's: ours).  sq_rounded: the squares are rounded
    (by u) before they are added, as in an implementation that works in one precision throughout.  dx [B, rows, T]: how far the
    implementation's input cells may lie from x, the reference's.  Cells of padding have bound 0; a row whose interval of the scale
    reaches 0 has bound inf."""
    x = np.asarray(x, dtype=np.float64)
    B, rows, T = x.shape
    yref, mu, sc = reference(x, valid, o)
    out = np.zeros(x.shape, dtype=np.float64)
    tiny = 2.0 ** -149
    eps = float(np.float32(o["eps"]))
    with np.errstate(all="ignore"):
        for k in range(B):
            n = int(valid[k])
            if n == 0:
                continue
            g = n * U64 if sum_rel is None else sum_rel
            xs = x[k, :, :n]
            ex = np.zeros_like(xs) if dx is None else np.asarray(dx, dtype=np.float64)[k, :, :n]
            D = xs - mu[k][:, None]
            absx = (np.abs(xs) + ex).sum(axis=1) / n
            dm = ex.sum(axis=1) / n + u * (np.abs(mu[k]) + ex.sum(axis=1) / n) + (1 + u) * g * absx + tiny   # |m - mu|
            dd = ex + dm[:, None] + u * (np.abs(D) + ex + dm[:, None]) + tiny                     # |d[t] - D[t]|
            if not o["var"]:
                out[k, :, :n] = dd if o["mean"] else ex
                continue
            nd = max(n - o["ddof"], 1)
            sq = (2 * np.abs(D) * dd + dd * dd).sum(axis=1)                                       # |sum d^2 - sum D^2|
            Qm = (np.abs(D) + dd) ** 2
            gq = g + (u if sq_rounded else 0.0)
            dQ = sq + gq * (1 + g) * Qm.sum(axis=1)
            V = sc[k] ** 2 - eps
            dv = (dQ / nd) * (1 + u) + u * np.abs(V) + tiny if n > o["ddof"] else np.zeros(rows)
            A = sc[k] ** 2
            da = dv + u * (A + dv) + tiny                                                         # |fl(v + eps) - (V + eps)|
            ds = da / sc[k] + u * (sc[k] + da / sc[k])                                            # |s - sigma|: sqrt, then one rounding
            num = D if o["mean"] else xs
            dn = dd if o["mean"] else ex
            lo = sc[k] - ds
            q = (dn * sc[k][:, None] + np.abs(num) * ds[:, None]) / (sc[k] * lo)[:, None]         # |d / s - D / sigma|
            b = q + u * (np.abs(yref[k, :, :n]) + q) + tiny
            b = np.where((lo > 0)[:, None], b, np.inf)
            out[k, :, :n] = b
    return out
