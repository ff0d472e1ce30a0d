"""Loader for the wave simulator build of SpecAugment (tests/wavesim/sim_specaug.cpp): clx_specaug.hip's argument checks and its
kernels as clx_specaug_windows runs them, on host buffers.  Also the definition of claxon_hip.h twice over: restate(), numpy float32
in the stated order, which the simulator and the GPU equal bit for bit, and reference(), the same in float64 without the float32
roundings, with bound(), the per-cell interval around it that DESIGN.md 4.20 derives; and torch_bound(), 4.20's interval around
torch.nn.functional.interpolate(mode="bicubic") of the two segments."""
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
_SO = os.path.join(_DIR, "libwavesim_specaug.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
TILE, THREADS, MAX_ROWS, MAX_MASKS, LDS_BYTES = 256, 256, 256, 32, 9248
U32 = 2.0 ** -24                         # the unit roundoff of float32
W_ERR = 48 * U32                         # how far a float32 weight lies from the exact one
SLOPE = 2 * 1.35 + 2 * 0.75              # the four weights' largest slopes added up
W_ABS = 1.5                              # more than the four weights' magnitudes added up (at most 1.375, at tx = 1/2)


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_specaug.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_norm.hip"),
            os.path.join(simlib._CSRC, "clx_specaug.hip"), os.path.join(_DIR, "fake", "hip", "hip_runtime.h"),
            os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: every add, subtract, multiply and divide is rounded once; fmaf is the one fused operation, asked for by name
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_specaug.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_specaug_windows.argtypes = [vp, vp, sz, u32, u32, vp, u32, vp, vp, vp, C.c_int, u32, u32, u32, f32, u32, vp]
        _lib.sim_specaug_error.restype = C.c_char_p
        for f in ("tile", "threads", "max_rows", "max_masks", "max_t", "lds_bytes"):
            getattr(_lib, "sim_specaug_" + f).restype = u32
    return _lib


def _u32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a):
    return None if a is None else a.ctypes.data


def specaug_windows(data, out, valid, layout, warp=None, fm=None, tm=None, fill="mean", fills=None, shape=None, opts=True, F=None, M=None,
                    reserved=0, fill_mean=None):
    """clx_specaug_windows under the simulator: `data` and `out` float32 arrays ([B, rows, T] for CT, [B, T, rows] for TC, or any
    float32 buffers with shape=(B, rows, T)), warp [B, 2], fm [B, F, 2], tm [B, M, 2] (each may be None), fill "mean" or a float.
    opts=False: a NULL options pointer; F, M, reserved and fill_mean override what the options would say.  Returns out."""
    if shape is None:
        B = data.shape[0]
        rows, T = (data.shape[2], data.shape[1]) if layout == TC else (data.shape[1], data.shape[2])
    else:
        B, rows, T = shape
    valid, warp, fm, tm = _u32(valid), _u32(warp), _u32(fm), _u32(tm)
    for a in (data, out, fills):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.dtype == np.float32)
    mean = fill == "mean"
    st = lib().sim_specaug_windows(_ptr(data), _ptr(out), B, rows, T, _ptr(valid), layout, _ptr(warp), _ptr(fm), _ptr(tm), 1 if opts else 0,
                                   (0 if fm is None else fm.shape[1]) if F is None else F, (0 if tm is None else tm.shape[1]) if M is None else M,
                                   (1 if mean else 0) if fill_mean is None else fill_mean, 0.0 if mean else fill, reserved, _ptr(fills))
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_specaug_error().decode())
    return out


def segments(V, c, w):
    """The resized segments of a window, (first input frame, I, first output frame, O); none where the warp copies."""
    return [] if c == w else [(0, c, 0, w), (c, V - c, w, V - w)]


def coordinates(I, O):
    """(ix, rem, den) of every local output frame j < O: exact integers."""
    j = np.arange(O, dtype=np.int64)
    num, den = (2 * j + 1) * I - O, 2 * O
    ix = num // den                                          # (numpy's floor division: -1 where num < 0)
    return ix, num - ix * den, den


def _near32(u):
    f = np.float32
    return ((f(1.25) * u - f(2.25)) * u) * u + f(1)          # (float32 arrays: every operation is rounded once)


def _far32(u):
    f = np.float32
    return ((f(-0.75) * u + f(3.75)) * u - f(6)) * u + f(3)


def weights32(rem, den):
    """tx and the four weights [4, O] in float32 with the stated roundings."""
    tx = (rem.astype(np.float64) / np.float64(den)).astype(np.float32)
    one, two = np.float32(1), np.float32(2)
    return tx, np.stack([_far32(tx + one), _near32(tx), _near32(one - tx), _far32(two - tx)])


def weights64(rem, den):
    tx = rem.astype(np.float64) / np.float64(den)
    near = lambda u: ((1.25 * u - 2.25) * u) * u + 1
    far = lambda u: ((-0.75 * u + 3.75) * u - 6) * u + 3
    return tx, np.stack([far(tx + 1), near(tx), near(1 - tx), far(2 - tx)])


def masked(V, rows, fm_k, tm_k):
    """[rows, V] bool: the live cells of a window that its masks cover."""
    m = np.zeros((rows, V), dtype=bool)
    for first, width in (fm_k if fm_k is not None else ()):
        m[int(first):int(first) + int(width), :] = True
    for first, width in (tm_k if tm_k is not None else ()):
        m[:, int(first):int(first) + int(width)] = True
    return m


def mean_fill(xk, V):
    """The mean of a window's live cells xk [rows, T] in the stated order."""
    if V == 0:
        return np.float32(0)
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for rs in sn.ordered_sum(xk[:, :V].astype(np.float64)):
            s = s + rs
        return np.float32(s / np.float64(V * xk.shape[0]))


def restate(x, valid, warp=None, fm=None, tm=None, fill="mean"):
    """The definition in numpy, in the stated order and with the stated roundings: x float32 [B, rows, T] (CT).  Returns (y, fills)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, rows, T = x.shape
    y = x.copy()                                             # (padding and copied cells: the input's words)
    fills = np.zeros(B, dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(B):
            V = int(valid[k])
            fills[k] = mean_fill(x[k], V) if fill == "mean" else np.float32(fill)
            c, w = (int(warp[k][0]), int(warp[k][1])) if warp is not None else (0, 0)
            for b, I, ob, O in segments(V, c, w):
                ix, rem, den = coordinates(I, O)
                _, wt = weights32(rem, den)
                acc = np.zeros((rows, O), dtype=np.float32)
                for q in range(4):
                    src = b + np.clip(ix - 1 + q, 0, I - 1)
                    acc = sa.fma32(np.broadcast_to(wt[q], (rows, O)), x[k][:, src], acc)
                y[k, :, ob:ob + O] = acc
            m = masked(V, rows, None if fm is None else fm[k], None if tm is None else tm[k])
            y[k, :, :V][m] = fills[k]
    return y, fills


def reference(x, valid, warp=None):
    """The warp in float64 with no float32 rounding (masks and fills are exact selections and are left out): x [B, rows, T], finite
    live cells.  Returns (y, allow): the float64 cells and bound(), DESIGN.md 4.20's per-cell interval: the four weights each within
    W_ERR of the exact ones, and the chain of four fused steps within gamma_4 of the sum of its terms' magnitudes."""
    x = np.asarray(x, dtype=np.float64)
    B, rows, T = x.shape
    y, allow = x.copy(), np.zeros(x.shape)
    g4 = 4 * U32 / (1 - 4 * U32)
    for k in range(B):
        V = int(valid[k])
        c, w = (int(warp[k][0]), int(warp[k][1])) if warp is not None else (0, 0)
        for b, I, ob, O in segments(V, c, w):
            ix, rem, den = coordinates(I, O)
            _, wt = weights64(rem, den)
            acc, mag, tap = np.zeros((rows, O)), np.zeros((rows, O)), np.zeros((rows, O))
            for q in range(4):
                xs = x[k][:, b + np.clip(ix - 1 + q, 0, I - 1)]
                acc += wt[q] * xs
                mag += (np.abs(wt[q]) + W_ERR) * np.abs(xs)
                tap += np.abs(xs)
            y[k, :, ob:ob + O] = acc
            allow[k, :, ob:ob + O] = W_ERR * tap + g4 * mag + 2.0 ** -149
    return y, allow


def bound(x, valid, warp=None):
    return reference(x, valid, warp)[1]


def torch_warp(x, valid, warp):
    """The two segments of every warped window through torch.nn.functional.interpolate(mode="bicubic", align_corners=False) on the
    CPU, and 4.20's interval around it.  torch takes the coordinate through a float32 scale: src = fl(fl(I / O) (j + 0.5)) - 0.5 is
    within 3 I 2^-24 frames of the exact one; the interpolant is continuous in the coordinate with a slope of at most SLOPE times
    the largest tap, so that moves a cell by at most 3 I 2^-24 SLOPE X, X the largest magnitude of the row's segment; and each of
    the two implementations then rounds: four weights within W_ERR, a chain within gamma_4 of W_ABS X.  Returns (y, allow)."""
    import torch
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, rows, T = x.shape
    y, allow = x.astype(np.float64), np.zeros(x.shape)
    g4 = 4 * U32 / (1 - 4 * U32)
    for k in range(B):
        V = int(valid[k])
        c, w = int(warp[k][0]), int(warp[k][1])
        for b, I, ob, O in segments(V, c, w):
            seg = torch.from_numpy(x[k][:, b:b + I].copy()).view(1, rows, 1, I)
            r = torch.nn.functional.interpolate(seg, size=(1, O), mode="bicubic", align_corners=False).view(rows, O).numpy()
            X = np.abs(x[k][:, b:b + I]).max(axis=1, keepdims=True).astype(np.float64)
            y[k, :, ob:ob + O] = r
            allow[k, :, ob:ob + O] = (3 * I * U32 * SLOPE + 2 * (4 * W_ERR + g4 * (W_ABS + 4 * W_ERR))) * X + 2.0 ** -149
    return y, allow
