"""Loader for the wave simulator build of the energy VAD and the frame selection (tests/wavesim/sim_vad.cpp): clx_vad.hip's
argument checks and its five kernels as clx_vad_windows and clx_select_windows run them, on host buffers, and its context rule.
Also the definition of claxon_hip.h restated: restate_vad() and restate_select(), numpy in the stated order and precisions, which
the simulator and the GPU equal word for word; reference_vad(), the same with an exact threshold (rational arithmetic over the
cells) and exact compares of the cells against it, with the bound on the threshold that DESIGN.md 4.23 derives; and window_rule(),
the context [lo, hi] of a frame."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

import claxon_amd as cx
import simlib
import simlib_norm as sn

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_vad.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
TILE, THREADS, SPAN, MAX_CONTEXT, MAX_ROWS = 256, 256, 512, 128, 8192
SUM_LDS_BYTES, DECIDE_LDS_BYTES, RANK_LDS_BYTES, SCAN_LDS_BYTES, MOVE_LDS_BYTES = 0, 2080, 16, 0, 1040
U32 = 2.0 ** -24                         # the unit roundoff of float32
U64 = 2.0 ** -53                         # ... and of float64


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_vad.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_vad.hip"),
            os.path.join(simlib._CSRC, "clx_norm.hip"), os.path.join(_DIR, "fake", "hip", "hip_runtime.h"),
            os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: every add, multiply and divide is rounded once, as the helpers the kernels use are on the GPU
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_vad.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_vad_windows.argtypes = [vp, sz, u32, u32, vp, u32, C.c_int, f32, f32, u32, f32, u32, vp, vp, vp]
        _lib.sim_select_windows.argtypes = [vp, vp, sz, u32, u32, vp, vp, u32, C.c_int, f32, vp, vp]
        _lib.sim_vad_context.argtypes = [u32, u32, u32, vp]
        _lib.sim_vad_shape.argtypes = [vp]
        _lib.sim_vad_error.restype = C.c_char_p
        for f in ("tile", "threads", "span", "max_context", "sum_lds_bytes", "decide_lds_bytes", "rank_lds_bytes", "scan_lds_bytes",
                  "move_lds_bytes", "launch_count"):
            getattr(_lib, "sim_vad_" + f).restype = u32
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _dims(data, layout, shape):
    if shape is not None:
        return shape
    return (data.shape[0],) + ((data.shape[2], data.shape[1]) if layout == TC else (data.shape[1], data.shape[2]))


def _raise():
    raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_vad_error().decode())


def launches():
    """Kernels the simulator has launched so far."""
    return int(lib().sim_vad_launch_count())


def last_shape():
    """(n_tiles, n_chunks, sum_blocks, scan_blocks, partials, table words) of the last simulated call that launched."""
    a = np.zeros(6, dtype=np.uint32)
    lib().sim_vad_shape(a.ctypes.data)
    return tuple(int(v) for v in a)


def vad_windows(data, valid, layout, E=5.0, s=0.5, c=0, p=0.6, row=0, mask=None, thresholds=None, shape=None, opts=True, reserved=None):
    """clx_vad_windows under the simulator: `data` a float32 array, [B, rows, T] for CT and [B, T, rows] for TC (or any float32 buffer
    with shape=(B, rows, T)); mask a uint8 buffer of B * T bytes and thresholds a float32 one of B (None: new ones; False: NULL).
    Returns (mask, thresholds)."""
    B, rows, T = _dims(data, layout, shape)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    assert data is None or (data.flags["C_CONTIGUOUS"] and data.dtype == np.float32)
    if mask is None:
        mask = np.full((B, T), 0xa5, dtype=np.uint8)
    if thresholds is None:
        thresholds = np.full(B, np.nan, dtype=np.float32)
    mask = None if mask is False else mask
    thresholds = None if thresholds is False else thresholds
    res = None if reserved is None else np.ascontiguousarray(reserved, dtype=np.uint32)
    if lib().sim_vad_windows(_ptr(data), B, rows, T, _ptr(valid), layout, 1 if opts else 0, E, s, c, p, row, _ptr(res), _ptr(mask),
                             _ptr(thresholds)) != cx.OK:
        _raise()
    return mask, thresholds


def select_windows(data, out, valid, mask, layout, pad=0.0, shape=None, opts=True, reserved=None, counts=True):
    """clx_select_windows under the simulator: `data` and `out` float32 arrays of one shape (or buffers with shape=(B, rows, T)), mask
    a uint8 buffer of B * T bytes.  Returns (out, counts); counts=False: no counts are asked for (None is returned for them)."""
    B, rows, T = _dims(data, layout, shape)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    for a in (data, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.dtype == np.float32)
    assert mask is None or (mask.flags["C_CONTIGUOUS"] and mask.dtype == np.uint8)
    cnt = np.full(B, 0xdeadbeef, dtype=np.uint32) if counts else None
    res = None if reserved is None else np.ascontiguousarray(reserved, dtype=np.uint32)
    if lib().sim_select_windows(_ptr(data), _ptr(out), B, rows, T, _ptr(valid), _ptr(mask), layout, 1 if opts else 0, pad, _ptr(res),
                                _ptr(cnt)) != cx.OK:
        _raise()
    return out, cnt


def sim_context(t, V, c):
    """clx_vad::context, the production rule: (lo, hi)."""
    lh = np.zeros(2, dtype=np.uint32)
    lib().sim_vad_context(t, V, c, lh.ctypes.data)
    return int(lh[0]), int(lh[1])


def window_rule(t, V, c):
    """The context of frame t < V as claxon_hip.h states it: (lo, hi, den)."""
    lo, hi = max(t - c, 0), min(t + c, V - 1)
    return lo, hi, hi - lo + 1


def _decide(above, V, c, p):
    """The bytes of the live frames from their `above` flags: the stated rule, the product in float32."""
    t = np.arange(V)
    lo, hi = np.maximum(t - c, 0), np.minimum(t + c, V - 1)
    pre = np.concatenate(([0], np.cumsum(above.astype(np.int64))))
    num, den = pre[hi + 1] - pre[lo], hi - lo + 1
    return (num.astype(np.float32) >= den.astype(np.float32) * np.float32(p)).astype(np.uint8)


def restate_vad(x, valid, E=5.0, s=0.5, c=0, p=0.6, row=0, plain=False):
    """The definition in numpy, in the stated order and with the stated roundings: x float32 [B, rows, T] (CT).  Returns (mask uint8
    [B, T], thresholds float32 [B]).  plain=True adds the cells up in plain ascending order instead (not the definition: what the
    `wide` cases tell apart)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, rows, T = x.shape
    E, s = np.float32(E), np.float32(s)
    mask, thr = np.zeros((B, T), dtype=np.uint8), np.full(B, E, dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(B):
            V = int(valid[k])
            if V == 0:
                continue
            e = x[k, row, :V]
            if s != 0:
                if plain:
                    S = np.float64(0.0)
                    for v in e.astype(np.float64):
                        S = S + v
                else:
                    S = sn.ordered_sum(e.astype(np.float64))
                thr[k] = np.float32(np.float64(E) + np.float64(s) * (S / np.float64(V)))
            mask[k, :V] = _decide(e > thr[k], V, c, p)
    return mask, thr


def restate_select(x, valid, mask, pad=0.0):
    """The selection in numpy: x float32 [B, rows, T] (CT), mask uint8 [B, T].  Returns (y [B, rows, T], counts uint32 [B])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, rows, T = x.shape
    y = np.full_like(x, np.float32(pad))
    counts = np.zeros(B, dtype=np.uint32)
    for k in range(B):
        V = int(valid[k])
        at = np.flatnonzero(mask[k, :V] != 0)
        counts[k] = at.size
        y.view(np.uint32)[k, :, :at.size] = x.view(np.uint32)[k][:, at]
    return y, counts


def reference_vad(x, valid, E=5.0, s=0.5, c=0, p=0.6, row=0):
    """The definition with an exact threshold: thr* = E + s * (sum of e) / V in rational arithmetic over the float32 cells (nothing
    is rounded), every `above` an exact compare of a cell against it, then the stated decision rule (its float32 product is part of
    the definition, not an error of the implementation).  x [B, rows, T] with finite energy cells.  Returns (mask uint8 [B, T],
    thr* float64 [B] (the rational rounded once), bound float64 [B], doubt bool [B, T]).

    bound: |thr - thr*| for an implementation that adds the V cells up in doubles in any order, divides, multiplies and adds with
    one rounding each and rounds once to float32.  With A = sum |e|: the sum is within (V - 1) u64 A of exact (to first order), the
    division, the product and the last sum add a relative u64 each on a value of magnitude at most |E| + |s| A / V, and the float32
    rounding a relative U32 on the result:  U32 |thr*| + (V + 3) u64 (|E| + |s| A / V), the spare u64 holding the higher-order
    terms.  With s == 0 or V == 0 thr is E itself and the bound is 0.
    doubt[k, t]: the context of live frame t holds a cell within `bound` of thr*, so the decision there may differ."""
    x = np.asarray(x, dtype=np.float32)
    B, rows, T = x.shape
    Ef, sf = float(np.float32(E)), float(np.float32(s))
    mask, thr, bound, doubt = np.zeros((B, T), dtype=np.uint8), np.full(B, Ef), np.zeros(B), np.zeros((B, T), dtype=bool)
    for k in range(B):
        V = int(valid[k])
        if V == 0:
            continue
        e = [float(v) for v in x[k, row, :V]]
        exact = Fraction(Ef)
        if sf != 0:
            total = sum((Fraction(v) for v in e), Fraction(0))
            exact = Fraction(Ef) + Fraction(sf) * total / V
            A = float(sum((abs(Fraction(v)) for v in e), Fraction(0)))
            bound[k] = U32 * abs(float(exact)) + (V + 3) * U64 * (abs(Ef) + abs(sf) * A / V)
        thr[k] = float(exact)
        above = np.array([Fraction(v) > exact for v in e], dtype=bool)
        mask[k, :V] = _decide(above, V, c, p)
        near = np.array([abs(Fraction(v) - exact) <= Fraction(bound[k]) for v in e], dtype=np.int64) if sf != 0 else np.zeros(V, dtype=np.int64)
        t = np.arange(V)
        pre = np.concatenate(([0], np.cumsum(near)))
        doubt[k, :V] = pre[np.minimum(t + c, V - 1) + 1] - pre[np.maximum(t - c, 0)] > 0
    return mask, thr, bound, doubt
