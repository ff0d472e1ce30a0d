"""Loader for the wave simulator build of frame splicing (tests/wavesim/sim_splice.cpp): clx_splice.hip's argument checks, its
kernel as clx_splice_windows runs it, on host buffers, and its host builder of the delta plan.  Also the definition of claxon_hip.h
twice over: restate(), numpy float32 in the stated order, which the simulator and the GPU equal bit for bit, and reference(), the
same in float64 without the float32 roundings, with the per-cell bound that DESIGN.md 4.21 derives; apply_lfr(), an index-level
restatement of FunASR's low-frame-rate stacking as this project reads it; and deltas64(), the delta filters in float64."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib
import simlib_add as sa

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_splice.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
TILE, THREADS, STAGE_WORDS, LDS_BYTES = 256, 256, 8192, 37504
U32 = 2.0 ** -24                         # the unit roundoff of float32


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_splice.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_splice.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: fmaf is the one fused operation, asked for by name
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_splice.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_splice_windows.argtypes = [vp, vp, sz, u32, u32, vp, u32, vp, vp, C.c_int, u32, u32, f32, u32]
        _lib.sim_splice_deltas.argtypes = [u32, u32, vp, vp, vp]
        _lib.sim_splice_shape.argtypes = [vp]
        _lib.sim_splice_error.restype = C.c_char_p
        for f in ("tile", "threads", "stage_words", "lds_bytes"):
            getattr(_lib, "sim_splice_" + f).restype = u32
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def splice_windows(data, out, valid, layout, splice, shape=None, opts=True, blocks=True, coefs=True, K=None, stride=None, reserved=0, raw=None):
    """clx_splice_windows under the simulator: `data` and `out` float32 arrays ([B, rows, T] for CT, [B, T, rows] for TC, or any
    float32 buffers with shape=(B, rows, T)) and a cx.Splice.  opts=False, blocks=False, coefs=False: that pointer is NULL; K, stride
    and reserved override what the options would say; raw=(blocks [K, 4] int32, coefs float32) takes the place of the Splice's own
    tables.  Returns out."""
    if shape is None:
        B = data.shape[0]
        rows, T = (data.shape[2], data.shape[1]) if layout == TC else (data.shape[1], data.shape[2])
    else:
        B, rows, T = shape
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    for a in (data, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.dtype == np.float32)
    blk, cf = splice._tables() if raw is None else (np.ascontiguousarray(raw[0], dtype=np.int32), np.ascontiguousarray(raw[1], dtype=np.float32))
    st = lib().sim_splice_windows(_ptr(data), _ptr(out), B, rows, T, _ptr(valid), layout, _ptr(blk) if blocks else None,
                                  _ptr(cf) if coefs and cf.size else None, 1 if opts else 0, blk.shape[0] if K is None else K,
                                  splice.stride if stride is None else stride, splice.pad, reserved)
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_splice_error().decode())
    return out


def last_shape():
    """(Fs, Rc, H) of the last simulated call that launched: the sub-tile's output frames and rows, the plan's reach."""
    a = np.zeros(3, dtype=np.uint32)
    lib().sim_splice_shape(a.ctypes.data)
    return tuple(int(v) for v in a)


def deltas_tables(order, window):
    """clx_splice_deltas_build under the simulator's host build: (blocks [order + 1, 4] int32, coefs float32)."""
    blk = np.zeros((order + 1, 4), dtype=np.int32)
    coefs = np.zeros(128, dtype=np.float32)
    n = C.c_uint32(0)
    if lib().sim_splice_deltas(order, window, blk.ctypes.data, coefs.ctypes.data, C.addressof(n)) != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_splice_error().decode())
    return blk, coefs[:n.value].copy()


def deltas64(order, window):
    """The delta filters in float64, [filter of order 1, .., filter of order `order`]: whole numerators (the i-fold convolution of
    [-window .. window]) over whole denominators (2 sum d^2)^i, one float64 division."""
    base = np.arange(-window, window + 1, dtype=np.int64)
    norm = 2 * int(sum(d * d for d in range(1, window + 1)))
    num, den, out = np.array([1], dtype=np.int64), 1, []
    for _ in range(order):
        num, den = np.convolve(num, base), den * norm
        out.append(num.astype(np.float64) / np.float64(den))
    return out


def _frames(V, V_out, stride, off):
    """clamp(u * stride + off) for u < V_out."""
    return np.clip(np.arange(V_out, dtype=np.int64) * stride + off, 0, V - 1)


def restate(x, valid, splice):
    """The definition in numpy, in the stated order and with the stated roundings: x float32 [B, rows, T] (CT).  Returns y
    [B, K * rows, ceil(T / stride)]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, rows, T = x.shape
    s, K = splice.stride, len(splice.blocks)
    y = np.full((B, K * rows, splice.frames_out(T)), np.float32(splice.pad), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(B):
            V = int(valid[k])
            V_out = splice.frames_out(V)
            if V == 0:
                continue
            for j, (off, c) in enumerate(splice.blocks):
                dst = y[k, j * rows:(j + 1) * rows, :V_out]
                if c is None:
                    dst.view(np.uint32)[...] = x[k][:, _frames(V, V_out, s, off)].view(np.uint32)
                    continue
                m = len(c) // 2
                acc = np.zeros((rows, V_out), dtype=np.float32)
                for d in range(-m, m + 1):
                    acc = sa.fma32(np.float32(c[d + m]), x[k][:, _frames(V, V_out, s, off + d)], acc)
                dst[...] = acc
    return y


def reference(x, valid, splice, coefs64=None):
    """The definition in float64 with no float32 rounding: x [B, rows, T].  coefs64, if given, holds for every block the exact
    coefficients that the Splice's float32 ones were rounded from (None for a copy block).  Returns (y, allow): the float64 cells
    and DESIGN.md 4.21's bound (gamma_n + u) sum |c_d| |x_d| with n = 2m + 1 (0 for a copied or a padding cell)."""
    x = np.asarray(x, dtype=np.float64)
    B, rows, T = x.shape
    s, K = splice.stride, len(splice.blocks)
    y = np.full((B, K * rows, splice.frames_out(T)), np.float64(splice.pad))
    allow = np.zeros(y.shape)
    with np.errstate(all="ignore"):
        for k in range(B):
            V = int(valid[k])
            V_out = splice.frames_out(V)
            if V == 0:
                continue
            for j, (off, c) in enumerate(splice.blocks):
                sl = (k, slice(j * rows, (j + 1) * rows), slice(0, V_out))
                if c is None:
                    y[sl] = x[k][:, _frames(V, V_out, s, off)]
                    continue
                c = np.asarray(c if coefs64 is None else coefs64[j], dtype=np.float64)
                m, n = len(c) // 2, len(c)
                acc, mag = np.zeros((rows, V_out)), np.zeros((rows, V_out))
                for d in range(-m, m + 1):
                    xs = x[k][:, _frames(V, V_out, s, off + d)]
                    acc += c[d + m] * xs
                    mag += abs(c[d + m]) * np.abs(xs)
                y[sl] = acc
                allow[sl] = (n * U32 / (1 - n * U32) + U32) * mag
    return y, allow


def apply_lfr(frames, m, n):
    """Low-frame-rate stacking of one utterance as FunASR's front end does it, restated index by index: frames [V, rows] -> [ceil(V / n),
    m * rows].  (m - 1) // 2 copies of the first frame go in front; output i is the m padded frames from i * n on, laid side by
    side; where the padded utterance ends early the last frame fills the rest."""
    V = frames.shape[0]
    left = (m - 1) // 2
    padded = [frames[0]] * left + [frames[t] for t in range(V)]
    out = []
    for i in range(-(-V // n)):
        got = padded[i * n:i * n + m]
        got = got + [frames[V - 1]] * (m - len(got))
        out.append(np.concatenate(got))
    return np.stack(out)
