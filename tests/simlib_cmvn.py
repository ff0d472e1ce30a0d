"""Loader for the wave simulator build of global and sliding-window CMVN (tests/wavesim/sim_cmvn.cpp): clx_cmvn.hip's argument
checks, its two kernels as clx_cmvn_global_windows and clx_cmvn_sliding_windows run them, on host buffers, its statistics window
and its host builder of shift and scale.  Also the definition of claxon_hip.h twice over: restate_global() and restate_sliding(),
numpy in the stated order and precisions, which the simulator and the GPU equal bit for bit; reference_sliding(), the same with
exact sums (math.fsum) and float64 arithmetic without the float32 rounding, with the per-cell bound that DESIGN.md 4.22 derives;
window(), the statistics window rule; and from_stats64(), the accumulator rule as one float64 numpy line."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_cmvn.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
TILE, THREADS, GROUP, RC, MAX_SPAN, SLIDING_LDS_BYTES, GLOBAL_LDS_BYTES = 256, 256, 32, 8, 1311, 48608, 0
U32 = 2.0 ** -24                         # the unit roundoff of float32
U64 = 2.0 ** -53                         # ... and of float64
VAR_FLOOR = 1e-10


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_cmvn.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_cmvn.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: every add, subtract, multiply and divide is rounded once, as the helpers of clx_cmvn.hip are on the GPU
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_cmvn.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_cmvn_global_windows.argtypes = [vp, sz, u32, u32, vp, u32, vp, vp, C.c_int, f32, u32]
        _lib.sim_cmvn_sliding_windows.argtypes = [vp, vp, sz, u32, u32, vp, u32, C.c_int, u32, u32, u32, u32, f32, u32]
        _lib.sim_cmvn_from_stats.argtypes = [vp, u32, u32, vp, vp]
        _lib.sim_cmvn_window.argtypes = [u32, u32, u32, u32, u32, vp]
        _lib.sim_cmvn_shape.argtypes = [vp]
        _lib.sim_cmvn_error.restype = C.c_char_p
        for f in ("tile", "threads", "row_chunk", "max_span", "sliding_lds_bytes", "global_lds_bytes", "launch_count"):
            getattr(_lib, "sim_cmvn_" + f).restype = u32
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _dims(data, layout, shape):
    if shape is not None:
        return shape
    return (data.shape[0],) + ((data.shape[2], data.shape[1]) if layout == TC else (data.shape[1], data.shape[2]))


def _raise():
    raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_cmvn_error().decode())


def launches():
    """Kernels the simulator has launched so far."""
    return int(lib().sim_cmvn_launch_count())


def global_windows(data, valid, layout, shift, scale, pad=0.0, shape=None, opts=True, reserved=0):
    """clx_cmvn_global_windows under the simulator, `data` (a float32 array, [B, rows, T] for CT and [B, T, rows] for TC, or any
    float32 buffer with shape=(B, rows, T)) normalised in place; shift and scale float32 arrays or None (NULL); opts=False: opts is
    NULL.  Returns data."""
    B, rows, T = _dims(data, layout, shape)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float32)
    scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    assert data is None or (data.flags["C_CONTIGUOUS"] and data.dtype == np.float32)
    if lib().sim_cmvn_global_windows(_ptr(data), B, rows, T, _ptr(valid), layout, _ptr(shift), _ptr(scale), 1 if opts else 0, pad, reserved) != cx.OK:
        _raise()
    return data


def sliding_windows(data, out, valid, layout, window, min_window, center, norm_vars, pad=0.0, shape=None, opts=True, reserved=0):
    """clx_cmvn_sliding_windows under the simulator: `data` and `out` float32 arrays of one shape (or any float32 buffers with
    shape=(B, rows, T)).  Returns out."""
    B, rows, T = _dims(data, layout, shape)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    for a in (data, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.dtype == np.float32)
    if lib().sim_cmvn_sliding_windows(_ptr(data), _ptr(out), B, rows, T, _ptr(valid), layout, 1 if opts else 0, window, min_window, int(center),
                                      int(norm_vars), pad, reserved) != cx.OK:
        _raise()
    return out


def last_shape():
    """(n_tiles, Rc, span, table words) of the last simulated call that launched."""
    a = np.zeros(4, dtype=np.uint32)
    lib().sim_cmvn_shape(a.ctypes.data)
    return tuple(int(v) for v in a)


def sim_window(t, V, N, M, center):
    """clx_cmvn::stat_window, the production rule: (a, b)."""
    ab = np.zeros(2, dtype=np.uint32)
    lib().sim_cmvn_window(t, V, N, M, int(center), ab.ctypes.data)
    return int(ab[0]), int(ab[1])


def window(t, V, N, M, center):
    """The statistics window [a, b) of frame t of a window with V live frames, as claxon_hip.h states it."""
    if center:
        a = t - N // 2
        b = a + N
    else:
        a = t - N
        b = t + 1
    if a < 0:
        b -= a
        a = 0
    if not center and b > t:
        b = max(t + 1, M)
    if b > V:
        a -= b - V
        b = V
        if a < 0:
            a = 0
    return a, b


def from_stats(stats, norm_vars=True):
    """clx_cmvn_from_stats_build under the simulator's host build: (shift, scale) float32."""
    st = np.ascontiguousarray(stats, dtype=np.float64)
    rows = st.shape[1] - 1
    shift, scale = np.zeros(rows, dtype=np.float32), np.zeros(rows, dtype=np.float32)
    if lib().sim_cmvn_from_stats(st.ctypes.data, rows, int(norm_vars), shift.ctypes.data, scale.ctypes.data) != cx.OK:
        _raise()
    return shift, scale


def from_stats64(stats, norm_vars=True):
    """The accumulator rule in float64 numpy, rounded once: (shift, scale) float32."""
    st = np.asarray(stats, dtype=np.float64)
    mean = st[0, :-1] / st[0, -1]
    var = np.maximum(st[1, :-1] / st[0, -1] - mean * mean, 1e-20)
    return (-mean).astype(np.float32), (1.0 / np.sqrt(var) if norm_vars else np.ones_like(var)).astype(np.float32)


def restate_global(x, valid, shift, scale, pad=0.0):
    """(x + shift) * scale in numpy float32 over the live frames, `pad` behind them: x float32 [B, rows, T] (CT)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.full_like(x, np.float32(pad))
    sh, sc = np.asarray(shift, dtype=np.float32)[:, None], np.asarray(scale, dtype=np.float32)[:, None]
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            V = int(valid[k])
            y[k, :, :V] = (x[k, :, :V] + sh) * sc
    return y


def _ordered(xs, G, a, b):
    """The sum over [a, b) of the float64 terms xs [rows, V] in the ORDER of claxon_hip.h, G [rows, groups] the group sums."""
    ka, kb = -(-a // GROUP), b // GROUP
    S = np.zeros(xs.shape[0], dtype=np.float64)
    if ka <= kb:
        for u in range(a, GROUP * ka):
            S = S + xs[:, u]
        for g in range(ka, kb):
            S = S + G[:, g]
        for u in range(GROUP * kb, b):
            S = S + xs[:, u]
    else:
        for u in range(a, b):
            S = S + xs[:, u]
    return S


def _group_sums(xs):
    """G[k] = the sum of xs[:, 32 k .. min(32 k + 32, V)) ascending from +0.0."""
    rows, V = xs.shape
    ng = -(-V // GROUP)
    padded = np.zeros((rows, ng * GROUP), dtype=np.float64)
    padded[:, :V] = xs                                       # (+0.0 behind V changes no sum that started at +0.0)
    padded = padded.reshape(rows, ng, GROUP)
    G = np.zeros((rows, ng), dtype=np.float64)
    for j in range(GROUP):
        G = G + padded[:, :, j]
    return G


def restate_sliding(x, valid, window_, min_window, center, norm_vars, pad=0.0):
    """The definition in numpy, in the stated order and with the stated roundings: x float32 [B, rows, T] (CT).  Returns y."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, rows, T = x.shape
    y = np.full_like(x, np.float32(pad))
    with np.errstate(all="ignore"):
        for k in range(B):
            V = int(valid[k])
            if V == 0:
                continue
            xs = x[k, :, :V].astype(np.float64)
            sq = xs * xs                                     # (exact: 24-bit factors)
            G, H = _group_sums(xs), _group_sums(sq)
            for t in range(V):
                a, b = window(t, V, window_, min_window, center)
                n = np.float64(b - a)
                m = _ordered(xs, G, a, b) / n
                yv = xs[:, t] - m
                if norm_vars and b - a > 1:
                    v = _ordered(sq, H, a, b) / n - m * m
                    v = np.where(v < VAR_FLOOR, VAR_FLOOR, v)
                    yv = yv / np.sqrt(v)
                y[k, :, t] = yv.astype(np.float32)
    return y


def reference_sliding(x, valid, window_, min_window, center, norm_vars, pad=0.0):
    """The definition with exact sums (math.fsum: rounded once) and float64 arithmetic, no float32 rounding: x [B, rows, T].
    Returns (y, allow, vmin): the float64 cells, DESIGN.md 4.22's bound on |cell - y| for an implementation whose sums are within
    n * 2^-53 of exact relative to the sum of their terms' magnitudes and whose other operations are one rounding each (0 for a
    padding cell; inf where the variance's interval reaches the floor), and the smallest variance met (inf without norm_vars)."""
    x = np.asarray(x, dtype=np.float64)
    B, rows, T = x.shape
    y = np.full(x.shape, float(np.float32(pad)))
    allow = np.zeros(x.shape)
    vmin = math.inf
    tiny = 2.0 ** -149
    u = U64
    for k in range(B):
        V = int(valid[k])
        for t in range(V):
            a, b = window(t, V, window_, min_window, center)
            n = b - a
            for r in range(rows):
                seg = x[k, r, a:b]
                mag = math.fsum(np.abs(seg))
                m = math.fsum(seg) / n
                dm = (n + 1) * u * mag / n * (1 + 4 * u)                       # the sum, then the division
                ys = x[k, r, t] - m
                dy = dm + u * (abs(ys) + dm)                                   # the subtraction
                if norm_vars and n > 1:
                    e2 = math.fsum(seg * seg) / n
                    v = e2 - m * m
                    # Q / n, m * m (from an m that is off by dm), their difference: the cancellation is the e2 + m^2 against v
                    dv = (n + 2) * u * e2 + (2 * abs(m) * dm + dm * dm) * (1 + u) + u * m * m + u * (abs(v) + (n + 2) * u * e2 + u * m * m)
                    vmin = min(vmin, v)
                    if v - dv <= VAR_FLOOR:
                        if v + dv >= VAR_FLOOR:
                            y[k, r, t], allow[k, r, t] = ys / math.sqrt(max(v, VAR_FLOOR)), math.inf
                            continue
                        v, dv = VAR_FLOOR, 0.0
                    s = math.sqrt(v)
                    ds = dv / (2 * math.sqrt(v - dv)) + u * (s + dv / (2 * math.sqrt(v - dv)))
                    q = ys / s
                    dq = (dy * s + abs(ys) * ds) / (s * (s - ds))
                    dy = dq + u * (abs(q) + dq)                                # the division
                    ys = q
                y[k, r, t] = ys
                allow[k, r, t] = dy + U32 * (abs(ys) + dy) + tiny              # the rounding to float32
    return y, allow, vmin
