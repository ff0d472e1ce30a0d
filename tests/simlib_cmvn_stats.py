"""Loader for the wave simulator build of the CMVN accumulator and the grouped normalisation (tests/wavesim/sim_cmvn_stats.cpp):
clx_cmvn_stats.hip's argument checks, its per-call table and its five kernels as clx_cmvn_stats_windows and
clx_cmvn_grouped_windows run them, on host buffers; its chunk partials beside clx_norm's own; its solve alone.  Also the
definition of claxon_hip.h twice over: restate_stats() and restate_grouped(), numpy in the stated ORDER and precisions, which the
simulator and the GPU equal word for word; and exact(), the sums rounded once from exact arithmetic (math.fsum over the cells and
over their exact float64 squares), with bound(), DESIGN.md 4.24's bound of the ordered sums against them."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_cmvn_stats.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
THREADS, CHUNK, STRANDS, VECS, MAX_GROUPS = 256, 4096, 64, 1024, 65536
SUM_LDS_BYTES, SUM_TC_LDS_BYTES, FOLD_LDS_BYTES, SOLVE_LDS_BYTES, APPLY_LDS_BYTES = 0, 4352, 0, 0, 0
U64 = 2.0 ** -53                         # the unit roundoff of float64
VAR_FLOOR = 1e-20


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_cmvn_stats.cpp", "wavesim.h")] + \
           [os.path.join(simlib._CSRC, f) for f in ("clx_norm.hip", "clx_cmvn.hip", "clx_cmvn_stats.hip")] + \
           [os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: every add, multiply and divide is rounded once, as the helpers of the three files are on the GPU
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_cmvn_stats.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_cmvn_stats_windows.argtypes = [vp, sz, u32, u32, vp, u32, vp, u32, vp, C.c_int, u32, u32]
        _lib.sim_cmvn_grouped_windows.argtypes = [vp, sz, u32, u32, vp, u32, vp, u32, vp, vp, C.c_int, u32, f32, u32]
        _lib.sim_cmvn_stats_solve.argtypes = [vp, u32, u32, u32, vp]
        _lib.sim_cmvn_stats_solve.restype = None
        _lib.sim_cmvn_stats_partials.argtypes = [vp, sz, u32, u32, vp, u32, vp, vp]
        _lib.sim_cmvn_stats_table.argtypes = [vp, sz, vp, vp, u32]
        _lib.sim_cmvn_stats_shape.argtypes = [vp]
        _lib.sim_cmvn_stats_error.restype = C.c_char_p
        for f in ("threads", "chunk", "strands", "vecs", "max_groups", "sum_lds_bytes", "sum_tc_lds_bytes", "fold_lds_bytes", "solve_lds_bytes",
                  "apply_lds_bytes", "launch_count"):
            getattr(_lib, "sim_cmvn_stats_" + f).restype = u32
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _dims(data, layout, shape):
    if shape is not None:
        return shape
    return (data.shape[0],) + ((data.shape[2], data.shape[1]) if layout == TC else (data.shape[1], data.shape[2]))


def _raise():
    raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_cmvn_stats_error().decode())


def _i32(groups):
    return None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)


def launches():
    """Kernels the simulator has launched so far."""
    return int(lib().sim_cmvn_stats_launch_count())


def last_shape():
    """(n_chunks, tc, sum_blocks, n_tiles, solve_blocks, partials, table words, present groups) of the last simulated call that launched."""
    a = np.zeros(8, dtype=np.uint32)
    lib().sim_cmvn_stats_shape(a.ctypes.data)
    return tuple(int(v) for v in a)


def stats_windows(data, valid, layout, groups, n_groups, stats, accumulate=True, shape=None, opts=True, reserved=0):
    """clx_cmvn_stats_windows under the simulator: `data` a float32 array ([B, rows, T] for CT, [B, T, rows] for TC, or any float32
    buffer with shape=(B, rows, T)), `stats` a float64 buffer of n_groups * 2 * (rows + 1) words, updated in place; groups an int
    sequence or None (NULL); opts=False: opts is NULL.  Returns stats."""
    B, rows, T = _dims(data, layout, shape)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    groups = _i32(groups)
    assert data is None or (data.flags["C_CONTIGUOUS"] and data.dtype == np.float32)
    assert stats is None or isinstance(stats, int) or (stats.flags["C_CONTIGUOUS"] and stats.dtype == np.float64)
    s_ptr = stats if isinstance(stats, int) else _ptr(stats)
    if lib().sim_cmvn_stats_windows(_ptr(data), B, rows, T, _ptr(valid), layout, _ptr(groups), n_groups, s_ptr, 1 if opts else 0, int(accumulate),
                                    reserved) != cx.OK:
        _raise()
    return stats


def grouped_windows(data, valid, layout, groups, n_groups, stats, ss, norm_vars=True, pad=0.0, shape=None, opts=True, reserved=0):
    """clx_cmvn_grouped_windows under the simulator: `data` normalised in place, `stats` float64 [n_groups][2][rows + 1] only read,
    `ss` a float32 buffer of n_groups * 2 * rows words that receives the shifts and scales.  Returns data."""
    B, rows, T = _dims(data, layout, shape)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    groups = _i32(groups)
    assert data is None or (data.flags["C_CONTIGUOUS"] and data.dtype == np.float32)
    s_ptr = stats if isinstance(stats, int) or stats is None else _ptr(stats)
    ss_ptr = ss if isinstance(ss, int) or ss is None else _ptr(ss)
    if lib().sim_cmvn_grouped_windows(_ptr(data), B, rows, T, _ptr(valid), layout, _ptr(groups), n_groups, s_ptr, ss_ptr, 1 if opts else 0,
                                      int(norm_vars), pad, reserved) != cx.OK:
        _raise()
    return data


def solve(stats, norm_vars=True):
    """clx_k_cmvn_stats_solve under the simulator: stats float64 [G, 2, rows + 1] -> float32 [G, 2, rows] (shifts, scales)."""
    st = np.ascontiguousarray(stats, dtype=np.float64)
    G, rows = st.shape[0], st.shape[2] - 1
    ss = np.zeros((G, 2, rows), dtype=np.float32)
    lib().sim_cmvn_stats_solve(st.ctypes.data, G, rows, int(norm_vars), ss.ctypes.data)
    return ss


def partials(data, valid, layout, shape=None):
    """(this file's chunk partials, clx_norm's own sum kernel's) over the same data, both float64 [B, rows, 2, n_chunks] with S in
    [:, :, 0] and Q in [:, :, 1]; a word nobody wrote is NaN (clx_norm's Q half always is)."""
    B, rows, T = _dims(data, layout, shape)
    valid = np.ascontiguousarray(valid, dtype=np.uint32)
    nc = -(-T // CHUNK)
    mine = np.full((B, rows, 2, nc), np.nan)
    norms = np.full((B, rows, 2, nc), np.nan)
    got = lib().sim_cmvn_stats_partials(_ptr(data), B, rows, T, _ptr(valid), layout, mine.ctypes.data, norms.ctypes.data)
    if got < 0:
        _raise()
    assert got == nc
    return mine, norms


def table(valid, groups, n_groups):
    """The host's counting sort (clx_cmvn_stats_fill_table): (gid of the present groups, start, list)."""
    valid = np.ascontiguousarray(valid, dtype=np.uint32)
    n = valid.size
    groups = _i32(groups)
    tab = np.zeros(5 * n + 1, dtype=np.uint32)
    present = lib().sim_cmvn_stats_table(tab.ctypes.data, n, _ptr(valid), _ptr(groups), n_groups)
    assert present >= 0, "the work array did not come back as zeros"
    assert np.array_equal(tab[:n], valid)
    return tab[2 * n:2 * n + present].tolist(), tab[3 * n:3 * n + present + 1].tolist(), tab[4 * n + 1:4 * n + 1 + tab[3 * n + present]].tolist()


# ---- the definition in numpy ---------------------------------------------------------------------------------------------------------

_FOLD = [np.arange(STRANDS) ^ d for d in (32, 16, 8, 4, 2, 1)]


def _chunk_sum(seg):
    """S_c of the float64 terms seg [rows, n] (n <= 4096): the strands ascending from +0.0, then the xor fold; [rows]."""
    rows, n = seg.shape
    steps = -(-n // STRANDS)
    padded = np.zeros((rows, steps * STRANDS))               # (+0.0 behind the end changes no sum that started at +0.0)
    padded[:, :n] = seg
    padded = padded.reshape(rows, steps, STRANDS)
    acc = np.zeros((rows, STRANDS))
    for j in range(steps):
        acc = acc + padded[:, j, :]
    for idx in _FOLD:
        acc = acc + acc[:, idx]
    return acc[:, 0].copy()


def window_sums(xs):
    """W of the float64 terms xs [rows, V]: the chunk partials added ascending from +0.0."""
    W = np.zeros(xs.shape[0])
    for c0 in range(0, xs.shape[1], CHUNK):
        W = W + _chunk_sum(xs[:, c0:c0 + CHUNK])
    return W


def restate_stats(x, valid, groups, n_groups, stats=None, accumulate=True):
    """clx_cmvn_stats_windows in numpy, in the stated ORDER: x float32 [B, rows, T] (CT); stats float64 [G, 2, rows + 1] (None:
    zeros).  Returns the new accumulator (a copy)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, rows, T = x.shape
    acc = np.zeros((n_groups, 2, rows + 1)) if stats is None or not accumulate else np.array(stats, dtype=np.float64).reshape(n_groups, 2, rows + 1)
    groups = [0] * B if groups is None else [int(g) for g in groups]
    with np.errstate(all="ignore"):
        for k in range(B):
            g, V = groups[k], int(valid[k])
            if g < 0:
                continue
            xs = x[k, :, :V].astype(np.float64)
            acc[g, 0, :rows] = acc[g, 0, :rows] + window_sums(xs)
            acc[g, 1, :rows] = acc[g, 1, :rows] + window_sums(xs * xs)       # (exact: 24-bit factors)
            acc[g, 0, rows] = acc[g, 0, rows] + np.float64(V)
    return acc


def solve64(stats, norm_vars=True):
    """The solve as float64 numpy lines, each rounded once: stats [G, 2, rows + 1] -> float32 [G, 2, rows]."""
    st = np.asarray(stats, dtype=np.float64)
    G, rows = st.shape[0], st.shape[2] - 1
    ss = np.zeros((G, 2, rows), dtype=np.float32)
    ss[:, 1, :] = 1.0
    with np.errstate(all="ignore"):
        for g in range(G):
            count = st[g, 0, rows]
            if not count > 0.0:
                continue
            mean = st[g, 0, :rows] / count
            var = st[g, 1, :rows] / count - mean * mean
            var = np.where(var >= VAR_FLOOR, var, VAR_FLOOR)
            ss[g, 0] = (-mean).astype(np.float32)
            if norm_vars:
                ss[g, 1] = (1.0 / np.sqrt(var)).astype(np.float32)
    return ss


def restate_grouped(x, valid, groups, ss, pad=0.0):
    """(x + shift[g]) * scale[g] in numpy float32 over the live frames, `pad` behind them, group -1 kept: x float32 [B, rows, T]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.full_like(x, np.float32(pad))
    groups = [0] * x.shape[0] if groups is None else [int(g) for g in groups]
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            V, g = int(valid[k]), groups[k]
            y[k, :, :V] = x[k, :, :V] if g < 0 else (x[k, :, :V] + ss[g, 0][:, None]) * ss[g, 1][:, None]
    return y


def exact(x, valid, groups, n_groups):
    """(E, A): E float64 [G, 2, rows + 1] the accumulator with every sum taken exactly and rounded once (math.fsum over the cells,
    and over their float64 squares, which are exact), the count exact; A float64 [G, 2, rows] the sums of the terms' magnitudes."""
    x = np.asarray(x, dtype=np.float32)
    B, rows, T = x.shape
    groups = [0] * B if groups is None else [int(g) for g in groups]
    E, A = np.zeros((n_groups, 2, rows + 1)), np.zeros((n_groups, 2, rows))
    for g in range(n_groups):
        ks = [k for k in range(B) if groups[k] == g]
        E[g, 0, rows] = sum(int(valid[k]) for k in ks)
        for r in range(rows):
            cells = np.concatenate([x[k, r, :int(valid[k])].astype(np.float64) for k in ks]) if ks else np.zeros(0)
            sq = cells * cells
            E[g, 0, r], E[g, 1, r] = math.fsum(cells), math.fsum(sq)
            A[g, 0, r], A[g, 1, r] = math.fsum(np.abs(cells)), E[g, 1, r]
    return E, A


def bound(A, E, n_chunks, n_added):
    """a term of group g passes through at most d = 64 + 6 + n_chunks + n_added[g] additions (its strand, the fold,
    the window's chunks, the group's own windows -- in this call and every earlier accumulating one), so
    |sum - exact| <= d u / (1 - d u) * sum |term|; plus the one rounding of the reference itself.  n_added is one number per group."""
    d = (STRANDS + 6 + n_chunks + np.asarray(n_added, dtype=np.float64))[:, None, None]
    return d * U64 / (1.0 - d * U64) * A + U64 * np.abs(E[:, :, :-1])
