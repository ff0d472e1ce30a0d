"""Loader for the wave simulator build of the partitioned FFT reverberator (tests/wavesim/sim_reverb_fft.cpp): clx_reverb_fft.hip's
argument checks, its plan of the call's transforms, its table and its kernels -- with clx_add's sum kernels and clx_reverb's gain
and scale kernels behind them -- as clx_reverb_windows_fft runs them, on host buffers.  Also the definition of claxon_hip.h twice
over: restate(), numpy in the stated schedule (the twiddle table the kernels get, the eleven radix-2 stages, the ascending sum over
the partitions, the mirror, the scaling) with simlib_add's fma32 and the ordered sums, which the simulator and the GPU equal bit for
bit, and reference(), which is simlib_reverb.reference itself (float64 np.convolve), with the normwise bound DESIGN.md 4.19 derives
around it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib
import simlib_add as sa
import simlib_reverb as sr

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_reverb_fft.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
U = sr.U
reference = sr.reference


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_reverb_fft.cpp", "wavesim.h")] \
        + [os.path.join(simlib._CSRC, f) for f in ("clx_norm.hip", "clx_add.hip", "clx_reverb.hip", "clx_reverb_fft.hip")] \
        + [os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: every add, multiply and divide is rounded once; fmaf is the one fused operation, and it is asked for by name
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_reverb_fft.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        _lib.sim_rvfft_windows.argtypes = [vp, sz, u32, u32, vp, vp, sz, u32, vp, vp, u32, C.c_int, u32, u32, u32, vp, vp, C.POINTER(C.c_int),
                                           C.POINTER(C.c_uint64), C.POINTER(u32)]
        _lib.sim_rvfft_error.restype = C.c_char_p
        _lib.sim_rvfft_twiddles.argtypes = [vp]
        _lib.sim_rvfft_twiddles.restype = None
        for f in ("hop", "n", "bins", "spec", "lds_bytes", "win_bytes"):
            getattr(_lib, "sim_rvfft_" + f).restype = u32
    return _lib


HOP, N, BINS, SPEC = (getattr(lib(), "sim_rvfft_" + f)() for f in ("hop", "n", "bins", "spec"))   # the kernel's own constants
LOG = N.bit_length() - 1
LAST = {}                                # the last launch: slots of the workspace, partitions transformed


def twiddles():
    """The table the kernels get, [N / 2, 2] float32 (re, im): built by the host code under test, in double, rounded once."""
    tw = np.zeros((N // 2, 2), dtype=np.float32)
    lib().sim_rvfft_twiddles(tw.ctypes.data)
    return tw


def _ptr(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def reverb_windows(data, valid, ir, ir_len, ir_index, layout, out, keep_power=None, gains=None, shape=None, n_ir=None, K=None, reserved=0, reserved2=0):
    """clx_reverb_windows_fft under the simulator, with simlib_reverb.reverb_windows' arguments; keep_power None: opts NULL, else
    opts = { keep_power, { reserved, 0, reserved2 } }.  Returns whether the kernels were launched."""
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
    launched, slots, jobs = C.c_int(0), C.c_uint64(0), C.c_uint32(0)
    st = lib().sim_rvfft_windows(_ptr(data), B, rows, T, _ptr(valid), _ptr(ir), n_ir, K, _ptr(ir_len), _ptr(ir_index), layout,
                                 0 if keep_power is None else 1, int(keep_power or 0), reserved, reserved2, _ptr(out), _ptr(gains),
                                 C.byref(launched), C.byref(slots), C.byref(jobs))
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_rvfft_error().decode())
    LAST.update(slots=int(slots.value), jobs=int(jobs.value))
    return bool(launched.value)


_REV = np.array([int(format(n, "0%db" % LOG)[::-1], 2) for n in range(N)])
_TW = None


def _stages(re, im, inverse):
    """The eleven stages of the header over [.., N] float32 words in bit-reversed order, in place."""
    global _TW
    if _TW is None:
        _TW = twiddles()
    i = np.arange(N // 2)
    for s in range(1, LOG + 1):
        half = 1 << (s - 1)
        k = i & (half - 1)
        lo = ((i - k) << 1) + k
        hi = lo + half
        wx, wy = _TW[k << (LOG - s), 0], _TW[k << (LOG - s), 1]
        if inverse:
            wy = -wy
        ux, uy, vx, vy = re[..., lo], im[..., lo], re[..., hi], im[..., hi]
        tx = sa.fma32(wx, vx, -(wy * vy))
        ty = sa.fma32(wx, vy, wy * vx)
        re[..., lo], im[..., lo], re[..., hi], im[..., hi] = ux + tx, uy + ty, ux - tx, uy - ty


def forward(words):
    """The kept bins 0 .. N / 2 of the transforms of [.., N] real float32 words: (re, im)."""
    w = np.asarray(words, dtype=np.float32)
    re, im = np.zeros_like(w), np.zeros_like(w)
    re[..., _REV] = w
    _stages(re, im, False)
    return re[..., :BINS].copy(), im[..., :BINS].copy()


def fft_row(h, x):
    """One row's cells: x [V] float32 convolved with the live taps h [min(L, V)] by the header's overlap-save."""
    x, h = np.asarray(x, dtype=np.float32), np.asarray(h, dtype=np.float32)
    V = x.size
    nb, npart = -(-V // HOP), -(-h.size // HOP)
    xp = np.zeros((nb + 1) * HOP, dtype=np.float32)
    xp[HOP:HOP + V] = x
    seg = np.stack([xp[s * HOP:s * HOP + N] for s in range(nb)])
    hp = np.zeros((npart, N), dtype=np.float32)
    for p in range(npart):
        n = min(HOP, h.size - p * HOP)
        hp[p, :n] = h[p * HOP:p * HOP + n]
    Xr, Xi = forward(seg)
    Hr, Hi = forward(hp)
    y = np.zeros(nb * HOP, dtype=np.float32)
    for b in range(nb):
        ar = sa.fma32(Xr[b], Hr[0], -(Xi[b] * Hi[0]))
        ai = sa.fma32(Xr[b], Hi[0], Xi[b] * Hr[0])
        for p in range(1, min(b + 1, npart)):
            ar = sa.fma32(-Xi[b - p], Hi[p], sa.fma32(Xr[b - p], Hr[p], ar))
            ai = sa.fma32(Xi[b - p], Hr[p], sa.fma32(Xr[b - p], Hi[p], ai))
        fr, fi = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
        fr[:BINS], fi[:BINS] = ar, ai
        fr[BINS:], fi[BINS:] = ar[N - np.arange(BINS, N)], -ai[N - np.arange(BINS, N)]
        re, im = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
        re[_REV], im[_REV] = fr, fi
        _stages(re, im, True)
        y[b * HOP:(b + 1) * HOP] = re[HOP:] * np.float32(1.0 / N)
    return y[:V]


def restate(x, valid, ir, ir_len, ir_index, keep_power):
    """The definition in numpy, in the stated schedule and with the stated roundings: x [B, rows, T] float32 (CT), ir [N, K].
    Returns (y, gains)."""
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
            if v == 0:
                continue
            for r in range(rows):
                y[k, r, :v] = fft_row(ir[j, :min(L, v)], x[k, r, :v])
            if not keep_power:
                continue
            ex, ey = sr._energy(x[k], v), sr._energy(y[k], v)
            if ex == 0.0 or ey == 0.0:
                continue
            g = np.float32(np.sqrt(ex / ey))
            gains[k] = g
            if g != 1:
                y[k, :, :v] = y[k, :, :v] * g
    return y, gains


# ---- the bound of DESIGN.md 4.19 ---------------------------------------------------------------------------------------------------

ETA = 7 * U                              # Higham's eta = mu + gamma_4 (sqrt 2 + mu) for twiddles within mu = u: below 7 u
EPS_F = LOG * ETA / (1 - LOG * ETA)      # one transform's relative 2-norm error


def c_of(P):
    """c(N, P) of DESIGN.md 4.19, in units of u: |e_t| <= c u sum_p ||x_seg[b - p]||_2 ||h_p||_2."""
    g2p = 2 * P * U / (1 - 2 * P * U)
    rho = math.sqrt(2) * (2 * EPS_F + EPS_F ** 2 + math.sqrt(2) * g2p * (1 + EPS_F) ** 2)
    return math.sqrt(N) * (rho + EPS_F * (1 + rho)) / U


def cell_bound(x, valid, ir, ir_len, ir_index):
    """per cell of the unscaled output the bound c(N, P) u S_b + the subnormal term, S_b the sum over the block's
    partitions of ||x_seg[b - p]||_2 ||h_p||_2; 0 where the cell is a copy or padding.  [B, rows, T] float64."""
    x64 = np.asarray(x, dtype=np.float64)
    B, rows, T = x64.shape
    bound = np.zeros(x64.shape)
    nu = 2.0 ** -149
    for k in range(B):
        j, v = int(ir_index[k]), int(valid[k])
        L = int(ir_len[j]) if j >= 0 else 0
        lv = min(L, v)
        if lv == 0:
            continue
        h = np.asarray(ir[j, :lv], dtype=np.float64)
        npart, nb = -(-lv // HOP), -(-v // HOP)
        hn2 = [math.sqrt(float((h[p * HOP:(p + 1) * HOP] ** 2).sum())) for p in range(npart)]
        hn1 = [float(np.abs(h[p * HOP:(p + 1) * HOP]).sum()) for p in range(npart)]
        for r in range(rows):
            xp = np.zeros((nb + 1) * HOP)
            xp[HOP:HOP + v] = x64[k, r, :v]
            xn2 = [math.sqrt(float((xp[s * HOP:s * HOP + N] ** 2).sum())) for s in range(nb)]
            xn1 = [float(np.abs(xp[s * HOP:s * HOP + N]).sum()) for s in range(nb)]
            for b in range(nb):
                ps = range(min(b + 1, npart))
                S = sum(xn2[b - p] * hn2[p] for p in ps)
                sub = nu * (sum(6 * N * (hn1[p] + xn1[b - p]) + 4 for p in ps) + 4)
                bound[k, r, b * HOP:min((b + 1) * HOP, v)] = c_of(len(ps)) * U * S + sub
    return bound


def gain_rel(y64, e, valid):
    """DESIGN.md 4.18's bound on |g / g64 - 1| per window with the cell error e of this method (simlib_reverb.gain_rel with
    cell_bound replaced)."""
    rel = np.zeros(y64.shape[0])
    for k, v in enumerate(valid):
        ey = math.fsum((y64[k, :, :v] ** 2).reshape(-1))
        d = math.fsum((2 * np.abs(y64[k, :, :v]) * e[k, :, :v] + e[k, :, :v] ** 2).reshape(-1)) / ey if ey > 0 else 0.0
        assert d < 0.5, d
        rel[k] = (1 + U) * (1 + 2.0 ** -40) * (1 + d / (2 * (1 - d))) - 1 + U
    return rel


def scaled_bound(out, y64, g64, e, g_rel):
    """DESIGN.md 4.18's scaled_bound with the cell error e of this method."""
    g, r = g64[:, None, None], g_rel[:, None, None]
    return g * (1 + r) * e + r * np.abs(g * y64) + U * np.abs(np.asarray(out, dtype=np.float64)) + 2.0 ** -149
