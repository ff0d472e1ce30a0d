"""Loader for the wave simulator build of the several-noise mixer (tests/wavesim/sim_addn.cpp): clx_addn.hip's argument checks, its
table and its kernels as clx_addn_windows runs them, on host buffers.  Also the definition of claxon_hip.h twice over: restate(),
numpy in the stated order of the sums and with the stated roundings (simlib_add's exact fmaf), which the simulator and the GPU
equal bit for bit, and reference(), the same in float64 with exact sums (math.fsum) and no float32 rounding, with the bounds
DESIGN.md 4.25 derives around it.

A window's terms are a list of (batch, index, offset, loop, snr_db) tuples; a call's terms a list of such lists."""
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
_SO = os.path.join(_DIR, "libwavesim_addn.so")

TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
CHUNK, STRANDS, MAX_ROWS, MAX_TERMS, MAX_BATCHES = sn.CHUNK, sn.STRANDS, 8, 16, 8
GAIN_REL = sa.GAIN_REL                   # |g / g_ref - 1| stays below this, as in DESIGN.md 4.17: the gain's arithmetic is the same
# every intermediate of a cell's chain stays below (1 + CHAIN_SLACK) (|x| + sum |g_ref n|): the gains are within
# 2^-23, at most 16 roundings of 2^-24 each, (1 + 2^-23) (1 + 2^-24)^16 < 1 + 2^-19
CHAIN_SLACK = 2.0 ** -19


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_addn.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, f) for f in ("clx_norm.hip", "clx_add.hip", "clx_addn.hip")] \
        + [os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: every add, multiply and divide is rounded once; fmaf is the one fused operation, and it is asked for by name
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_addn.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        _lib.sim_addn_windows.argtypes = [vp, sz, u32, u32, vp, vp, vp, u32, vp, vp, vp, u32, C.c_int, u32, vp, C.POINTER(C.c_int)]
        _lib.sim_addn_error.restype = C.c_char_p
        for f in ("max_terms", "max_batches", "max_rows", "rec_bytes", "term_bytes"):
            getattr(_lib, "sim_addn_" + f).restype = u32
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def flatten(terms):
    """(term_first uint32 [B + 1], the terms as a cx.ADDN_TERM_DTYPE array) of a call's list of per-window term lists."""
    first = np.zeros(len(terms) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([len(t) for t in terms])
    flat = np.zeros(int(first[-1]), dtype=cx.ADDN_TERM_DTYPE)
    for m, t in enumerate(t for w in terms for t in w):
        flat[m] = (t[0], t[1], t[2], int(t[3]), t[4])
    return first, flat


def addn_windows(data, valid, noises, noise_valid, term_first, terms, layout, gains=None, shape=None, n_noise=None, reserved=None, n_batches=None,
                 null_counts=False):
    """clx_addn_windows under the simulator: `data` (a float32 array, [B, rows, T] for CT and [B, T, rows] for TC, or any float32
    buffer with shape=(B, rows, T)) mixed in place with the batches of `noises` (a list of arrays [N_b, ...] alike, or of buffers
    with n_noise=[N_b, ...]; None: a null pointer, and a None in it a null batch); noise_valid is one array over all batches,
    term_first and terms what flatten() gives; reserved None: opts NULL, else opts->reserved; null_counts: n_noise is a null
    pointer.  Returns whether the kernels were launched."""
    if shape is None:
        B = data.shape[0]
        rows, T = (data.shape[2], data.shape[1]) if layout == TC else (data.shape[1], data.shape[2])
    else:
        B, rows, T = shape
    if n_noise is None:
        n_noise = [n.shape[0] for n in noises]
    if n_batches is None:
        n_batches = len(n_noise)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    noise_valid = None if noise_valid is None else np.ascontiguousarray(noise_valid, dtype=np.uint32)
    term_first = None if term_first is None else np.ascontiguousarray(term_first, dtype=np.uint32)
    terms = None if terms is None else np.ascontiguousarray(terms, dtype=cx.ADDN_TERM_DTYPE)
    for a in [data, gains] + list(noises or []):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.dtype == np.float32)
    ptrs = None
    if noises is not None:
        ptrs = (C.c_void_p * max(len(noises), 1))()
        for b, n in enumerate(noises):
            ptrs[b] = _ptr(n)
    counts = None if null_counts else (C.c_size_t * max(len(n_noise), 1))(*n_noise)
    launched = C.c_int(0)
    st = lib().sim_addn_windows(_ptr(data), B, rows, T, _ptr(valid), ptrs, counts, n_batches, _ptr(noise_valid), _ptr(term_first), _ptr(terms),
                                layout, 0 if reserved is None else 1, reserved or 0, _ptr(gains), C.byref(launched))
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_addn_error().decode())
    return bool(launched.value)


def cover(term, vs, noise_valids):
    """(off, end, P) of a term in a window with vs live samples; end == off: the cover is empty (or the term names no noise)."""
    b, j, off, loop, _ = term
    if j < 0:
        return off, off, 0
    P = int(noise_valids[b][j])
    if off >= vs or P == 0:
        return off, off, P
    return off, (vs if loop else min(vs, off + P)), P


def _heard(noise, off, end, P):
    """[rows, Nc]: the noise samples the term reads, in the order of i = t - off."""
    return noise[:, np.arange(end - off) % P]


def restate(x, valid, noises, noise_valids, terms):
    """The definition in numpy, in the stated order and with the stated roundings: x [B, rows, T] and the noises [N_b, rows, T]
    float32 (CT).  Returns (y, gains [M]); cells that the definition leaves alone keep x's words."""
    x = np.asarray(x, dtype=np.float32)
    y = x.copy()
    gains = []
    with np.errstate(all="ignore"):
        for k, window in enumerate(terms):
            vs = int(valid[k])
            es = None
            for term in window:
                off, end, P = cover(term, vs, noise_valids)
                q = sa.ratio(term[4])
                g = np.float32(0.0)
                if end > off and q != 0.0:
                    if es is None:
                        es = sa._energy(x[k], vs)
                    nc = end - off
                    heard = _heard(noises[term[0]][term[1]], off, end, P)
                    en = sa._energy(heard, nc)
                    if es != 0.0 and en != 0.0:
                        g = np.float32(np.sqrt((es * np.float64(nc) * np.float64(q)) / (en * np.float64(vs))))
                    if g != 0:
                        y[k, :, off:end] = sa.fma32(g, heard, y[k, :, off:end])
                gains.append(g)
    return y, np.array(gains, dtype=np.float32)


def reference(x, valid, noises, noise_valids, terms):
    """The definition in float64 with exact sums (math.fsum of squares that are exact in float64) and no rounding to float32.
    Returns (y [B, rows, T] float64, g [M] float64, gn [B, rows, T]: the sum of |g n| over the terms that reach the cell, cnt
    [B, rows, T]: how many do)."""
    x64 = np.asarray(x, dtype=np.float64)
    y, gn, cnt, gs = x64.copy(), np.zeros(x64.shape), np.zeros(x64.shape, dtype=np.int64), []
    for k, window in enumerate(terms):
        vs = int(valid[k])
        for term in window:
            off, end, P = cover(term, vs, noise_valids)
            q = sa.ratio(term[4])
            g = 0.0
            if end > off and q != 0.0:
                nc = end - off
                heard = _heard(np.asarray(noises[term[0]][term[1]], dtype=np.float64), off, end, P)
                s = x64[k, :, :vs].reshape(-1)
                es, en = math.fsum(s * s), math.fsum(heard.reshape(-1) ** 2)
                if es != 0.0 and en != 0.0:
                    g = math.sqrt((es / vs) / (en / nc) * q)
                    y[k, :, off:end] += g * heard
                    gn[k, :, off:end] += np.abs(g * heard)
                    cnt[k, :, off:end] += 1
            gs.append(g)
    return y, np.array(gs), gn, cnt


def cell_bound(x, gn, cnt):
    """a cell that S terms reach is S fused multiply-adds behind the reference.  Step s rounds once: an error of at
    most 2^-24 |y_s| + 2^-149, which the later steps carry unchanged; |y_s| <= (1 + 2^-19) (|x| + sum |g_ref n|).  The gains add
    2^-23 sum |g_ref n| (4.17).  So |out - reference| <= S (2^-24 (1 + 2^-19) (|x| + gn) + 2^-149) + 2^-23 gn."""
    a = np.abs(np.asarray(x, dtype=np.float64)) + gn
    return cnt * (sn.U32 * (1.0 + CHAIN_SLACK) * a + 2.0 ** -149) + GAIN_REL * gn
