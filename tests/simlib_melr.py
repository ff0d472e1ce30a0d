"""Loader for the wave simulator build of the reflected mel specs (tests/wavesim/sim_melr.cpp): clx_mel.hip's reflected table builder,
its argument checks, the count rule and clx_k_mel_fr / clx_k_mel_qr as clx_mel_create_reflected / clx_mel_windows run them, beside the
snipped siblings with the same tables, on host buffers; and the definition's index map -- Kaldi's loop, written out -- with the batch
of explicitly reflected windows that a whole-frame spec turns into the same frames.  The simulator and the GPU tests share it."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib
from simlib_mel import CT, LN, LOG10, POWER, TC  # noqa: F401

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_melr.so")
KERNELS = ("clx_k_mel", "clx_k_mel_f", "clx_k_mel_q", "clx_k_mel_fr", "clx_k_mel_qr")


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_melr.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_mel.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: the conditioning's steps, the energy's folds and the lifter product are each rounded once, as on the GPU
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_melr.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_melr_create.argtypes = [C.c_int, u32, u32, u32, vp, vp, u32, u32, u32, f32, C.c_int, u32, u32, f32, C.c_int, u32, vp, vp, u32, f32, f32]
        _lib.sim_melr_destroy.argtypes = [C.c_int]
        _lib.sim_melr_destroy.restype = None
        _lib.sim_melr_kernel.argtypes = [C.c_int]
        _lib.sim_melr_rows.argtypes = [C.c_int]
        _lib.sim_melr_rows.restype = u32
        _lib.sim_melr_origin.argtypes = [C.c_int]
        _lib.sim_melr_origin.restype = C.c_int32
        _lib.sim_melr_table_words.argtypes = [C.c_int, vp]
        _lib.sim_melr_table_words.restype = sz
        _lib.sim_melr_windows.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, vp, vp]
        _lib.sim_melr_guarded.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, C.c_int, vp]
        _lib.sim_melr_error.restype = C.c_char_p
        _lib.sim_melr_lds_bytes.restype = u32
    return _lib


def _check(st):
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_melr_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data


def create(n_fft, win_length, hop, window, fbank, n_bins, n_mels, mode, floor, opts=None, cep=None, reflected=True):
    """clx_mel_create_reflected under the simulator (reflected=False: the snipped sibling, clx_mel_create_cepstral with `cep`, else
    clx_mel_create_framed): the spec's number.  opts is None (a NULL pointer) or a dict with any of remove_dc, whole_frames, preemph
    (the rest zero).  cep is None (a NULL pointer: an fbank spec) or a dict with any of n_ceps, dct, lifter, energy, energy_scale,
    energy_floor (the rest: n_ceps 1, no table, 0, 1.0, 0.0)."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    window, fbank = f32(window), f32(fbank)
    o = dict(remove_dc=0, whole_frames=0, preemph=0.0)
    o.update(opts or {})
    q = dict(n_ceps=1, dct=None, lifter=None, energy=0, energy_scale=1.0, energy_floor=0.0)
    q.update(cep or {})
    dct, lifter = f32(q["dct"]), f32(q["lifter"])
    h = lib().sim_melr_create(1 if reflected else 0, n_fft, win_length, hop, _ptr(window), _ptr(fbank), n_bins, n_mels, mode, floor,
                              0 if opts is None else 1, o["remove_dc"], o["whole_frames"], o["preemph"], 0 if cep is None else 1,
                              q["n_ceps"], _ptr(dct), _ptr(lifter), q["energy"], q["energy_scale"], q["energy_floor"])
    if h < 0:
        _check(cx.API_ERROR)
    return h


def destroy(h):
    lib().sim_melr_destroy(h)


def kernel(h):
    """The kernel clx_mel_windows launches for the spec."""
    return KERNELS[lib().sim_melr_kernel(h)]


def rows(h):
    """The rows of the spec's output: n_ceps of a cepstral spec, else n_mels."""
    return int(lib().sim_melr_rows(h))


def origin(h):
    """The index of frame 0's tap 0 as the launch passes it."""
    return int(lib().sim_melr_origin(h))


def table_words(h):
    """The spec's basis, filterbank, row ends, dct and lifter as the builder left them, as one uint32 array."""
    n = lib().sim_melr_table_words(h, None)
    out = np.zeros(n, dtype=np.uint32)
    lib().sim_melr_table_words(h, out.ctypes.data)
    return out


def mel_windows(h, audio, valid, n_frames, layout, out, shape=None, tables=False):
    """clx_mel_windows under the simulator, `out` written in place.  tables=True: returns (out, valid_frames)."""
    B, L = shape if shape is not None else audio.shape
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    for a in (audio, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.itemsize == 4)
    vf = np.zeros(max(B, 1), np.uint32)
    _check(lib().sim_melr_windows(h, _ptr(audio), B, L, _ptr(valid), n_frames, layout, _ptr(out), vf.ctypes.data))
    return (out, vf[:B]) if tables else out


def mel_guarded(h, audio, valid, n_frames, layout, at_end, out):
    """The batch read from where an inaccessible page follows its last float (at_end) or precedes its first."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    valid = np.ascontiguousarray(valid, dtype=np.uint32)
    _check(lib().sim_melr_guarded(h, a.ctypes.data, a.shape[0], a.shape[1], valid.ctypes.data, n_frames, layout, 1 if at_end else 0,
                                  out.ctypes.data))
    return out


# ---- the definition, independently of the library ---------------------------------------------------------------------------------

def count(valid, H, n_frames):
    """min(n_frames, (V + H // 2) // H)."""
    v = np.asarray(valid, dtype=np.int64)
    return np.minimum((v + H // 2) // H, int(n_frames))


def kaldi_index(i, V):
    """Kaldi's loop of feature-window.cc (ExtractWindow, snip_edges=false) on an array of indices, for V >= 1: while an index is
    outside [0, V) it becomes -i - 1 if it is negative and 2 V - 1 - i otherwise."""
    i = np.array(i, dtype=np.int64)
    assert V >= 1
    while True:
        low, high = i < 0, i >= V
        if not (low.any() or high.any()):
            return i
        i = np.where(low, -i - 1, np.where(high, 2 * V - 1 - i, i))


def reflected_batch(a, valid, Nw, H, n_frames):
    """(p [B, Lp] float32, valid_p, counts): for every window p[k][i] = a[k][r(i + H // 2 - Nw // 2)] for i < (T_k - 1) H + Nw, T_k the
    window's live frame count, zeros behind; Lp = (n_frames - 1) H + Nw, valid_p[k] = (T_k - 1) H + Nw (0 for T_k = 0): frame t of a
    whole-frame spec on p[k] is frame t of the reflected spec on a[k], and it counts T_k frames."""
    a = np.asarray(a, dtype=np.float32)
    T = count(valid, H, n_frames)
    Lp = (int(n_frames) - 1) * H + Nw
    p = np.zeros((a.shape[0], Lp), dtype=np.float32)
    vp = np.zeros(a.shape[0], dtype=np.uint32)
    for k in range(a.shape[0]):
        if T[k] > 0:
            n = (int(T[k]) - 1) * H + Nw
            p[k, :n] = a[k][kaldi_index(np.arange(n, dtype=np.int64) + (H // 2 - Nw // 2), int(valid[k]))]
            vp[k] = n
    return p, vp, T
