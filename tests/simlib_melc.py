"""Loader for the wave simulator build of the centred and range-scaled mel features (tests/wavesim/sim_melc.cpp): clx_mel.hip's
table builder with options, its argument checks, the table fill and the three kernels as clx_mel_create_ex / clx_mel_windows run
them, on host buffers.  The float64 reference, the tables and the log step's allowance are simlib_mel's."""
import ctypes as C
import os
import subprocess

import numpy as np

import claxon_amd as cx
import simlib
import simlib_mel
from simlib_mel import CT, LN, LOG10, LOG_ULPS, POWER, TC, hann, log_ulps, reference, triangles  # noqa: F401

_DIR = simlib._DIR
_SO = os.path.join(_DIR, "libwavesim_melc.so")

PAD_REFLECT, PAD_ZERO = 0, 1


def build(force=False):
    deps = [os.path.join(_DIR, f) for f in ("sim_melc.cpp", "wavesim.h")] + [os.path.join(simlib._CSRC, "clx_mel.hip"),
            os.path.join(_DIR, "fake", "hip", "hip_runtime.h"), os.path.join(simlib._CSRC, "..", "..", "include", "claxon_hip.h")]
    if not force and os.path.exists(_SO) and os.path.getmtime(_SO) >= max(os.path.getmtime(d) for d in deps):
        return _SO
    tmp = "%s.%d.tmp" % (_SO, os.getpid())                   # (several workers may build at once -- each to its own name, then a rename)
    # -ffp-contract=off: the range step's subtract, add and multiply are each rounded once, as __fsub_rn and its kin are on the GPU
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++",
                           "-I", os.path.join(_DIR, "fake"), "-I", simlib._CSRC, "-I", _DIR, "-o", tmp, os.path.join(_DIR, "sim_melc.cpp")])
    os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        vp, u32, sz, f32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
        _lib.sim_melc_create.argtypes = [u32, u32, vp, vp, u32, u32, f32, C.c_int, u32, u32, u32, f32, f32, f32]
        _lib.sim_melc_destroy.argtypes = [C.c_int]
        _lib.sim_melc_destroy.restype = None
        _lib.sim_melc_table_words.argtypes = [C.c_int, vp]
        _lib.sim_melc_table_words.restype = sz
        _lib.sim_melc_windows.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, vp, vp, vp]
        _lib.sim_melc_guarded.argtypes = [C.c_int, vp, sz, u32, vp, u32, u32, C.c_int, vp]
        _lib.sim_melc_error.restype = C.c_char_p
        _lib.sim_melc_lds_bytes.restype = u32
        _lib.sim_melc_range_vectors.restype = u32
        _lib.sim_melc_enc.argtypes = [f32]
        _lib.sim_melc_enc.restype = u32
        _lib.sim_melc_dec.argtypes = [u32]
        _lib.sim_melc_dec.restype = f32
    return _lib


def _check(st):
    if st != cx.OK:
        raise cx.ClaxonError(cx.API_ERROR, 0, lib().sim_melc_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data


def create(n_fft, hop, window, fbank, n_mels, mode, floor, opts=None):
    """clx_mel_create_ex under the simulator: the spec's number.  opts is None (a NULL pointer: clx_mel_create) or a dict with any
    of center, pad, range, range_width, shift, scale (the rest zero)."""
    window = None if window is None else np.ascontiguousarray(window, dtype=np.float32)
    fbank = None if fbank is None else np.ascontiguousarray(fbank, dtype=np.float32)
    o = dict(center=0, pad=0, range=0, range_width=0.0, shift=0.0, scale=0.0)
    o.update(opts or {})
    h = lib().sim_melc_create(n_fft, hop, _ptr(window), _ptr(fbank), n_mels, mode, floor, 0 if opts is None else 1, o["center"], o["pad"],
                              o["range"], o["range_width"], o["shift"], o["scale"])
    if h < 0:
        _check(cx.API_ERROR)
    return h


def destroy(h):
    lib().sim_melc_destroy(h)


def table_words(h):
    """The spec's basis, filterbank and row ends as the builder left them, as one uint32 array."""
    n = lib().sim_melc_table_words(h, None)
    out = np.zeros(n, dtype=np.uint32)
    lib().sim_melc_table_words(h, out.ctypes.data)
    return out


def mel_windows(h, audio, valid, n_frames, layout, out, shape=None, tables=False):
    """clx_mel_windows under the simulator, `out` written in place.  tables=True: returns (out, valid_frames, wmax as floats)."""
    B, L = shape if shape is not None else audio.shape
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint32)
    for a in (audio, out):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.itemsize == 4)
    vf, wm = np.zeros(max(B, 1), np.uint32), np.zeros(max(B, 1), np.uint32)
    _check(lib().sim_melc_windows(h, _ptr(audio), B, L, _ptr(valid), n_frames, layout, _ptr(out), vf.ctypes.data, wm.ctypes.data))
    if tables:
        return out, vf[:B], np.array([lib().sim_melc_dec(int(e)) for e in wm[:B]], dtype=np.float32)
    return out


def mel_guarded(h, audio, valid, n_frames, layout, at_end, out):
    """The batch read from where an inaccessible page follows its last float (at_end) or precedes its first."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    valid = np.ascontiguousarray(valid, dtype=np.uint32)
    _check(lib().sim_melc_guarded(h, a.ctypes.data, a.shape[0], a.shape[1], valid.ctypes.data, n_frames, layout, 1 if at_end else 0,
                                  out.ctypes.data))
    return out


def valid_frames(valid, H, n_frames, P):
    """The centred rule: 0 for valid == 0, else min(n_frames, ceil((valid + P) / H))."""
    v = np.asarray(valid, dtype=np.int64)
    return np.where(v == 0, 0, np.minimum((v + P + H - 1) // H, n_frames))


def pad_batch(a, P, mode):
    """The host-padded batch of the definition: P samples on both sides, reflected about the window's ends or zeros."""
    return np.ascontiguousarray(np.pad(a, ((0, 0), (P, P)), mode="reflect" if mode == PAD_REFLECT else "constant"))
