"""Shared pieces of the stream MD5 tests: the FLAC rule on the host (hashlib) and source buffers in every sample format."""
import hashlib

import numpy as np

import claxon_amd as cx

FORMATS = (1, 2, 3, 4, cx.SAMPLE_F32)


def width(bps):
    return (int(bps) + 7) // 8


def ref_md5(vals, bps):
    """FLAC's signature of the interleaved samples `vals`: each as its low ceil(bps / 8) bytes, little-endian."""
    v = np.asarray(vals, dtype=np.int64).reshape(-1)
    w = width(bps)
    b = np.stack([(v >> (8 * k)) & 0xff for k in range(w)], axis=1).astype(np.uint8) if v.size else np.zeros(0, np.uint8)
    return hashlib.md5(b.tobytes()).digest()


def random_samples(rng, n, bps):
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1))
    return rng.integers(lo, hi, size=n, dtype=np.int64)


def encode(vals, fmt, bps):
    """The samples as a source buffer of `fmt` (uint8): little-endian PCM of fmt bytes, or the floats of CLX_OUT_F32."""
    v = np.asarray(vals, dtype=np.int64).reshape(-1)
    if fmt == cx.SAMPLE_F32:
        return (v.astype(np.float64) * 2.0 ** -(bps - 1)).astype(np.float32).view(np.uint8)
    return np.stack([(v >> (8 * k)) & 0xff for k in range(fmt)], axis=1).astype(np.uint8).reshape(-1)


def sample_size(fmt):
    return 4 if fmt == cx.SAMPLE_F32 else fmt


def valid_bps(fmt):
    top = 24 if fmt == cx.SAMPLE_F32 else 8 * fmt
    return [b for b in (1, 5, 8, 9, 12, 16, 17, 20, 24, 25, 31, 32) if b <= top]


def streaminfo(bs, ch, bps, samples, md5):
    """fLaC + a STREAMINFO block (the last metadata block) of min = max block size `bs`, 44.1 kHz, `samples` per channel, `md5`."""
    si = bytearray(34)
    si[0:2] = bs.to_bytes(2, "big"); si[2:4] = bs.to_bytes(2, "big")
    si[10:14] = ((44100 << 12) | ((ch - 1) << 9) | ((bps - 1) << 4) | (samples >> 32)).to_bytes(4, "big")
    si[14:18] = (samples & 0xffffffff).to_bytes(4, "big")
    si[18:34] = md5
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + bytes(si)


def stream(w, bs, ch, bps, vals, frames=None):
    """fLaC + STREAMINFO (sample count and MD5 of the source PCM `vals`) + the workload's frames (or the frame order `frames`)."""
    order = range(w.n) if frames is None else frames
    body = b"".join(w.arena[int(w.offs[i]):int(w.offs[i] + w.lens[i])].tobytes() for i in order)
    return streaminfo(bs, ch, bps, vals.size // ch, ref_md5(vals, bps)) + body
