"""claxon_amd -- MI355X (gfx950) batched FLAC frame decoder behind Claxon's FrameReader/Block API.

This package is a thin ctypes binding of the C ABI in ``include/claxon_hip.h``
(implemented by ``claxon_amd/csrc`` as ``libclaxon_hip.so``: hand-written HIP
kernels + a C++ host layer).  It exists so that tests and ``bench.py`` can drive
the library; the product is the shared library.

There is no CPU decode path: creating a :class:`Context` raises when the
library or a gfx950 device is missing.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
# CLAXON_HIP_LIB selects another build of the same library (e.g. one compiled with -DCLX_TIMELINE for tools/timeline.py)
LIB_PATH = os.environ.get("CLAXON_HIP_LIB") or os.path.join(_HERE, "libclaxon_hip.so")

OK, IO_ERROR, FORMAT_ERROR, UNSUPPORTED, END_OF_STREAM, API_ERROR = range(6)
CH_INDEPENDENT, CH_LEFT_SIDE, CH_RIGHT_SIDE, CH_MID_SIDE = range(4)
ARENA_ON_DEVICE, OUT_ON_DEVICE, VERIFY_CRC16, PATH_WAVES, PATH_LANES, PCM_ON_DEVICE, LANES_FUSED, LANES_SPLIT = 1, 2, 4, 8, 16, 32, 64, 128
K2_LATENCY, K2_THROUGHPUT = 256, 512
LANES_GENERAL = 1024        # the fused lane build without clx_k_lean (the 16-bit tier): every group through the general kernels
COMPOSE, NO_COMPOSE = 2048, 4096   # waves composed by content (clx_k_compose) forced on / off (default: by the descriptors)
OUT_PCM16 = 8192            # planned batches: the output buffers hold interleaved little-endian 16-bit PCM, written by the decode itself
POOL = 16384                # pipelined submissions: the scan and the 16-bit tier as clx_k_pool's tickets (round 6's other launch form; off by default)
OUT_PCM24 = 32768           # the same with packed 24-bit samples (3 bytes each), written by the general lane kernels
OUT_F32 = 65536             # the same with channel-interleaved float32 normalized to [-1, 1): (float)v * 2^-(bps-1), 4 bytes per sample
SAMPLE_F32 = 0x104          # sample format of interleave / decode_frames_stream: the floats of OUT_F32 (next to sample_bytes 1..4)
WINDOW_TC, WINDOW_CT = 0, 1   # clx_gather_windows layouts: [B, L, C] and [B, C, L]
MEL_POWER, MEL_LN, MEL_LOG10 = 0, 1, 2   # clx_mel_create modes
MEL_PAD_REFLECT, MEL_PAD_ZERO = 0, 1     # clx_mel_opts.pad
SUBMIT_DEPTH = 24           # CLX_SUBMIT_DEPTH: the most submissions a Batch keeps in flight (Batch.submit_depth: this batch's)


class ClaxonError(RuntimeError):
    """Mirrors claxon::Error (error.rs:18-32): .status is the variant, .message the reference's string."""

    def __init__(self, status, msg=0, text=None):
        self.status, self.msg = status, msg
        self.message = text if text is not None else (message(msg) if _lib is not None else "")
        super().__init__("status %d: %s" % (status, self.message))


class FrameDesc(C.Structure):
    _fields_ = [("byte_off", C.c_uint64), ("max_bytes", C.c_uint32), ("header_bytes", C.c_uint16),
                ("block_size", C.c_uint16), ("n_channels", C.c_uint8), ("channel_assignment", C.c_uint8),
                ("bps", C.c_uint8), ("reserved", C.c_uint8 * 5)]


class FrameResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("msg", C.c_uint32), ("end_bit", C.c_uint64)]


class FrameHeader(C.Structure):
    _fields_ = [("time", C.c_uint64), ("sample_rate", C.c_uint32), ("frame_or_sample_lo", C.c_uint32),
                ("block_size", C.c_uint16), ("header_bytes", C.c_uint16), ("n_channels", C.c_uint8),
                ("channel_assignment", C.c_uint8), ("bps", C.c_uint8), ("variable_blocking", C.c_uint8)]


class StreamInfo(C.Structure):
    _fields_ = [("min_block_size", C.c_uint16), ("max_block_size", C.c_uint16),
                ("min_frame_size", C.c_uint32), ("max_frame_size", C.c_uint32),
                ("sample_rate", C.c_uint32), ("channels", C.c_uint32), ("bits_per_sample", C.c_uint32),
                ("samples", C.c_uint64), ("md5sum", C.c_uint8 * 16)]


class MetadataBlock(C.Structure):
    """clx_metadata_block (metadata::MetadataBlock, metadata.rs:104-131)"""
    _fields_ = [("kind", C.c_uint32), ("length", C.c_uint32), ("streaminfo", StreamInfo), ("application_id", C.c_uint32),
                ("application_data", C.c_void_p), ("application_len", C.c_size_t), ("tags", C.c_void_p)]


BLOCK_STREAMINFO, BLOCK_PADDING, BLOCK_APPLICATION, BLOCK_VORBIS_COMMENT, BLOCK_RESERVED = 0, 1, 2, 4, 126


class BlockInfo(C.Structure):
    _fields_ = [("time", C.c_uint64), ("block_size", C.c_uint32), ("channels", C.c_uint32)]


FRAME_DESC_DTYPE = np.dtype([("byte_off", "<u8"), ("max_bytes", "<u4"), ("header_bytes", "<u2"),
                             ("block_size", "<u2"), ("n_channels", "u1"), ("channel_assignment", "u1"),
                             ("bps", "u1"), ("reserved", "u1", (5,))])
FRAME_RESULT_DTYPE = np.dtype([("status", "<i4"), ("msg", "<u4"), ("end_bit", "<u8")])
FRAME_HEADER_DTYPE = np.dtype([("time", "<u8"), ("sample_rate", "<u4"), ("frame_or_sample_lo", "<u4"),
                               ("block_size", "<u2"), ("header_bytes", "<u2"), ("n_channels", "u1"),
                               ("channel_assignment", "u1"), ("bps", "u1"), ("variable_blocking", "u1")])
ADDN_TERM_DTYPE = np.dtype([("batch", "<i4"), ("index", "<i4"), ("offset", "<u4"), ("loop", "<u4"), ("snr_db", "<f4")])   # clx_addn_term
ADDN_MAX_TERMS, ADDN_MAX_BATCHES = 16, 8
assert FRAME_DESC_DTYPE.itemsize == C.sizeof(FrameDesc) == 24
assert FRAME_RESULT_DTYPE.itemsize == C.sizeof(FrameResult) == 16
assert FRAME_HEADER_DTYPE.itemsize == C.sizeof(FrameHeader) == 24

EXPORTS = [
    "clx_message", "clx_message_status", "clx_version", "clx_parse_frame_header", "clx_crc8", "clx_crc16",
    "clx_create", "clx_destroy", "clx_last_error", "clx_decode_frames", "clx_decode_frames_multi", "clx_decode_frames_stream", "clx_set_stream_chunk", "clx_host_alloc", "clx_host_free", "clx_decode_subframes", "clx_interleave",
    "clx_batch_create", "clx_batch_run", "clx_batch_submit", "clx_batch_submit_depth", "clx_batch_submit_lanes", "clx_batch_submit_merge", "clx_batch_flush", "clx_batch_interleave", "clx_batch_results", "clx_batch_slots", "clx_batch_set_profiling",
    "clx_batch_kernel_ms", "clx_batch_kernel_name", "clx_batch_destroy", "clx_read_stream_header", "clx_read_stream_header_ext",
    "clx_tags_vendor", "clx_tags_count", "clx_tags_get", "clx_tags_lookup", "clx_tags_free", "clx_reader_tags", "clx_reader_open", "clx_reader_new",
    "clx_reader_streaminfo", "clx_reader_next_block", "clx_reader_close", "clx_index_frames", "clx_index_frames_device",
    "clx_read_metadata_block", "clx_read_metadata_block_with_header", "clx_describe_packets", "clx_md5_streams", "clx_index_streams_device", "clx_gather_windows",
    "clx_resample_windows", "clx_mix_windows", "clx_mel_create", "clx_mel_create_ex", "clx_mel_create_framed", "clx_mel_create_cepstral", "clx_mel_create_reflected", "clx_mel_destroy", "clx_mel_windows",
    "clx_norm_windows", "clx_add_windows", "clx_addn_windows", "clx_reverb_windows", "clx_reverb_windows_fft", "clx_specaug_windows",
    "clx_splice_windows", "clx_splice_deltas", "clx_cmvn_global_windows", "clx_cmvn_sliding_windows", "clx_cmvn_from_stats",
    "clx_vad_windows", "clx_select_windows", "clx_cmvn_stats_windows", "clx_cmvn_grouped_windows",
]


def build(force=False, verbose=False):
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in ("clx_api.hip", "clx_kernels.hip", "clx_lanes.hip", "clx_lean.hip", "clx_md5.hip", "clx_index.hip", "clx_window.hip", "clx_resample.hip", "clx_mix.hip", "clx_mel.hip", "clx_norm.hip", "clx_add.hip", "clx_addn.hip", "clx_reverb.hip", "clx_reverb_fft.hip", "clx_specaug.hip", "clx_splice.hip", "clx_cmvn.hip", "clx_cmvn_stats.hip", "clx_vad.hip", "clx_device.h", "clx_crct.h", "clx_plan.h",
                                            os.path.join("intrin", "clx_intrin.h"), os.path.join("intrin", "clx_k2_dot2.h"), os.path.join("host", "claxon.hpp"))]
    srcs.append(os.path.join(_HERE, "..", "include", "claxon_hip.h"))
    if (not force and os.path.exists(LIB_PATH)
            and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(s) for s in srcs)):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(_CSRC, "intrin"),
           os.path.join(_CSRC, "clx_api.hip"), "-o", LIB_PATH] + os.environ.get("CLX_EXTRA_FLAGS", "").split()
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=_CSRC)
    return LIB_PATH


_lib = None


def lib():
    """Load libclaxon_hip.so (raises if it has not been built -- there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ClaxonError(API_ERROR, 0, "libclaxon_hip.so is not built (run `python -c 'import __graft_entry__ as g; "
                                        "g.build()'`); claxon_amd has no CPU fallback")
    # When PyTorch shares the process (it is the allocator / stream owner for tests and bench.py) its wheel
    # brings its own copy of the HIP runtime under the unversioned name libamdhip64.so.  Importing torch FIRST
    # makes our NEEDED libamdhip64.so.7 resolve to that already-loaded copy (same SONAME); the other order
    # would put two HIP/HSA runtimes in one process and the second one finds no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
    L.clx_message.restype = C.c_char_p
    L.clx_message.argtypes = [C.c_uint32]
    L.clx_message_status.argtypes = [C.c_uint32]
    L.clx_version.restype = C.c_uint32
    L.clx_parse_frame_header.argtypes = [vp, sz, C.c_int, C.POINTER(FrameHeader), u32p]
    L.clx_crc8.restype = C.c_uint8
    L.clx_crc8.argtypes = [vp, sz]
    L.clx_crc16.restype = C.c_uint16
    L.clx_crc16.argtypes = [vp, sz]
    L.clx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.clx_destroy.argtypes = [vp]
    L.clx_destroy.restype = None
    L.clx_last_error.restype = C.c_char_p
    L.clx_last_error.argtypes = [vp]
    L.clx_decode_frames.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, C.c_uint32]
    L.clx_decode_subframes.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, C.c_uint32]
    L.clx_batch_create.argtypes = [vp, vp, sz, vp, C.c_uint32, C.POINTER(vp)]
    L.clx_decode_frames_multi.argtypes = [vp, sz, vp, sz, vp, sz, vp, vp, vp, C.c_uint32]
    L.clx_decode_frames_stream.argtypes = [vp, vp, sz, vp, sz, vp, C.c_uint32, vp, vp, C.c_uint32]
    L.clx_host_alloc.restype = vp
    L.clx_host_alloc.argtypes = [sz]
    L.clx_host_free.argtypes = [vp]
    L.clx_set_stream_chunk.argtypes = [vp, sz]
    L.clx_set_stream_chunk.restype = None
    L.clx_batch_run.argtypes = [vp, vp, sz, vp, vp]
    L.clx_batch_submit.argtypes = [vp, vp, sz, vp, vp]
    L.clx_batch_flush.argtypes = [vp, vp]
    L.clx_batch_submit_depth.argtypes = [vp]
    L.clx_batch_submit_lanes.argtypes = [vp]
    L.clx_batch_submit_merge.argtypes = [vp]
    L.clx_batch_submit_merge.restype = C.c_int
    L.clx_batch_results.argtypes = [vp, vp]
    L.clx_batch_interleave.argtypes = [vp, vp, vp, C.c_uint32, vp]
    L.clx_index_frames_device.argtypes = [vp, vp, sz, sz, vp, vp, sz, C.POINTER(sz), C.POINTER(sz), C.c_uint32]
    L.clx_index_streams_device.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, vp, sz, vp, vp, C.POINTER(sz), C.c_uint32]
    L.clx_interleave.argtypes = [vp, vp, vp, sz, vp, vp, vp, C.c_uint32, C.c_uint32]
    L.clx_md5_streams.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, sz, vp, vp]
    L.clx_gather_windows.argtypes = [vp, vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    L.clx_resample_windows.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    L.clx_mix_windows.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    L.clx_mel_create.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(vp)]
    L.clx_mel_create_ex.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_float, vp, C.POINTER(vp)]
    L.clx_mel_create_framed.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp,
                                        C.POINTER(vp)]
    L.clx_mel_create_cepstral.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp,
                                          vp, C.POINTER(vp)]
    L.clx_mel_create_reflected.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp,
                                           vp, C.POINTER(vp)]
    L.clx_mel_destroy.argtypes = [vp, vp]
    L.clx_mel_destroy.restype = None
    L.clx_mel_windows.argtypes = [vp, vp, vp, sz, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp]
    L.clx_norm_windows.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp]
    L.clx_add_windows.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, vp, sz, vp, vp, vp, C.c_uint32, vp, vp, vp]
    L.clx_addn_windows.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp]
    L.clx_reverb_windows.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, vp, sz, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, vp]
    L.clx_reverb_windows_fft.argtypes = L.clx_reverb_windows.argtypes
    L.clx_specaug_windows.argtypes = [vp, vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.clx_splice_windows.argtypes = [vp, vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp]
    L.clx_splice_deltas.argtypes = [C.c_uint32, C.c_uint32, vp, vp, u32p]
    L.clx_cmvn_global_windows.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp]
    L.clx_cmvn_sliding_windows.argtypes = [vp, vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp]
    L.clx_cmvn_from_stats.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp]
    L.clx_cmvn_stats_windows.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp]
    L.clx_cmvn_grouped_windows.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp]
    L.clx_vad_windows.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp]
    L.clx_select_windows.argtypes = [vp, vp, vp, sz, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, vp]
    L.clx_batch_slots.restype = C.c_uint64
    L.clx_batch_slots.argtypes = [vp]
    L.clx_batch_set_profiling.argtypes = [vp, C.c_int]
    L.clx_batch_kernel_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.clx_batch_kernel_name.restype = C.c_char_p
    L.clx_batch_kernel_name.argtypes = [vp, C.c_int]
    L.clx_batch_destroy.argtypes = [vp]
    L.clx_batch_destroy.restype = None
    L.clx_read_stream_header.argtypes = [vp, sz, C.POINTER(StreamInfo), C.POINTER(sz), u32p]
    L.clx_read_stream_header_ext.argtypes = [vp, sz, C.c_uint32, C.POINTER(StreamInfo), C.POINTER(sz), C.POINTER(vp), u32p]
    L.clx_tags_vendor.restype = vp
    L.clx_tags_vendor.argtypes = [vp, C.POINTER(sz)]
    L.clx_tags_count.restype = sz
    L.clx_tags_count.argtypes = [vp]
    L.clx_tags_get.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]
    L.clx_tags_lookup.restype = vp
    L.clx_tags_lookup.argtypes = [vp, C.c_char_p, sz, C.POINTER(sz)]
    L.clx_tags_free.argtypes = [vp]
    L.clx_tags_free.restype = None
    L.clx_reader_tags.restype = vp
    L.clx_reader_tags.argtypes = [vp]
    L.clx_reader_open.argtypes = [vp, C.c_char_p, C.POINTER(vp), u32p]
    L.clx_reader_new.argtypes = [vp, vp, sz, C.POINTER(vp), u32p]
    L.clx_reader_streaminfo.argtypes = [vp, C.POINTER(StreamInfo)]
    L.clx_reader_next_block.argtypes = [vp, vp, sz, C.POINTER(BlockInfo), u32p]
    L.clx_reader_close.argtypes = [vp]
    L.clx_reader_close.restype = None
    L.clx_index_frames.argtypes = [vp, sz, sz, vp, vp, sz, C.POINTER(sz), C.POINTER(sz)]
    L.clx_read_metadata_block.argtypes = [vp, sz, C.c_uint8, C.c_uint32, C.POINTER(MetadataBlock), C.POINTER(sz), u32p]
    L.clx_read_metadata_block_with_header.argtypes = [vp, sz, C.POINTER(MetadataBlock), C.POINTER(C.c_int), C.POINTER(sz), u32p]
    L.clx_describe_packets.argtypes = [vp, sz, vp, vp, sz, C.c_int, vp, vp, vp]
    _lib = L
    return L


def message(msg):
    return lib().clx_message(int(msg)).decode()


def _sample_size(sample_bytes):
    """Bytes per sample of a narrow stage's sample format (1..4, SAMPLE_F32); 0: none."""
    return 4 if sample_bytes == SAMPLE_F32 else sample_bytes if 1 <= sample_bytes <= 4 else 0


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


# ----------------------------------------------------------------------------- host-side helpers

def crc8(data):
    a = _u8(data)
    return int(lib().clx_crc8(_np_ptr(a), a.size))


def crc16(data):
    a = _u8(data)
    return int(lib().clx_crc16(_np_ptr(a), a.size))


def parse_frame_header(data, check_crc=True):
    """read_frame_header_or_eof (frame.rs:131-316).  Returns (status, msg, FrameHeader)."""
    a = _u8(data)
    h = FrameHeader()
    m = C.c_uint32(0)
    st = lib().clx_parse_frame_header(_np_ptr(a), a.size, 1 if check_crc else 0, C.byref(h), C.byref(m))
    return st, int(m.value), h


def read_stream_header(data):
    a = _u8(data)
    si = StreamInfo()
    off = C.c_size_t(0)
    m = C.c_uint32(0)
    st = lib().clx_read_stream_header(_np_ptr(a), a.size, C.byref(si), C.byref(off), C.byref(m))
    return st, int(m.value), si, int(off.value)


def _tags_to_py(t):
    """(vendor bytes | None, [(name bytes, value bytes)]) from a clx_tags handle (not freed here)."""
    if not t:
        return None, []
    n = C.c_size_t(0)
    v = lib().clx_tags_vendor(t, C.byref(n))
    vendor = C.string_at(v, n.value)
    out = []
    for i in range(lib().clx_tags_count(t)):
        pn, pv, ln, lv = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
        assert lib().clx_tags_get(t, i, C.byref(pn), C.byref(ln), C.byref(pv), C.byref(lv)) == OK
        out.append((C.string_at(pn, ln.value), C.string_at(pv, lv.value)))
    return vendor, out


def _tags_lookup(t, name):
    """metadata::GetTag (metadata.rs:197-211): every value whose name matches ASCII-case-insensitively, in order."""
    out, k = [], 0
    while True:
        n = C.c_size_t(0)
        v = lib().clx_tags_lookup(t, name.encode() if isinstance(name, str) else name, k, C.byref(n))
        if not v:
            return out
        out.append(C.string_at(v, n.value))
        k += 1


def read_stream_header_ext(data, metadata_only=False, read_vorbis_comment=True):
    """FlacReader::new_ext (lib.rs:230-307) on bytes: (status, msg, StreamInfo, audio offset, vendor | None, [(name, value)])."""
    a = _u8(data)
    si = StreamInfo()
    off = C.c_size_t(0)
    m = C.c_uint32(0)
    t = C.c_void_p()
    opts = (1 if metadata_only else 0) | (0 if read_vorbis_comment else 2)
    st = lib().clx_read_stream_header_ext(_np_ptr(a), a.size, opts, C.byref(si), C.byref(off), C.byref(t), C.byref(m))
    vendor, tags = _tags_to_py(t.value)
    if t.value:
        lib().clx_tags_free(t)
    return st, int(m.value), si, int(off.value), vendor, tags


def read_metadata_block(data, block_type=None, length=None):
    """metadata::read_metadata_block (metadata.rs:261) when block_type / length are given, else
    read_metadata_block_with_header (metadata.rs:244).  Same dict as oracle.read_metadata_block."""
    a = _u8(data)
    blk = MetadataBlock()
    used, m = C.c_size_t(0), C.c_uint32(0)
    out = {}
    if block_type is None:
        last = C.c_int(0)
        st = lib().clx_read_metadata_block_with_header(_np_ptr(a), a.size, C.byref(blk), C.byref(last), C.byref(used), C.byref(m))
        out["is_last"] = bool(last.value)
    else:
        st = lib().clx_read_metadata_block(_np_ptr(a), a.size, int(block_type), int(length), C.byref(blk), C.byref(used), C.byref(m))
    out.update(status=st, msg=int(m.value))
    if st != OK:
        return out
    out.update(kind=int(blk.kind), length=int(blk.length), consumed=int(used.value))
    if blk.kind == BLOCK_STREAMINFO:
        out["streaminfo"] = blk.streaminfo
    elif blk.kind == BLOCK_APPLICATION:
        out["app_id"] = int(blk.application_id)
        out["app_data"] = C.string_at(blk.application_data, blk.application_len) if blk.application_len else b""
    elif blk.kind == BLOCK_VORBIS_COMMENT:
        out["vendor"], out["tags"] = _tags_to_py(blk.tags)
        lib().clx_tags_free(blk.tags)
    return out


def describe_packets(arena, offs, lens, check_crc=True):
    """Container packets -> frame descriptors (clx_describe_packets): returns (descs, headers, results)."""
    a = _u8(arena)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n = offs.size
    descs = np.zeros(n, dtype=FRAME_DESC_DTYPE)
    hdrs = np.zeros(n, dtype=FRAME_HEADER_DTYPE)
    res = np.zeros(n, dtype=FRAME_RESULT_DTYPE)
    st = lib().clx_describe_packets(_np_ptr(a), a.size, _np_ptr(offs), _np_ptr(lens), n, 1 if check_crc else 0,
                                    _np_ptr(descs), _np_ptr(hdrs), _np_ptr(res))
    if st == API_ERROR:
        raise ClaxonError(API_ERROR, 0, "clx_describe_packets: a packet lies outside the arena")
    return descs, hdrs, res


def index_frames(data, start=0, cap=1 << 20):
    """Host frame indexer.  Returns (descs[np FRAME_DESC_DTYPE], headers[np FRAME_HEADER_DTYPE], stop_offset)."""
    a = _u8(data)
    cap = max(1, min(cap, a.size // 8 + 2))
    descs = np.zeros(cap, dtype=FRAME_DESC_DTYPE)
    hdrs = np.zeros(cap, dtype=FRAME_HEADER_DTYPE)
    n = C.c_size_t(0)
    stop = C.c_size_t(0)
    st = lib().clx_index_frames(_np_ptr(a), a.size, start, _np_ptr(descs), _np_ptr(hdrs), cap, C.byref(n), C.byref(stop))
    if st != OK:
        raise ClaxonError(st)
    return descs[:n.value].copy(), hdrs[:n.value].copy(), int(stop.value)


def descs_from_offsets(arena, offs, max_bytes=None, check_crc=True):
    """Build frame descriptors for frames whose start offsets are known (containers, the synthetic
    generator): parses each frame header on the host.  Raises on a malformed header."""
    a = _u8(arena)
    offs = np.asarray(offs, dtype=np.uint64)
    descs = np.zeros(offs.size, dtype=FRAME_DESC_DTYPE)
    hdrs = np.zeros(offs.size, dtype=FRAME_HEADER_DTYPE)
    L = lib()
    h = FrameHeader()
    m = C.c_uint32(0)
    base = a.ctypes.data
    for i, off in enumerate(offs.tolist()):
        avail = a.size - off if max_bytes is None else min(int(max_bytes[i]), a.size - off)
        st = L.clx_parse_frame_header(C.c_void_p(base + off), avail, 1 if check_crc else 0, C.byref(h), C.byref(m))
        if st != OK:
            raise ClaxonError(st, int(m.value))
        descs[i] = (off, avail, h.header_bytes, h.block_size, h.n_channels, h.channel_assignment, h.bps, (0,) * 5)
        hdrs[i] = (h.time, h.sample_rate, h.frame_or_sample_lo, h.block_size, h.header_bytes, h.n_channels,
                   h.channel_assignment, h.bps, h.variable_blocking)
    return descs, hdrs


def descs_for_subframes(offs, block_sizes, bps):
    n = len(offs)
    d = np.zeros(n, dtype=FRAME_DESC_DTYPE)
    d["byte_off"] = offs
    d["max_bytes"] = 0xffffffff
    d["block_size"] = block_sizes
    d["n_channels"] = 1
    d["bps"] = bps
    d["reserved"][:, 0] = 1
    return d


# ----------------------------------------------------------------------------- device objects

class PinnedArray:
    """A numpy view of pinned host memory from clx_host_alloc (freed with the object): buffers handed to
    Context.decode_frames_stream in this kind of memory are copied asynchronously at link speed."""

    def __init__(self, shape, dtype=np.uint8):
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        self._p = lib().clx_host_alloc(max(n, 1))
        if not self._p:
            raise MemoryError("clx_host_alloc(%d) failed" % n)
        buf = (C.c_uint8 * max(n, 1)).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if self._p:
            self.array = None
            lib().clx_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_frames_multi(ctxs, arena, descs, out_offs, out=None, verify_crc=False, path=0):
    """clx_decode_frames_multi: one batch, several contexts (one per GPU, or several on one), no exchange between them."""
    a = _u8(arena)
    descs = np.ascontiguousarray(descs, dtype=FRAME_DESC_DTYPE)
    out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
    n = descs.size
    total = int((out_offs + descs["n_channels"].astype(np.uint64) * descs["block_size"].astype(np.uint64)).max()) if n else 0
    if out is None:
        out = np.zeros(total, dtype=np.int32)
    res = np.zeros(n, dtype=FRAME_RESULT_DTYPE)
    hs = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    st = lib().clx_decode_frames_multi(hs, len(ctxs), _np_ptr(a), a.size, _np_ptr(descs), n, _np_ptr(out), _np_ptr(out_offs),
                                       _np_ptr(res), (VERIFY_CRC16 if verify_crc else 0) | path)
    ctxs[0]._check(st)
    return out, res


def _wait_for_gpu_node(deadline):
    """Poll (in child processes) until the kernel driver exposes a gfx950 agent or the deadline passes."""
    import time
    probe = "/opt/rocm/bin/rocminfo"
    while time.time() < deadline:
        if os.path.exists("/dev/kfd"):
            if not os.path.exists(probe):
                return
            try:
                r = subprocess.run([probe], capture_output=True, timeout=30)
                if r.returncode == 0 and b"gfx950" in r.stdout:
                    return
            except Exception:
                pass
        time.sleep(1.0)


class Context:
    """clx_ctx: one per GPU / stream; not thread safe."""

    def __init__(self, device=0, wait_s=0.0):
        """`wait_s`: keep retrying for this long while the device is not (yet) visible -- a freshly
        booted GPU box can take a few seconds to expose /dev/kfd.  It never falls back to the CPU."""
        import time
        self._h = C.c_void_p(None)
        deadline = time.time() + wait_s
        if wait_s > 0:
            _wait_for_gpu_node(deadline)       # probe from a child process: never poison this one's HIP runtime
        while True:
            st = lib().clx_create(int(device), C.byref(self._h))
            if (st == OK and self._h) or time.time() >= deadline:
                break
            time.sleep(1.0)
        if st != OK or not self._h:
            self._h = None
            raise ClaxonError(API_ERROR, 0, "clx_create(%d) failed: no usable gfx950 HIP device; claxon_amd has no "
                                            "CPU fallback" % device)
        self.device = device

    def close(self):
        if self._h:
            lib().clx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return lib().clx_last_error(self._h).decode()

    def _check(self, st):
        if st != OK:
            raise ClaxonError(st, 0, self.last_error())

    def index_frames(self, data, start=0, cap=1 << 20):
        """Device frame indexer: same contract as claxon_amd.index_frames (host), byte work on the GPU."""
        a = _u8(data)
        cap = max(1, min(cap, a.size // 8 + 2))
        descs = np.zeros(cap, dtype=FRAME_DESC_DTYPE)
        hdrs = np.zeros(cap, dtype=FRAME_HEADER_DTYPE)
        n = C.c_size_t(0)
        stop = C.c_size_t(0)
        st = lib().clx_index_frames_device(self._h, _np_ptr(a), a.size, start, _np_ptr(descs), _np_ptr(hdrs), cap,
                                           C.byref(n), C.byref(stop), 0)
        self._check(st)
        return descs[:n.value].copy(), hdrs[:n.value].copy(), int(stop.value)

    def index_streams(self, arena, offs, lens, starts=None, cap=None):
        """The device indexer for a whole shard (clx_index_streams_device): the streams arena[offs[k] : offs[k] + lens[k]] (offs multiples
        of 16, ascending), each indexed from offs[k] + starts[k] on, in one pass.  `arena` is bytes-like / numpy (a host arena, uploaded
        once) or a CUDA uint8 tensor (16-byte aligned, padded like a decode arena; the work pending on the current torch stream is
        waited for first).  Returns (descs, headers, first_frame, stop_offs): stream k's frames are descs[first_frame[k]:first_frame[k + 1]],
        exactly the host indexer's answer for that stream alone with byte_off and stop_offs[k] rebased onto the arena."""
        offs = np.ascontiguousarray(offs, dtype=np.uint64).reshape(-1)
        lens = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
        if starts is not None:
            starts = np.ascontiguousarray(starts, dtype=np.uint64).reshape(-1)
        if offs.size != lens.size or (starts is not None and starts.size != offs.size):
            raise ValueError("index_streams: offs, lens and starts differ in length")
        flags = 0
        if hasattr(arena, "data_ptr"):
            import torch
            if not arena.is_cuda:
                raise ValueError("index_streams: a tensor arena must be on the GPU")
            torch.cuda.current_stream(arena.device).synchronize()
            ptr, size, flags = arena.data_ptr(), arena.numel() * arena.element_size(), ARENA_ON_DEVICE
        else:
            a = _u8(arena)
            ptr, size = _np_ptr(a), a.size
        n = offs.size
        first = np.zeros(n + 1, dtype=np.uint64)
        stops = np.zeros(n, dtype=np.uint64)
        found = C.c_size_t(0)
        cap = int(cap) if cap is not None else int(lens.sum()) // 512 + 4 * n + 64
        while True:
            descs = np.zeros(max(cap, 1), dtype=FRAME_DESC_DTYPE)
            hdrs = np.zeros(max(cap, 1), dtype=FRAME_HEADER_DTYPE)
            st = lib().clx_index_streams_device(self._h, ptr, size, _np_ptr(offs), _np_ptr(lens), _np_ptr(starts), n, _np_ptr(descs),
                                                _np_ptr(hdrs), cap, _np_ptr(first), _np_ptr(stops), C.byref(found), flags)
            if st == API_ERROR and found.value > cap:           # told how many frames there are: once more with room for them
                cap = int(found.value)
                continue
            self._check(st)
            return descs[:found.value].copy(), hdrs[:found.value].copy(), first, stops

    def decode_frames(self, arena, descs, out_offs, out=None, verify_crc=False, path=0):
        """One-shot host->device->host decode.  Returns (out int32, results np FRAME_RESULT_DTYPE)."""
        a = _u8(arena)
        descs = np.ascontiguousarray(descs, dtype=FRAME_DESC_DTYPE)
        out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
        n = descs.size
        total = int((out_offs + descs["n_channels"].astype(np.uint64) * descs["block_size"].astype(np.uint64)).max()) if n else 0
        if out is None:
            out = np.zeros(total, dtype=np.int32)
        assert out.dtype == np.int32 and out.size >= total
        res = np.zeros(n, dtype=FRAME_RESULT_DTYPE)
        st = lib().clx_decode_frames(self._h, _np_ptr(a), a.size, _np_ptr(descs), n, _np_ptr(out), _np_ptr(out_offs),
                                     _np_ptr(res), (VERIFY_CRC16 if verify_crc else 0) | path)
        self._check(st)
        return out, res

    def set_stream_chunk(self, frames_per_chunk):
        """Frames per chunk of decode_frames_stream (0: the library's rule: a third of the batch, 256 .. 8192)."""
        lib().clx_set_stream_chunk(self._h, int(frames_per_chunk))

    def decode_frames_stream(self, arena, descs, out_offs, out=None, sample_bytes=0, verify_crc=False, path=0, copy_back=True):
        """clx_decode_frames_stream: host-to-host decode, chunks pipelined (upload | decode | download).  sample_bytes 0: planar
        int32 (returned as int32 array); 1..4: channel-interleaved little-endian PCM (returned as uint8 array); SAMPLE_F32:
        channel-interleaved normalized floats (returned as float32 array);
        copy_back=False: only the results come back.  Returns (out or None, results)."""
        a = _u8(arena)
        descs = np.ascontiguousarray(descs, dtype=FRAME_DESC_DTYPE)
        out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
        n = descs.size
        total = int((out_offs + descs["n_channels"].astype(np.uint64) * descs["block_size"].astype(np.uint64)).max()) if n else 0
        if copy_back and out is None:
            out = (np.zeros(total, dtype=np.int32) if sample_bytes == 0 else np.zeros(total, dtype=np.float32) if sample_bytes == SAMPLE_F32
                   else np.zeros(total * sample_bytes, dtype=np.uint8))
        if copy_back:
            assert out.nbytes >= total * (_sample_size(sample_bytes) or 4)
        res = np.zeros(n, dtype=FRAME_RESULT_DTYPE)
        st = lib().clx_decode_frames_stream(self._h, _np_ptr(a), a.size, _np_ptr(descs), n, _np_ptr(out) if copy_back else None, sample_bytes,
                                            _np_ptr(out_offs), _np_ptr(res), (VERIFY_CRC16 if verify_crc else 0) | path)
        self._check(st)
        return (out if copy_back else None), res

    def interleave(self, planar, descs, out_offs, sample_bytes, results=None, pcm=None):
        """One-shot interleave / narrow stage on host arrays: planar i32 -> channel-interleaved little-endian PCM of
        `sample_bytes` bytes per sample (uint8 array, frame i at byte out_offs[i] * sample_bytes), or with SAMPLE_F32 the
        normalized floats of OUT_F32 (float32 array, frame i at index out_offs[i]).  Frames whose `results` status is not OK
        keep whatever `pcm` held."""
        planar = np.ascontiguousarray(planar, dtype=np.int32)
        descs = np.ascontiguousarray(descs, dtype=FRAME_DESC_DTYPE)
        out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
        n = descs.size
        total = int((out_offs + descs["n_channels"].astype(np.uint64) * descs["block_size"].astype(np.uint64)).max()) if n else 0
        assert planar.size >= total
        if pcm is None:
            pcm = np.zeros(total, dtype=np.float32) if sample_bytes == SAMPLE_F32 else np.zeros(total * sample_bytes, dtype=np.uint8)
        if sample_bytes == SAMPLE_F32:
            assert pcm.dtype == np.float32 and pcm.size >= total
        else:
            assert pcm.dtype == np.uint8 and pcm.size >= total * sample_bytes
        if results is not None:
            results = np.ascontiguousarray(results, dtype=FRAME_RESULT_DTYPE)
        st = lib().clx_interleave(self._h, _np_ptr(planar), _np_ptr(descs), n, _np_ptr(out_offs),
                                  _np_ptr(results) if results is not None else None, _np_ptr(pcm), sample_bytes, 0)
        self._check(st)
        return pcm

    def md5_streams(self, samples, sample_format, first, counts, bps):
        """FLAC audio MD5s (clx_md5_streams) of many streams held on the device, one GPU lane per stream: uint8 [n, 16].  `samples` is a
        CUDA tensor (the work pending on the current torch stream is waited for first) or a device pointer, holding channel-interleaved
        samples in `sample_format` (1..4 bytes of little-endian PCM, or SAMPLE_F32); stream k is counts[k] samples from sample index
        first[k] on, hashed as the low ceil(bps[k] / 8) bytes of each."""
        first = np.ascontiguousarray(first, dtype=np.uint64).reshape(-1)
        counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        bps = np.ascontiguousarray(bps, dtype=np.uint8).reshape(-1)
        if not (first.size == counts.size == bps.size):
            raise ValueError("md5_streams: first, counts and bps differ in length")
        if hasattr(samples, "data_ptr"):
            import torch
            if not samples.is_cuda:
                raise ValueError("md5_streams: samples must be on the GPU")
            torch.cuda.current_stream(samples.device).synchronize()
            ptr = samples.data_ptr()
        else:
            ptr = int(samples) if samples else None
        out = np.zeros((first.size, 16), dtype=np.uint8)
        self._check(lib().clx_md5_streams(self._h, ptr, int(sample_format), _np_ptr(first), _np_ptr(counts), _np_ptr(bps), first.size,
                                          _np_ptr(out), None))
        return out

    def gather_windows(self, src, src_first, valid, window_len, channels, layout, out, stream=None):
        """clx_gather_windows: window k = valid[k] samples per channel from float src_first[k] of `src` on (channel-interleaved float32,
        what OUT_F32 writes), zero-filled to window_len, written to `out` as [B, L, C] (WINDOW_TC) or [B, C, L] (WINDOW_CT).  `src` and
        `out` are CUDA float32 tensors or device pointers.  Asynchronous on `stream` (a torch stream or a raw handle; None: the current
        torch stream when `out` is a tensor, else the context's own): nothing is waited for, before or after."""
        src_first = np.ascontiguousarray(src_first, dtype=np.uint64).reshape(-1)
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        if src_first.size != valid.size:
            raise ValueError("gather_windows: src_first and valid differ in length")
        if stream is None and hasattr(out, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(out.device)
        handle = getattr(stream, "cuda_stream", stream)
        ptr = [t.data_ptr() if hasattr(t, "data_ptr") else (int(t) if t else None) for t in (src, out)]
        self._check(lib().clx_gather_windows(self._h, ptr[0], _np_ptr(src_first), _np_ptr(valid), src_first.size, int(window_len), int(channels),
                                             int(layout), ptr[1], C.c_void_p(handle) if handle else None))
        return out

    def resample_windows(self, src, src_first, src_t0, src_n, out_t0, valid, src_rate, out_rate, window_len, channels, layout, out, stream=None):
        """clx_resample_windows: window k = outputs out_t0[k] .. out_t0[k] + valid[k] - 1 of its stream resampled from src_rate[k] to
        out_rate (the fixed windowed-sinc resampler of claxon_hip.h; a plain copy where the two are equal), zero-filled to window_len,
        written to `out` as [B, L, C] (WINDOW_TC) or [B, C, L] (WINDOW_CT).  The window's source span is src_n[k] samples per channel
        of `src` (channel-interleaved float32) from float src_first[k] on, the first of them stream sample src_t0[k]; samples outside
        it count as zero.  `src`, `out` and `stream` as for gather_windows."""
        arrs = [np.ascontiguousarray(a, dtype=t).reshape(-1) for a, t in ((src_first, np.uint64), (src_t0, np.int64), (src_n, np.uint32),
                                                                           (out_t0, np.uint64), (valid, np.uint32), (src_rate, np.uint32))]
        if len({a.size for a in arrs}) != 1:
            raise ValueError("resample_windows: the per-window arrays differ in length")
        for name, v in (("out_rate", out_rate), ("window_len", window_len), ("channels", channels), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("resample_windows: %s is out of range" % name)
        if stream is None and hasattr(out, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(out.device)
        handle = getattr(stream, "cuda_stream", stream)
        ptr = [t.data_ptr() if hasattr(t, "data_ptr") else (int(t) if t else None) for t in (src, out)]
        self._check(lib().clx_resample_windows(self._h, ptr[0], *[_np_ptr(a) for a in arrs], arrs[0].size, int(out_rate), int(window_len),
                                               int(channels), int(layout), ptr[1], C.c_void_p(handle) if handle else None))
        return out

    def mix_windows(self, src, src_first, src_t0, src_n, out_t0, valid, src_rate, src_channels, out_rate, window_len, out_channels, layout,
                    out, stream=None):
        """clx_mix_windows: resample_windows with window k's source holding src_channels[k] interleaved channels and every window brought
        to out_channels: unchanged where the two are equal, the float32 mean of the channels (claxon_hip.h gives its order) for
        out_channels == 1, a mono source copied to every channel; any other combination is refused.  `out` is [B, L, out_channels]
        (WINDOW_TC) or [B, out_channels, L] (WINDOW_CT).  Everything else as for resample_windows."""
        arrs = [np.ascontiguousarray(a, dtype=t).reshape(-1) for a, t in ((src_first, np.uint64), (src_t0, np.int64), (src_n, np.uint32),
                                                                           (out_t0, np.uint64), (valid, np.uint32), (src_rate, np.uint32),
                                                                           (src_channels, np.uint8))]
        if len({a.size for a in arrs}) != 1:
            raise ValueError("mix_windows: the per-window arrays differ in length")
        for name, v in (("out_rate", out_rate), ("window_len", window_len), ("out_channels", out_channels), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("mix_windows: %s is out of range" % name)
        if stream is None and hasattr(out, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(out.device)
        handle = getattr(stream, "cuda_stream", stream)
        ptr = [t.data_ptr() if hasattr(t, "data_ptr") else (int(t) if t else None) for t in (src, out)]
        self._check(lib().clx_mix_windows(self._h, ptr[0], *[_np_ptr(a) for a in arrs], arrs[0].size, int(out_rate), int(window_len),
                                          int(out_channels), int(layout), ptr[1], C.c_void_p(handle) if handle else None))
        return out

    def mel_windows(self, spec, audio, valid, n_frames, layout, out, stream=None):
        """clx_mel_windows: the features of `spec` (a MelSpec of this context) for the dense mono batch `audio` [B, L] (float32, the
        samples from valid[k] on zero), n_frames frames per window, written to `out` as [B, n_frames, n_out] (WINDOW_TC) or
        [B, n_out, n_frames] (WINDOW_CT), n_out = spec.n_out: n_mels, or n_ceps of a cepstral spec; a frame from spec.valid_frames(valid[k], n_frames) on is zeros (the scaled silence value
        for a spec with top).  A centred spec takes the [B, L] batch as the crops its frames are centred on.  `audio` and `out` are CUDA float32 tensors
        (B and L are the tensor's) or `audio` is a (pointer, B, L) triple and `out` a pointer.  Asynchronous on `stream` as
        gather_windows is."""
        if getattr(spec, "_h", None) is None or spec.ctx is not self:
            raise ValueError("mel_windows: the spec is closed or belongs to another context")
        if hasattr(audio, "data_ptr"):
            if audio.dim() != 2 or not audio.is_contiguous():
                raise ValueError("mel_windows: audio must be a contiguous [B, L] tensor")
            a_ptr, B, L = audio.data_ptr(), int(audio.shape[0]), int(audio.shape[1])
        else:
            a_ptr, B, L = (int(audio[0]) if audio[0] else None), int(audio[1]), int(audio[2])
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        if valid.size != B:
            raise ValueError("mel_windows: valid has %d entries for %d windows" % (valid.size, B))
        for name, v in (("window_len", L), ("n_frames", n_frames), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("mel_windows: %s is out of range" % name)
        if stream is None and hasattr(out, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(out.device)
        handle = getattr(stream, "cuda_stream", stream)
        o_ptr = out.data_ptr() if hasattr(out, "data_ptr") else (int(out) if out else None)
        self._check(lib().clx_mel_windows(self._h, spec._h, a_ptr, B, L, _np_ptr(valid), int(n_frames), int(layout), o_ptr,
                                          C.c_void_p(handle) if handle else None))
        return out

    def norm_windows(self, data, valid, layout, norm, stats=None, stream=None):
        """clx_norm_windows: the dense float32 batch `data` -- [B, rows, T] (WINDOW_CT) or [B, T, rows] (WINDOW_TC) -- normalised in
        place per window and row over the first valid[k] time steps, by `norm` (a Norm; claxon_hip.h has the definition and the order
        of the sums); every cell from valid[k] on becomes norm.pad.  `stats`, if given, is a [B, rows, 2] float32 tensor that receives
        (mean, scale) of every row.  `data` and `stats` are CUDA float32 tensors, or `data` is a (pointer, B, rows, T) tuple and
        `stats` a pointer.  Asynchronous on `stream` as gather_windows is.  Returns `data`."""
        if not isinstance(norm, Norm):
            raise ValueError("norm_windows: norm must be a Norm, not %r" % (norm,))
        tc = int(layout) == WINDOW_TC
        if hasattr(data, "data_ptr"):
            if data.dim() != 3 or not data.is_contiguous() or str(data.dtype) != "torch.float32":
                raise ValueError("norm_windows: data must be a contiguous float32 [B, rows, T] or [B, T, rows] tensor")
            d_ptr, B = data.data_ptr(), int(data.shape[0])
            rows, T = (int(data.shape[2]), int(data.shape[1])) if tc else (int(data.shape[1]), int(data.shape[2]))
        else:
            d_ptr, B, rows, T = (int(data[0]) if data[0] else None), int(data[1]), int(data[2]), int(data[3])
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        if valid.size != B:
            raise ValueError("norm_windows: valid has %d entries for %d windows" % (valid.size, B))
        for name, v in (("rows", rows), ("T", T), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("norm_windows: %s is out of range" % name)
        if hasattr(stats, "data_ptr"):
            if tuple(stats.shape) != (B, rows, 2) or not stats.is_contiguous() or str(stats.dtype) != "torch.float32":
                raise ValueError("norm_windows: stats must be a contiguous float32 [B, rows, 2] tensor")
        if stream is None and hasattr(data, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(data.device)
        handle = getattr(stream, "cuda_stream", stream)
        s_ptr = stats.data_ptr() if hasattr(stats, "data_ptr") else (int(stats) if stats else None)
        opts = norm._opts()
        self._check(lib().clx_norm_windows(self._h, d_ptr, B, rows, T, _np_ptr(valid), int(layout), C.byref(opts), s_ptr,
                                           C.c_void_p(handle) if handle else None))
        return data

    def add_windows(self, data, valid, noise, noise_valid, noise_index, snr_db, layout, gains=None, stream=None):
        """clx_add_windows: the windows of `noise` -- [N, rows, T] (WINDOW_CT) or [N, T, rows] (WINDOW_TC) -- added in place to the
        dense float32 batch `data` ([B, rows, T] / [B, T, rows], rows 1..8) at a signal-to-noise ratio: window k gets noise window
        noise_index[k] (-1: none) times the gain that puts the mean power of the signal's valid[k] live samples snr_db[k] dB above
        that of the noise samples inside them (claxon_hip.h has the definition and the order of the sums); snr_db is a scalar or
        one value per window.  Padding and the cells behind the noise's end keep their words; `noise` is not written.  `gains`, if
        given, is a [B] float32 tensor that receives every window's gain.  `data`, `noise` and `gains` are CUDA float32 tensors,
        or `data` is a (pointer, B, rows, T) tuple, `noise` a (pointer, N) pair and `gains` a pointer.  Asynchronous on `stream` as
        gather_windows is.  Returns `data`."""
        tc = int(layout) == WINDOW_TC
        if hasattr(data, "data_ptr"):
            if data.dim() != 3 or not data.is_contiguous() or str(data.dtype) != "torch.float32":
                raise ValueError("add_windows: data must be a contiguous float32 [B, rows, T] or [B, T, rows] tensor")
            d_ptr, B = data.data_ptr(), int(data.shape[0])
            rows, T = (int(data.shape[2]), int(data.shape[1])) if tc else (int(data.shape[1]), int(data.shape[2]))
        else:
            d_ptr, B, rows, T = (int(data[0]) if data[0] else None), int(data[1]), int(data[2]), int(data[3])
        if hasattr(noise, "data_ptr"):
            if noise.dim() != 3 or not noise.is_contiguous() or str(noise.dtype) != "torch.float32" \
                    or tuple(noise.shape[1:]) != ((T, rows) if tc else (rows, T)):
                raise ValueError("add_windows: noise must be a contiguous float32 [N, rows, T] or [N, T, rows] tensor with data's rows and T")
            n_ptr, N = noise.data_ptr(), int(noise.shape[0])
        elif noise is None:
            n_ptr, N = None, 0
        else:
            n_ptr, N = (int(noise[0]) if noise[0] else None), int(noise[1])
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        noise_valid = np.ascontiguousarray(noise_valid, dtype=np.uint32).reshape(-1)
        noise_index = np.ascontiguousarray(noise_index, dtype=np.int32).reshape(-1)
        snr = np.ascontiguousarray(snr_db, dtype=np.float32).reshape(-1)
        if snr.size == 1 and B != 1:
            snr = np.full(B, snr[0], dtype=np.float32)
        for name, a, want in (("valid", valid, B), ("noise_index", noise_index, B), ("snr_db", snr, B), ("noise_valid", noise_valid, N)):
            if a.size != want:
                raise ValueError("add_windows: %s has %d entries for %d windows" % (name, a.size, want))
        for name, v in (("rows", rows), ("T", T), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("add_windows: %s is out of range" % name)
        if hasattr(gains, "data_ptr"):
            if tuple(gains.shape) != (B,) or not gains.is_contiguous() or str(gains.dtype) != "torch.float32":
                raise ValueError("add_windows: gains must be a contiguous float32 [B] tensor")
        if stream is None and hasattr(data, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(data.device)
        handle = getattr(stream, "cuda_stream", stream)
        g_ptr = gains.data_ptr() if hasattr(gains, "data_ptr") else (int(gains) if gains else None)
        self._check(lib().clx_add_windows(self._h, d_ptr, B, rows, T, _np_ptr(valid), n_ptr, N, _np_ptr(noise_valid), _np_ptr(noise_index),
                                          _np_ptr(snr), int(layout), None, g_ptr, C.c_void_p(handle) if handle else None))
        return data

    def addn_windows(self, data, valid, noises, noise_valid, term_first, batch, index, offset, loop, snr_db, layout, gains=None, stream=None):
        """clx_addn_windows: several placed or looped noises added in place to the dense float32 batch `data` ([B, rows, T] for
        WINDOW_CT, [B, T, rows] for WINDOW_TC, rows 1..8) in one pass, each at its own signal-to-noise ratio against the signal as it
        arrives (claxon_hip.h has the definition and the order of the sums).  `noises` is a sequence of up to 8 noise batches with
        data's layout, rows and T; noise_valid is one array, concatenated over the batches.  Window k has the terms
        term_first[k] .. term_first[k + 1] - 1 (at most 16); term m adds noise window index[m] (-1: nothing) of batch batch[m] from
        window sample offset[m] on, looped over the rest of the window where loop[m] is 1, at snr_db[m].  batch, offset, loop and
        snr_db are scalars or one value per term.  Padding and the cells no term covers keep their words; no noise is written.
        `gains`, if given, is an [M] float32 tensor that receives every term's gain.  `data`, the noises and `gains` are CUDA
        float32 tensors, or `data` is a (pointer, B, rows, T) tuple, each noise a (pointer, N) pair and `gains` a pointer.
        Asynchronous on `stream` as gather_windows is.  Returns `data`."""
        tc = int(layout) == WINDOW_TC
        if hasattr(data, "data_ptr"):
            if data.dim() != 3 or not data.is_contiguous() or str(data.dtype) != "torch.float32":
                raise ValueError("addn_windows: data must be a contiguous float32 [B, rows, T] or [B, T, rows] tensor")
            d_ptr, B = data.data_ptr(), int(data.shape[0])
            rows, T = (int(data.shape[2]), int(data.shape[1])) if tc else (int(data.shape[1]), int(data.shape[2]))
        else:
            d_ptr, B, rows, T = (int(data[0]) if data[0] else None), int(data[1]), int(data[2]), int(data[3])
        noises = list(noises)
        ptrs, counts = (C.c_void_p * max(len(noises), 1))(), (C.c_size_t * max(len(noises), 1))()
        for b, noise in enumerate(noises):
            if hasattr(noise, "data_ptr"):
                if noise.dim() != 3 or not noise.is_contiguous() or str(noise.dtype) != "torch.float32" \
                        or tuple(noise.shape[1:]) != ((T, rows) if tc else (rows, T)):
                    raise ValueError("addn_windows: a noise batch must be a contiguous float32 [N, rows, T] or [N, T, rows] tensor with data's rows and T")
                ptrs[b], counts[b] = noise.data_ptr() or None, int(noise.shape[0])
            else:
                ptrs[b], counts[b] = (int(noise[0]) if noise[0] else None), int(noise[1])
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        noise_valid = np.ascontiguousarray(noise_valid, dtype=np.uint32).reshape(-1)
        term_first = np.ascontiguousarray(term_first, dtype=np.uint32).reshape(-1)
        if valid.size != B:
            raise ValueError("addn_windows: valid has %d entries for %d windows" % (valid.size, B))
        if term_first.size != B + 1:
            raise ValueError("addn_windows: term_first has %d entries for %d windows" % (term_first.size, B))
        if noise_valid.size != sum(counts[:len(noises)]):
            raise ValueError("addn_windows: noise_valid has %d entries for %d windows" % (noise_valid.size, sum(counts[:len(noises)])))
        M = int(term_first[-1])
        terms = np.zeros(M, dtype=ADDN_TERM_DTYPE)
        for name, a, dt in (("batch", batch, np.int32), ("index", index, np.int32), ("offset", offset, np.uint32), ("loop", loop, np.uint32),
                            ("snr_db", snr_db, np.float32)):
            wide = np.asarray(a, dtype=np.float32 if dt is np.float32 else np.int64).reshape(-1)
            if dt is not np.float32 and wide.size and (wide.min() < np.iinfo(dt).min or wide.max() > np.iinfo(dt).max):
                raise ValueError("addn_windows: %s is out of range" % name)
            if wide.size == 1 and M != 1 and name != "index":
                wide = np.full(M, wide[0])
            if wide.size != M:
                raise ValueError("addn_windows: %s has %d entries for %d terms" % (name, wide.size, M))
            terms[name] = wide.astype(dt)
        for name, v in (("rows", rows), ("T", T), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("addn_windows: %s is out of range" % name)
        if hasattr(gains, "data_ptr"):
            if gains.numel() != M or not gains.is_contiguous() or str(gains.dtype) != "torch.float32":
                raise ValueError("addn_windows: gains must be a contiguous float32 tensor of one value per term")
        if stream is None and hasattr(data, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(data.device)
        handle = getattr(stream, "cuda_stream", stream)
        g_ptr = gains.data_ptr() if hasattr(gains, "data_ptr") else (int(gains) if gains else None)
        self._check(lib().clx_addn_windows(self._h, d_ptr, B, rows, T, _np_ptr(valid), ptrs, counts, len(noises), _np_ptr(noise_valid),
                                           _np_ptr(term_first), _np_ptr(terms), int(layout), None, g_ptr, C.c_void_p(handle) if handle else None))
        return data

    def reverb_windows(self, data, valid, ir, ir_len, ir_index, layout, out=None, keep_power=True, gains=None, stream=None, method="direct"):
        """clx_reverb_windows: the dense float32 batch `data` -- [B, rows, T] (WINDOW_CT) or [B, T, rows] (WINDOW_TC), rows 1..8 --
        convolved with the mono impulse responses `ir` ([N, K] float32, row j live for ir_len[j] taps), out of place: window k gets
        response ir_index[k] (-1: none, a copy) on every row, as the ascending chain of fused multiply-adds that claxon_hip.h
        defines; the window is the crop, cells from valid[k] on become zero.  keep_power=True then rescales every window to the power
        of its dry signal (lhotse's normalize_output).  `out` has data's shape and must not overlap it (None: a new tensor);
        `gains`, if given, is a [B] float32 tensor that receives every window's scale, 1 where nothing was scaled.  `data`, `ir`,
        `out` and `gains` are CUDA float32 tensors, or `data` is a (pointer, B, rows, T) tuple, `ir` a (pointer, N, K) triple and
        `out` and `gains` pointers.  `data` and `ir` are not written.  Asynchronous on `stream` as gather_windows is.  Returns `out`.
        method="fft" is clx_reverb_windows_fft: the same arguments, refusals and keep_power, the cells by uniformly partitioned
        overlap-save as claxon_hip.h defines it -- close to the direct form's, not its words; method="auto" takes it from REVERB_FFT_TAPS
        taps (K) on and the direct form below; ValueError for any other method."""
        _reverb_method(method, "reverb_windows")
        tc = int(layout) == WINDOW_TC
        if hasattr(data, "data_ptr"):
            if data.dim() != 3 or not data.is_contiguous() or str(data.dtype) != "torch.float32":
                raise ValueError("reverb_windows: data must be a contiguous float32 [B, rows, T] or [B, T, rows] tensor")
            d_ptr, B = data.data_ptr(), int(data.shape[0])
            rows, T = (int(data.shape[2]), int(data.shape[1])) if tc else (int(data.shape[1]), int(data.shape[2]))
            if out is None:
                import torch
                out = torch.empty_like(data)
        else:
            d_ptr, B, rows, T = (int(data[0]) if data[0] else None), int(data[1]), int(data[2]), int(data[3])
        if hasattr(out, "data_ptr"):
            if not hasattr(data, "data_ptr") or tuple(out.shape) != tuple(data.shape) or not out.is_contiguous() or str(out.dtype) != "torch.float32":
                raise ValueError("reverb_windows: out must be a contiguous float32 tensor of data's shape")
        if hasattr(ir, "data_ptr"):
            if ir.dim() != 2 or not ir.is_contiguous() or str(ir.dtype) != "torch.float32":
                raise ValueError("reverb_windows: ir must be a contiguous float32 [N, K] tensor")
            i_ptr, N, K = ir.data_ptr(), int(ir.shape[0]), int(ir.shape[1])
        elif ir is None:
            i_ptr, N, K = None, 0, 1
        else:
            i_ptr, N, K = (int(ir[0]) if ir[0] else None), int(ir[1]), int(ir[2])
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        ir_len = np.ascontiguousarray(ir_len if ir_len is not None else [], dtype=np.uint32).reshape(-1)
        ir_index = np.ascontiguousarray(ir_index, dtype=np.int32).reshape(-1)
        for name, a, want in (("valid", valid, B), ("ir_index", ir_index, B), ("ir_len", ir_len, N)):
            if a.size != want:
                raise ValueError("reverb_windows: %s has %d entries for %d windows" % (name, a.size, want))
        for name, v in (("rows", rows), ("T", T), ("K", K), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("reverb_windows: %s is out of range" % name)
        if hasattr(gains, "data_ptr"):
            if tuple(gains.shape) != (B,) or not gains.is_contiguous() or str(gains.dtype) != "torch.float32":
                raise ValueError("reverb_windows: gains must be a contiguous float32 [B] tensor")
        if stream is None and hasattr(data, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(data.device)
        handle = getattr(stream, "cuda_stream", stream)
        o_ptr = out.data_ptr() if hasattr(out, "data_ptr") else (int(out) if out else None)
        g_ptr = gains.data_ptr() if hasattr(gains, "data_ptr") else (int(gains) if gains else None)
        if reverb_method_for(method, K) == "fft":
            opts, call = _ReverbFftOpts(1 if keep_power else 0), lib().clx_reverb_windows_fft
        else:
            opts, call = _ReverbOpts(1 if keep_power else 0, 0), lib().clx_reverb_windows
        self._check(call(self._h, d_ptr, B, rows, T, _np_ptr(valid), i_ptr, N, K, _np_ptr(ir_len), _np_ptr(ir_index),
                         int(layout), C.byref(opts), o_ptr, g_ptr, C.c_void_p(handle) if handle else None))
        return out

    def specaug_windows(self, data, valid, layout, warp=None, freq_masks=None, time_masks=None, fill="mean", out=None, fills=None, stream=None):
        """clx_specaug_windows: SpecAugment of the dense float32 feature batch `data` -- [B, rows, T] (WINDOW_CT) or [B, T, rows]
        (WINDOW_TC), rows 1..256 --, out of place: window k's first valid[k] frames are warped in time about the pair warp[k] =
        (c, w) (output frames [0, w) are input frames [0, c) resized by the bicubic rule of claxon_hip.h, [w, valid[k]) are
        [c, valid[k]); (0, 0): no warp), then the rows of freq_masks[k] ([F, 2]: first row, width) and the frames of
        time_masks[k] ([M, 2]: first output frame, width; F, M <= 32) become the fill: a float, or "mean", the mean of the window's
        live input cells.  Frames from valid[k] on are copied as they are.  warp is [B, 2], freq_masks [B, F, 2], time_masks
        [B, M, 2], whole numbers that are not negative; each may be None.  `out` has data's shape and must not be data (None: a
        new tensor); `fills`, if given, is a [B] float32 tensor that receives every window's fill.  `data`, `out` and `fills`
        are CUDA float32 tensors, or `data` is a (pointer, B, rows, T) tuple and `out` and `fills` pointers.  `data` is not
        written.  Asynchronous on `stream` as gather_windows is.  Returns `out`."""
        tc = int(layout) == WINDOW_TC
        if hasattr(data, "data_ptr"):
            if data.dim() != 3 or not data.is_contiguous() or str(data.dtype) != "torch.float32":
                raise ValueError("specaug_windows: data must be a contiguous float32 [B, rows, T] or [B, T, rows] tensor")
            d_ptr, B = data.data_ptr(), int(data.shape[0])
            rows, T = (int(data.shape[2]), int(data.shape[1])) if tc else (int(data.shape[1]), int(data.shape[2]))
            if out is None:
                import torch
                out = torch.empty_like(data)
        else:
            d_ptr, B, rows, T = (int(data[0]) if data[0] else None), int(data[1]), int(data[2]), int(data[3])
        if hasattr(out, "data_ptr"):
            if not hasattr(data, "data_ptr") or tuple(out.shape) != tuple(data.shape) or not out.is_contiguous() or str(out.dtype) != "torch.float32":
                raise ValueError("specaug_windows: out must be a contiguous float32 tensor of data's shape")
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        if valid.size != B:
            raise ValueError("specaug_windows: valid has %d entries for %d windows" % (valid.size, B))
        warp = _specaug_table(warp, B, "warp", pairs=False)
        fm = _specaug_table(freq_masks, B, "freq_masks")
        tm = _specaug_table(time_masks, B, "time_masks")
        for name, v in (("rows", rows), ("T", T), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("specaug_windows: %s is out of range" % name)
        mean, value = _specaug_fill(fill, "specaug_windows")
        if hasattr(fills, "data_ptr"):
            if tuple(fills.shape) != (B,) or not fills.is_contiguous() or str(fills.dtype) != "torch.float32":
                raise ValueError("specaug_windows: fills must be a contiguous float32 [B] tensor")
        if stream is None and hasattr(data, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(data.device)
        handle = getattr(stream, "cuda_stream", stream)
        o_ptr = out.data_ptr() if hasattr(out, "data_ptr") else (int(out) if out else None)
        f_ptr = fills.data_ptr() if hasattr(fills, "data_ptr") else (int(fills) if fills else None)
        opts = _SpecAugOpts(0 if fm is None else fm.shape[1], 0 if tm is None else tm.shape[1], 1 if mean else 0, value, 0)
        self._check(lib().clx_specaug_windows(self._h, d_ptr, o_ptr, B, rows, T, _np_ptr(valid), int(layout),
                                              None if warp is None else _np_ptr(warp), None if fm is None else _np_ptr(fm),
                                              None if tm is None else _np_ptr(tm), C.byref(opts), f_ptr,
                                              C.c_void_p(handle) if handle else None))
        return out

    def splice_windows(self, data, valid, layout, splice, out=None, stream=None):
        """clx_splice_windows: the dense float32 feature batch `data` -- [B, rows, T] (WINDOW_CT) or [B, T, rows] (WINDOW_TC), rows
        1..256 -- spliced by `splice` (a Splice: deltas, context frames, subsampling, low-frame-rate stacking), out of place: window
        k's first valid[k] frames give its first splice.frames_out(valid[k]) output frames of splice.n_out(rows) rows, every tap
        clamped into [0, valid[k]) (the edge frame repeated; claxon_hip.h has the definition and the order of the taps); the
        output frames from there on are splice.pad.  `out` is [B, splice.n_out(rows), splice.frames_out(T)] (CT) or the same
        transposed (TC) and must not be data (None: a new tensor).  `data` and `out` are CUDA float32 tensors, or `data` is a
        (pointer, B, rows, T) tuple and `out` a pointer.  `data` is not written, and nothing of it from valid[k] on is read.
        Asynchronous on `stream` as gather_windows is.  Returns `out`.  read_mel(..., splice=) runs this before normalize=; whoever
        wants CMVN in front of the deltas calls norm_windows and then this."""
        if not isinstance(splice, Splice):
            raise ValueError("splice_windows: splice must be a Splice, not %r" % (splice,))
        tc = int(layout) == WINDOW_TC
        if hasattr(data, "data_ptr"):
            if data.dim() != 3 or not data.is_contiguous() or str(data.dtype) != "torch.float32":
                raise ValueError("splice_windows: data must be a contiguous float32 [B, rows, T] or [B, T, rows] tensor")
            d_ptr, B = data.data_ptr(), int(data.shape[0])
            rows, T = (int(data.shape[2]), int(data.shape[1])) if tc else (int(data.shape[1]), int(data.shape[2]))
        else:
            d_ptr, B, rows, T = (int(data[0]) if data[0] else None), int(data[1]), int(data[2]), int(data[3])
        for name, v in (("rows", rows), ("T", T), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("splice_windows: %s is out of range" % name)
        shape = (B, splice.frames_out(T), splice.n_out(rows)) if tc else (B, splice.n_out(rows), splice.frames_out(T))
        if hasattr(data, "data_ptr") and out is None:
            import torch
            out = torch.empty(shape, dtype=torch.float32, device=data.device)
        if hasattr(out, "data_ptr"):
            if not hasattr(data, "data_ptr") or tuple(out.shape) != shape or not out.is_contiguous() or str(out.dtype) != "torch.float32":
                raise ValueError("splice_windows: out must be a contiguous float32 tensor of shape %r" % (shape,))
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        if valid.size != B:
            raise ValueError("splice_windows: valid has %d entries for %d windows" % (valid.size, B))
        if stream is None and hasattr(data, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(data.device)
        handle = getattr(stream, "cuda_stream", stream)
        o_ptr = out.data_ptr() if hasattr(out, "data_ptr") else (int(out) if out else None)
        blocks, coefs = splice._tables()
        opts = _SpliceOpts(len(splice.blocks), splice.stride, splice.pad, 0)
        self._check(lib().clx_splice_windows(self._h, d_ptr, o_ptr, B, rows, T, _np_ptr(valid), int(layout), _np_ptr(blocks),
                                             _np_ptr(coefs) if coefs.size else None, C.byref(opts), C.c_void_p(handle) if handle else None))
        return out

    def cmvn_windows(self, data, valid, layout, cmvn, out=None, stream=None, groups=None):
        """clx_cmvn_global_windows or clx_cmvn_sliding_windows, as `cmvn` (a Cmvn) says, over the dense float32 feature batch `data`
        -- [B, rows, T] (WINDOW_CT) or [B, T, rows] (WINDOW_TC), rows 1..8192 -- and the first valid[k] frames of window k
        (claxon_hip.h has the definitions, the statistics window and the order of the sums); every frame from valid[k] on becomes
        cmvn.pad.  A global Cmvn (cmvn.rows == rows) works in place: `out` must be None, and `data` is returned.  A sliding one is
        out of place: `out` has data's shape and must not be data (None: a new tensor), `data` is not written and nothing of it
        from valid[k] on is read; `out` is returned.  `data` and `out` are CUDA float32 tensors, or `data` is a (pointer, B, rows, T)
        tuple and `out` a pointer.  A grouped Cmvn (Cmvn.grouped(stats)) works in place like a global one, by
        clx_cmvn_grouped_windows: window k is normalised by the accumulator of group groups[k] of the Cmvn's CmvnStats as it stands
        when the launch runs (-1: the window keeps its live cells and gets its padding; groups=None: every window group 0, for a
        CmvnStats of one group only).  groups= goes with a grouped Cmvn alone.  Asynchronous on `stream` as gather_windows is."""
        if not isinstance(cmvn, Cmvn):
            raise ValueError("cmvn_windows: cmvn must be a Cmvn, not %r" % (cmvn,))
        if groups is not None and cmvn._stats is None:
            raise ValueError("cmvn_windows: groups= goes with a grouped Cmvn (Cmvn.grouped), not %r" % (cmvn,))
        tc = int(layout) == WINDOW_TC
        if hasattr(data, "data_ptr"):
            if data.dim() != 3 or not data.is_contiguous() or str(data.dtype) != "torch.float32":
                raise ValueError("cmvn_windows: data must be a contiguous float32 [B, rows, T] or [B, T, rows] tensor")
            d_ptr, B = data.data_ptr(), int(data.shape[0])
            rows, T = (int(data.shape[2]), int(data.shape[1])) if tc else (int(data.shape[1]), int(data.shape[2]))
        else:
            d_ptr, B, rows, T = (int(data[0]) if data[0] else None), int(data[1]), int(data[2]), int(data[3])
        for name, v in (("rows", rows), ("T", T), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("cmvn_windows: %s is out of range" % name)
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        if valid.size != B:
            raise ValueError("cmvn_windows: valid has %d entries for %d windows" % (valid.size, B))
        if stream is None and hasattr(data, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(data.device)
        handle = getattr(stream, "cuda_stream", stream)
        handle = C.c_void_p(handle) if handle else None
        if cmvn._stats is not None:
            st = cmvn._stats
            st._open("a grouped Cmvn")
            if out is not None:
                raise ValueError("cmvn_windows: a grouped Cmvn works in place: out must be None")
            if cmvn.rows != rows:
                raise ValueError("cmvn_windows: the Cmvn has %d rows, the batch %d" % (cmvn.rows, rows))
            if groups is None and st.groups > 1:
                raise ValueError("cmvn_windows: the Cmvn's CmvnStats has %d groups: give groups=" % st.groups)
            g = _cmvn_groups("cmvn_windows", groups, B, st.groups)
            opts = _CmvnGroupedOpts(int(cmvn.norm_vars), cmvn.pad, 0)
            self._check(lib().clx_cmvn_grouped_windows(self._h, d_ptr, B, rows, T, _np_ptr(valid), int(layout), _np_ptr(g) if g is not None else None,
                                                       st.groups, st._acc.data_ptr(), st._shift_scale().data_ptr(), C.byref(opts), handle))
            return data
        if cmvn.rows is not None:
            if out is not None:
                raise ValueError("cmvn_windows: a global Cmvn works in place: out must be None")
            if cmvn.rows != rows:
                raise ValueError("cmvn_windows: the Cmvn has %d rows, the batch %d" % (cmvn.rows, rows))
            opts = _CmvnGlobalOpts(cmvn.pad, 0)
            self._check(lib().clx_cmvn_global_windows(self._h, d_ptr, B, rows, T, _np_ptr(valid), int(layout), _np_ptr(cmvn._shift),
                                                      _np_ptr(cmvn._scale), C.byref(opts), handle))
            return data
        shape = (B, T, rows) if tc else (B, rows, T)
        if hasattr(data, "data_ptr") and out is None:
            import torch
            out = torch.empty(shape, dtype=torch.float32, device=data.device)
        if hasattr(out, "data_ptr"):
            if not hasattr(data, "data_ptr") or tuple(out.shape) != shape or not out.is_contiguous() or str(out.dtype) != "torch.float32":
                raise ValueError("cmvn_windows: out must be a contiguous float32 tensor of shape %r" % (shape,))
        o_ptr = out.data_ptr() if hasattr(out, "data_ptr") else (int(out) if out else None)
        opts = cmvn._sliding_opts()
        self._check(lib().clx_cmvn_sliding_windows(self._h, d_ptr, o_ptr, B, rows, T, _np_ptr(valid), int(layout), C.byref(opts), handle))
        return out

    def _feature_batch(self, who, data, valid, layout, stream):
        """(pointer, B, rows, T, valid as uint32, stream handle) of a dense float32 feature batch: a CUDA tensor or a (pointer, B, rows,
        T) tuple, as the *_windows methods take them."""
        tc = int(layout) == WINDOW_TC
        if hasattr(data, "data_ptr"):
            if data.dim() != 3 or not data.is_contiguous() or str(data.dtype) != "torch.float32":
                raise ValueError("%s: data must be a contiguous float32 [B, rows, T] or [B, T, rows] tensor" % who)
            d_ptr, B = data.data_ptr(), int(data.shape[0])
            rows, T = (int(data.shape[2]), int(data.shape[1])) if tc else (int(data.shape[1]), int(data.shape[2]))
        else:
            d_ptr, B, rows, T = (int(data[0]) if data[0] else None), int(data[1]), int(data[2]), int(data[3])
        for name, v in (("rows", rows), ("T", T), ("layout", layout)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError("%s: %s is out of range" % (who, name))
        valid = np.ascontiguousarray(valid, dtype=np.uint32).reshape(-1)
        if valid.size != B:
            raise ValueError("%s: valid has %d entries for %d windows" % (who, valid.size, B))
        if stream is None and hasattr(data, "data_ptr"):
            import torch
            stream = torch.cuda.current_stream(data.device)
        handle = getattr(stream, "cuda_stream", stream)
        return d_ptr, B, rows, T, valid, (C.c_void_p(handle) if handle else None)

    def vad_windows(self, data, valid, layout, vad, mask=None, thresholds=None, stream=None):
        """clx_vad_windows: Kaldi's energy VAD (compute-vad, as this project reads it) over row vad.row of the dense float32 feature
        batch `data` -- [B, rows, T] (WINDOW_CT) or [B, T, rows] (WINDOW_TC), rows 1..8192 -- and the first valid[k] frames of window
        k: byte 1 for a voiced frame, 0 for an unvoiced one and for every frame from valid[k] on (claxon_hip.h has the definition and
        the order of the sum behind the threshold).  `vad` is a Vad; its select and pad are not read here.  mask is a uint8 [B, T]
        CUDA tensor (None: a new one), thresholds an optional float32 [B] CUDA tensor that receives each window's threshold; with a
        (pointer, B, rows, T) tuple for `data` both are pointers and mask must be given.  `data` is not written; nothing of it from
        valid[k] on and no other row is read.  Asynchronous on `stream` as gather_windows is.  Returns mask."""
        if not isinstance(vad, Vad):
            raise ValueError("vad_windows: vad must be a Vad, not %r" % (vad,))
        d_ptr, B, rows, T, valid, handle = self._feature_batch("vad_windows", data, valid, layout, stream)
        if vad.row >= rows:
            raise ValueError("vad_windows: the Vad reads row %d, the batch has %d" % (vad.row, rows))
        if hasattr(data, "data_ptr") and mask is None:
            import torch
            mask = torch.empty((B, T), dtype=torch.uint8, device=data.device)
        if hasattr(mask, "data_ptr"):
            if tuple(mask.shape) != (B, T) or not mask.is_contiguous() or str(mask.dtype) != "torch.uint8":
                raise ValueError("vad_windows: mask must be a contiguous uint8 tensor of shape %r" % ((B, T),))
        if hasattr(thresholds, "data_ptr"):
            if tuple(thresholds.shape) != (B,) or not thresholds.is_contiguous() or str(thresholds.dtype) != "torch.float32":
                raise ValueError("vad_windows: thresholds must be a contiguous float32 [B] tensor")
        m_ptr = mask.data_ptr() if hasattr(mask, "data_ptr") else (int(mask) if mask else None)
        t_ptr = thresholds.data_ptr() if hasattr(thresholds, "data_ptr") else (int(thresholds) if thresholds else None)
        opts = vad._opts()
        self._check(lib().clx_vad_windows(self._h, d_ptr, B, rows, T, _np_ptr(valid), int(layout), C.byref(opts), m_ptr, t_ptr, handle))
        return mask

    def select_windows(self, data, valid, mask, layout, pad=0.0, out=None, stream=None):
        """clx_select_windows: of the first valid[k] frames of window k of the dense float32 feature batch `data` -- [B, rows, T]
        (WINDOW_CT) or [B, T, rows] (WINDOW_TC), rows 1..8192 -- those whose byte of `mask` (uint8 [B, T]: vad_windows', or any
        other) is not 0, moved to the front in their order, every row's words as they are; the frames behind them are `pad`.  Out
        of place: `out` has data's shape and must not overlap it (None: a new tensor); `data` is not written, and neither it nor
        the mask is read from valid[k] on.  `data`, `mask` and `out` are CUDA tensors, or `data` is a (pointer, B, rows, T) tuple and
        the other two pointers.  Returns (out, counts): counts[k] (a host int64 numpy array) is the number of frames kept, the new
        valid[k]; 0 is a window that is all pad.  THE CALL WAITS for its own launches and for those B words to arrive; everything
        else here is asynchronous on `stream` as gather_windows is."""
        d_ptr, B, rows, T, valid, handle = self._feature_batch("select_windows", data, valid, layout, stream)
        if isinstance(pad, bool) or not isinstance(pad, (int, float, np.integer, np.floating)):
            raise ValueError("select_windows: pad must be a number, not %r" % (pad,))
        shape = (B, T, rows) if int(layout) == WINDOW_TC else (B, rows, T)
        if hasattr(mask, "data_ptr"):
            if tuple(mask.shape) != (B, T) or not mask.is_contiguous() or str(mask.dtype) != "torch.uint8":
                raise ValueError("select_windows: mask must be a contiguous uint8 tensor of shape %r" % ((B, T),))
        if hasattr(data, "data_ptr") and out is None:
            import torch
            out = torch.empty(shape, dtype=torch.float32, device=data.device)
        if hasattr(out, "data_ptr"):
            if not hasattr(data, "data_ptr") or tuple(out.shape) != shape or not out.is_contiguous() or str(out.dtype) != "torch.float32":
                raise ValueError("select_windows: out must be a contiguous float32 tensor of shape %r" % (shape,))
        m_ptr = mask.data_ptr() if hasattr(mask, "data_ptr") else (int(mask) if mask else None)
        o_ptr = out.data_ptr() if hasattr(out, "data_ptr") else (int(out) if out else None)
        with np.errstate(over="ignore"):
            opts = _SelectOpts(float(np.float32(pad)), (C.c_uint32 * 3)(0, 0, 0))
        counts = np.zeros(B, dtype=np.uint32)
        self._check(lib().clx_select_windows(self._h, d_ptr, o_ptr, B, rows, T, _np_ptr(valid), m_ptr, int(layout), C.byref(opts), None,
                                             _np_ptr(counts) if B else None, handle))
        return out, counts.astype(np.int64)

    def decode_subframes(self, arena, offs, block_sizes, bps, out_offs, out=None):
        a = _u8(arena)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        bsz = np.ascontiguousarray(block_sizes, dtype=np.uint16)
        bp = np.ascontiguousarray(bps, dtype=np.uint8)
        out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
        n = offs.size
        total = int((out_offs + bsz.astype(np.uint64)).max()) if n else 0
        if out is None:
            out = np.zeros(total, dtype=np.int32)
        res = np.zeros(n, dtype=FRAME_RESULT_DTYPE)
        st = lib().clx_decode_subframes(self._h, _np_ptr(a), a.size, _np_ptr(offs), _np_ptr(bsz), _np_ptr(bp), n,
                                        _np_ptr(out), _np_ptr(out_offs), _np_ptr(res), 0)
        self._check(st)
        return out, res

    def plan(self, descs, out_offs, verify_crc=False, path=0):
        """path: 0 = automatic, PATH_WAVES or PATH_LANES to force a kernel path."""
        return Batch(self, descs, out_offs, verify_crc, path)


class Batch:
    """clx_batch: a planned batch, run on device-resident buffers (what bench.py times)."""

    def __init__(self, ctx, descs, out_offs, verify_crc=False, path=0):
        self.ctx = ctx
        descs = np.ascontiguousarray(descs, dtype=FRAME_DESC_DTYPE)
        out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
        self.n = descs.size
        self._h = C.c_void_p(None)
        st = lib().clx_batch_create(ctx._h, _np_ptr(descs), self.n, _np_ptr(out_offs),
                                    (VERIFY_CRC16 if verify_crc else 0) | path, C.byref(self._h))
        ctx._check(st)

    @property
    def slots(self):
        return int(lib().clx_batch_slots(self._h))

    def run(self, d_arena_ptr, arena_len, d_out_ptr, stream=0):
        """d_arena_ptr / d_out_ptr: integer device addresses (e.g. torch tensor .data_ptr())."""
        st = lib().clx_batch_run(self._h, C.c_void_p(d_arena_ptr), arena_len, C.c_void_p(d_out_ptr),
                                 C.c_void_p(stream) if stream else None)
        self.ctx._check(st)

    def submit(self, d_arena_ptr, arena_len, d_out_ptr, stream=0):
        """Pipelined run (clx_batch_submit): up to self.submit_depth submissions in flight on internal streams.  Rotate over
        that many output buffers; flush() (or results()) before reading them."""
        st = lib().clx_batch_submit(self._h, C.c_void_p(d_arena_ptr), arena_len, C.c_void_p(d_out_ptr),
                                    C.c_void_p(stream) if stream else None)
        self.ctx._check(st)

    @property
    def submit_depth(self):
        """Submissions this batch keeps in flight = output buffers to rotate over (clx_batch_submit_depth)."""
        return int(lib().clx_batch_submit_depth(self._h))

    @property
    def submit_lanes(self):
        """True when this batch's pipelined submissions run the fused lane kernels (clx_batch_submit_lanes)."""
        return bool(lib().clx_batch_submit_lanes(self._h))

    @property
    def submit_merge(self):
        """How many consecutive submissions go out as one launch (clx_batch_submit_merge)."""
        return int(lib().clx_batch_submit_merge(self._h))

    def flush(self, stream=0):
        self.ctx._check(lib().clx_batch_flush(self._h, C.c_void_p(stream) if stream else None))

    def interleave(self, d_planar_ptr, d_pcm_ptr, sample_bytes, stream=0):
        """Device-resident interleave / narrow stage after run(): integer device addresses, async on `stream`."""
        st = lib().clx_batch_interleave(self._h, C.c_void_p(d_planar_ptr), C.c_void_p(d_pcm_ptr), sample_bytes,
                                        C.c_void_p(stream) if stream else None)
        self.ctx._check(st)

    def results(self):
        res = np.zeros(self.n, dtype=FRAME_RESULT_DTYPE)
        self.ctx._check(lib().clx_batch_results(self._h, _np_ptr(res)))
        return res

    def set_profiling(self, on=True):
        """True / 1: plain runs with per-kernel events; 2: pipelined submissions, events around the kernels of each merged launch."""
        lib().clx_batch_set_profiling(self._h, int(on) if not isinstance(on, bool) else (1 if on else 0))

    def kernel_ms(self, kernel):
        ms = C.c_float(0)
        self.ctx._check(lib().clx_batch_kernel_ms(self._h, kernel, C.byref(ms)))
        return float(ms.value)

    def kernel_times(self):
        """{kernel name: ms} of the last profiled run, in launch order."""
        out, k = {}, 0
        while True:
            name = lib().clx_batch_kernel_name(self._h, k)
            if not name:
                return out
            out[name.decode()] = self.kernel_ms(k)
            k += 1

    def close(self):
        if self._h:
            lib().clx_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Block:
    """frame.rs:402-529"""

    def __init__(self, time, block_size, channels, buffer):
        self._time, self._bs, self._ch, self._buf = time, block_size, channels, buffer

    def time(self):
        return self._time

    def len(self):
        return self._bs * self._ch

    def duration(self):
        return self._bs

    def channels(self):
        return self._ch

    def channel(self, ch):
        if ch >= self._ch:
            raise IndexError(ch)
        return self._buf[ch * self._bs:(ch + 1) * self._bs]

    def sample(self, ch, i):
        return int(self._buf[ch * self._bs + i])

    def into_buffer(self):
        return self._buf

    def stereo_samples(self):
        if self._ch != 2:
            raise ValueError("stereo_samples() must only be called for blocks with two channels.")
        return zip(self._buf[:self._bs].tolist(), self._buf[self._bs:2 * self._bs].tolist())


class FlacReader:
    """lib.rs:93-97, 207-471 over an in-memory stream; frames are decoded on the GPU in batches."""

    def __init__(self, ctx, data=None, path=None):
        self.ctx = ctx
        self._h = C.c_void_p(None)
        m = C.c_uint32(0)
        if path is not None:
            st = lib().clx_reader_open(ctx._h, os.fsencode(path), C.byref(self._h), C.byref(m))
        else:
            a = _u8(data)
            st = lib().clx_reader_new(ctx._h, _np_ptr(a), a.size, C.byref(self._h), C.byref(m))
        if st != OK:
            self._h = None
            raise ClaxonError(st, int(m.value))
        self._si = StreamInfo()
        self._buf = None
        lib().clx_reader_streaminfo(self._h, C.byref(self._si))

    @classmethod
    def open(cls, ctx, path):
        return cls(ctx, path=path)

    def streaminfo(self):
        return self._si

    def vendor(self):
        """lib.rs:321: the encoder's vendor string (str), or None when the stream has no Vorbis comment block."""
        v, _ = _tags_to_py(lib().clx_reader_tags(self._h))
        return None if v is None else v.decode("utf-8")

    def tags(self):
        """lib.rs:335: (name, value) pairs in stream order."""
        _, t = _tags_to_py(lib().clx_reader_tags(self._h))
        return [(n.decode("utf-8"), v.decode("utf-8")) for n, v in t]

    def get_tag(self, name):
        """lib.rs:356: every value of the tag `name` (ASCII-case-insensitive), in stream order."""
        t = lib().clx_reader_tags(self._h)
        return [v.decode("utf-8") for v in _tags_lookup(t, name)] if t else []

    def read_next_or_eof(self):
        """Returns a Block, or None at the end of the stream; raises ClaxonError like the reference returns Err."""
        # one staging buffer per reader, sized from STREAMINFO (max block size x channels); a block that is larger than announced
        # stays pending in the library and is fetched again into a buffer of the size it reports
        if self._buf is None:
            si = self._si
            self._buf = np.empty(max(1, int(si.max_block_size or 65535) * int(si.channels or 8)), dtype=np.int32)
        buf = self._buf
        info = BlockInfo()
        m = C.c_uint32(0)
        st = lib().clx_reader_next_block(self._h, _np_ptr(buf), buf.size, C.byref(info), C.byref(m))
        if st == API_ERROR and info.block_size * info.channels > buf.size:
            self._buf = buf = np.empty(int(info.block_size) * int(info.channels), dtype=np.int32)
            st = lib().clx_reader_next_block(self._h, _np_ptr(buf), buf.size, C.byref(info), C.byref(m))
        if st == END_OF_STREAM:
            return None
        if st != OK:
            raise ClaxonError(st, int(m.value), self.ctx.last_error() if st == API_ERROR else None)
        n = info.block_size * info.channels
        return Block(info.time, info.block_size, info.channels, buf[:n].copy())

    def blocks(self):
        while True:
            b = self.read_next_or_eof()
            if b is None:
                return
            yield b

    def samples(self):
        """Interleaved samples (lib.rs:473-520)."""
        for b in self.blocks():
            inter = b.into_buffer().reshape(b.channels(), b.duration()).T.reshape(-1)
            for s in inter.tolist():
                yield s

    def close(self):
        if self._h:
            lib().clx_reader_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- whole streams to float tensors on the GPU ----------------------------------------------------------------------------------

INDEX_CALL_BYTES = (1 << 32) - 64       # clx_index_streams_device takes an arena below 4 GiB per call


def _index_arena(ctx, arena, offs, lens, starts, limit=INDEX_CALL_BYTES):
    """Context.index_streams over the device arena `arena`: (descs, first_frame, stop_offs).  One call, unless the streams span more
    than a call takes (`limit` bytes): then one call per run of streams that fits, each on its own slice of the tensor, the answers
    rebased and joined.  (A single stream beyond the limit is refused by the call.)"""
    n = len(offs)
    if n == 0 or offs[-1] + lens[-1] <= limit:
        d, _, first, stops = ctx.index_streams(arena, offs, lens, starts)
        return d, first, stops
    descs, first, stops, j = [], [0], [], 0
    while j < n:
        g0, e = offs[j], j + 1
        while e < n and offs[e] + lens[e] - g0 <= limit:
            e += 1
        sub = arena[g0:min(((offs[e - 1] + lens[e - 1] + 15) // 16) * 16 + 32, arena.numel())]
        d, _, f, s = ctx.index_streams(sub, [o - g0 for o in offs[j:e]], lens[j:e], starts[j:e])
        d["byte_off"] += np.uint64(g0)
        descs.append(d)
        first.extend((f[1:].astype(np.int64) + first[-1]).tolist())
        stops.extend((s.astype(np.int64) + g0).tolist())
        j = e
    return np.concatenate(descs), np.array(first, dtype=np.uint64), np.array(stops, dtype=np.uint64)


def _index_streams(ctx, arrs, short=None):
    """Whole FLAC streams `arrs` (uint8) made ready to decode: their headers parsed on the host, the streams whose header parses laid
    out in one arena at 16-byte aligned places, that arena uploaded once and indexed with one Context.index_streams call.  Returns
    (arena tensor | None, arena length, entries): entries[k] is (descs, sample_rate, channels, STREAMINFO) -- the descriptors address
    the arena and read no further than the stream's own end -- or the ClaxonError that stream raises.  Bytes the indexer cannot chain
    up (a damaged or truncated frame) become one more descriptor when they start with a valid frame header, so that decoding reports
    that frame's error as the reference's reader would; a header that does not parse there is the stream's error.  `short`: a list that
    gets, for every stream with an entry of descriptors, (k, byte of the stream where its index stopped) when that is not its end."""
    entries, live, offs, starts, infos, base = [None] * len(arrs), [], [], [], [], 0
    for k, a in enumerate(arrs):
        st, msg, si, off = read_stream_header(a)
        if st != OK:
            entries[k] = ClaxonError(st, msg)
            continue
        live.append(k); offs.append(base); starts.append(off); infos.append(si)
        base = ((base + a.size + 15) // 16) * 16
    if not live:
        return None, 0, entries
    arena = _arena_on_device(ctx, [(o, arrs[k]) for o, k in zip(offs, live)], base)
    descs, first, stops = _index_arena(ctx, arena, offs, [arrs[k].size for k in live], starts)
    for j, k in enumerate(live):
        a, si = arrs[k], infos[j]
        d, stop, end = descs[int(first[j]):int(first[j + 1])], int(stops[j]), offs[j] + a.size
        if stop < end:
            if short is not None:
                short.append((k, stop - offs[j]))
            st, msg, h = parse_frame_header(a[stop - offs[j]:], True)
            if st != OK:
                entries[k] = ClaxonError(st, msg)
                continue
            tail = np.zeros(1, dtype=FRAME_DESC_DTYPE)
            tail[0] = (stop, min(end - stop, 0xffffffff), h.header_bytes, h.block_size, h.n_channels, h.channel_assignment, h.bps, (0,) * 5)
            d = np.concatenate([d, tail])
        if d.size and np.any(d["bps"] == 0):
            entries[k] = ClaxonError(UNSUPPORTED, 0, "a frame header without bits per sample")
            continue
        entries[k] = (d, int(si.sample_rate), int(d["n_channels"][0]) if d.size else int(si.channels), si)
    return arena, base, entries


def _decode_f32(ctx, arena, arena_len, descs, out_offs, out):
    """One plan (OUT_F32 | VERIFY_CRC16), one run of `arena` (a padded uint8 tensor on the GPU) into the float tensor `out`."""
    import torch
    batch = ctx.plan(descs, out_offs, verify_crc=True, path=OUT_F32)
    try:
        torch.cuda.current_stream(out.device).synchronize()        # (the uploads and the zero fill go first)
        batch.run(arena.data_ptr(), int(arena_len), out.data_ptr())
        return batch.results()
    finally:
        batch.close()


def _raise_first_failure(res, where=""):
    bad = np.nonzero(np.asarray(res["status"]) != OK)[0]
    if bad.size:
        r = res[int(bad[0])]
        e = ClaxonError(int(r["status"]), int(r["msg"]))
        if where:
            e.args = (e.args[0] + where,)
        raise e


def _arena_on_device(ctx, pieces, total):
    """The byte strings `pieces` [(offset, uint8 array)] in one arena on the context's GPU, padded as the decoder reads it."""
    import torch
    host = np.zeros(((total + 15) // 16) * 16 + 32, dtype=np.uint8)
    for o, a in pieces:
        host[o:o + a.size] = a
    return torch.from_numpy(host).to("cuda:%d" % ctx.device)


def _stream_problem(si, n_samples, digest):
    """What STREAMINFO says is wrong with a stream that decoded to `n_samples` samples per channel with MD5 `digest` (None: not
    computed): (text, md5 checked) -- text None when nothing is."""
    if int(si.samples) and int(si.samples) != n_samples:
        return "length mismatch: decoded %d samples per channel, STREAMINFO says %d" % (n_samples, int(si.samples)), False
    if digest is None:
        return None, False
    return (None if bytes(digest) == bytes(si.md5sum) else "MD5 signature mismatch"), True


_EMPTY_MD5 = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")     # (the MD5 of no samples: nothing to hash on the device)


def _md5_set(si):
    return any(bytes(si.md5sum))


def load(ctx, data, verify_md5=False):
    """A whole FLAC stream to (float32 tensor [T, C] on the context's GPU, sample rate): the header, one upload, the frames indexed on the
    device from that upload (Context.index_streams), one plan with OUT_F32 | VERIFY_CRC16 and one run.  A stream of 4 GiB or more is
    refused by the indexer (ClaxonError(API_ERROR)).  Samples are normalized as torchaudio / libsndfile do: v * 2^-(bps-1), in
    [-1, 1).  Raises ClaxonError with the first failing frame's status and message (the reference's reader stops there too).
    verify_md5: also check the stream against STREAMINFO, as `flac -t` does -- its sample count when it is set, then its MD5 when
    that is set (not all zero), computed on the device from the float output; a mismatch raises ClaxonError(FORMAT_ERROR).  The MD5
    of ONE stream runs on one GPU lane, far slower than a host core (README); verify() checks many streams at once."""
    import torch
    a = _u8(data)
    arena, arena_len, entries = _index_streams(ctx, [a])
    if isinstance(entries[0], ClaxonError):
        raise entries[0]
    descs, rate, ch, si = entries[0]
    bs = descs["block_size"].astype(np.uint64) * descs["n_channels"].astype(np.uint64)
    out_offs = np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64) if descs.size else np.zeros(0, dtype=np.uint64)
    if descs.size and np.any(descs["n_channels"] != ch):
        raise ClaxonError(FORMAT_ERROR, 0, "the stream's frames differ in their channel count")
    total = int(bs.sum())
    out = torch.zeros(total, dtype=torch.float32, device="cuda:%d" % ctx.device)
    if descs.size:
        res = _decode_f32(ctx, arena, arena_len, descs, out_offs, out)
        _raise_first_failure(res)
    if verify_md5:
        n = total // max(ch, 1)
        digest = None
        if _md5_set(si) and not (int(si.samples) and int(si.samples) != n):
            digest = ctx.md5_streams(out, SAMPLE_F32, [0], [total], [int(si.bits_per_sample)])[0] if total else _EMPTY_MD5
        why, _ = _stream_problem(si, n, digest)
        if why:
            raise ClaxonError(FORMAT_ERROR, 0, why)
    return out.view(total // max(ch, 1), ch), rate


def _decode_streams(ctx, arena, arena_len, all_descs, starts, out_len):
    """The streams of `arena` (_index_streams; their frames `all_descs`) decoded with one plan and one run into a zeroed float tensor of
    `out_len` samples, stream k's interleaved samples from index starts[k] on.  Returns (tensor, per-frame results or None, index of
    each stream's first frame)."""
    import torch
    offs = []
    for d, start in zip(all_descs, starts):
        bs = d["block_size"].astype(np.uint64) * d["n_channels"].astype(np.uint64)
        offs.append(np.uint64(start) + np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64) if d.size else np.zeros(0, np.uint64))
    out = torch.zeros(out_len, dtype=torch.float32, device="cuda:%d" % ctx.device)
    first = np.cumsum([0] + [d.size for d in all_descs])
    descs = np.concatenate(all_descs) if all_descs else np.zeros(0, dtype=FRAME_DESC_DTYPE)
    if not descs.size:
        return out, None, first
    return out, _decode_f32(ctx, arena, arena_len, descs, np.concatenate(offs).astype(np.uint64), out), first


def load_batch(ctx, streams, verify_md5=False):
    """Several whole FLAC streams to (float32 tensor [N, T_max, C] on the context's GPU, zero-padded; lengths int64 [N]; sample rates)
    with one upload, one Context.index_streams call (one per 4 GiB of streams) and one plan and one run: the streams sit in one arena at
    16-byte aligned places, every frame reads no further than its own stream's end.  T_max is rounded up to a multiple of 8 so that every block starts on 32 bytes (the float tiers' alignment).
    Raises ValueError when the streams differ in their channel count, ClaxonError on the first failing frame.  verify_md5: then
    checks every stream against its STREAMINFO as load(verify_md5=True) does, all MD5s in one call; ClaxonError names the first
    stream that fails."""
    import torch
    arrs = [_u8(s) for s in streams]
    arena, arena_len, idx = _index_streams(ctx, arrs)
    for e in idx:
        if isinstance(e, ClaxonError):
            raise e
    chans = {c for _, _, c, _ in idx}
    if len(chans) > 1:
        raise ValueError("load_batch: the streams differ in their channel count (%s)" % sorted(chans))
    ch = chans.pop() if chans else 1
    lengths = [int(d["block_size"].astype(np.int64).sum()) for d, _, _, _ in idx]
    t_max = ((max(lengths, default=0) + 7) // 8) * 8
    for k, (d, _, _, _) in enumerate(idx):
        if d.size and np.any(d["n_channels"] != ch):
            raise ClaxonError(FORMAT_ERROR, 0, "stream %d: its frames differ in their channel count" % k)
    out, res, first = _decode_streams(ctx, arena, arena_len, [d for d, _, _, _ in idx], [k * t_max * ch for k in range(len(arrs))],
                                      len(arrs) * t_max * ch)
    if res is not None:
        bad = np.nonzero(np.asarray(res["status"]) != OK)[0]
        if bad.size:
            k = int(np.searchsorted(first, int(bad[0]), side="right")) - 1
            _raise_first_failure(res, " (stream %d)" % k)
    if verify_md5:
        sis = [si for _, _, _, si in idx]
        todo = [k for k, si in enumerate(sis) if _md5_set(si) and not (int(si.samples) and int(si.samples) != lengths[k])] if out.numel() else []
        digests = dict(zip(todo, ctx.md5_streams(out, SAMPLE_F32, [k * t_max * ch for k in todo], [lengths[k] * ch for k in todo],
                                                 [int(sis[k].bits_per_sample) for k in todo]))) if todo else {}
        for k, si in enumerate(sis):
            why, _ = _stream_problem(si, lengths[k], digests.get(k, _EMPTY_MD5 if _md5_set(si) and not lengths[k] else None))
            if why:
                raise ClaxonError(FORMAT_ERROR, 0, "%s (stream %d)" % (why, k))
    return out.view(len(arrs), t_max, ch), torch.tensor(lengths, dtype=torch.int64), [r for _, r, _, _ in idx]


class Verdict:
    """verify()'s word on one stream: ok; md5_checked (the MD5 was set and compared); status and message of the first problem (OK and
    "" when there is none); samples: samples per channel decoded (0 when the stream did not get that far)."""
    __slots__ = ("ok", "md5_checked", "status", "message", "samples")

    def __init__(self, ok, md5_checked, status, message, samples):
        self.ok, self.md5_checked, self.status, self.message, self.samples = ok, md5_checked, status, message, samples

    def __repr__(self):
        return "Verdict(ok=%r, md5_checked=%r, status=%d, message=%r, samples=%d)" % (self.ok, self.md5_checked, self.status, self.message,
                                                                                     self.samples)


def verify(ctx, streams):
    """The `flac -t` of this library, for a corpus: a Verdict per stream (bytes-like FLAC streams), never raising for a bad stream.  All
    streams decode with one plan and one run (OUT_F32 | VERIFY_CRC16); each sits contiguously in one flat float buffer at a multiple of
    8 floats, so the streams may differ in channel count and bit depth.  Then every stream whose STREAMINFO has an MD5 is hashed on the
    device, all in one clx_md5_streams call.  A verdict names the first problem: a header or frame-index error, the first failing
    frame's status and message, a sample count other than STREAMINFO's, or "MD5 signature mismatch".
    The decoded audio of the whole call stays on the device, 4 bytes per sample, until the call returns: pass a corpus in chunks."""
    verdicts = [None] * len(streams)
    entries, all_descs, starts, at = [], [], [], 0     # entries: (k, STREAMINFO, samples per channel, samples)
    arena, arena_len, idx = _index_streams(ctx, [_u8(s) for s in streams])
    for k, e in enumerate(idx):
        if isinstance(e, ClaxonError):
            verdicts[k] = Verdict(False, False, e.status, e.message, 0)
            continue
        d, _, ch, si = e
        total = int((d["block_size"].astype(np.int64) * d["n_channels"].astype(np.int64)).sum())
        entries.append((k, si, total // max(ch, 1), total))
        all_descs.append(d)
        starts.append(at)
        at += ((total + 7) // 8) * 8
    out, res, first = _decode_streams(ctx, arena, arena_len, all_descs, starts, max(at, 1))
    todo = []
    for (k, si, n, total), at, f0, f1 in zip(entries, starts, first[:-1], first[1:]):
        bad = np.nonzero(np.asarray(res["status"][f0:f1]) != OK)[0] if f1 > f0 else []
        if len(bad):
            r = res[f0 + int(bad[0])]
            verdicts[k] = Verdict(False, False, int(r["status"]), message(int(r["msg"])), n)
        else:
            why, _ = _stream_problem(si, n, None)
            if why:
                verdicts[k] = Verdict(False, False, FORMAT_ERROR, why, n)
            elif not _md5_set(si):
                verdicts[k] = Verdict(True, False, OK, "", n)
            elif not 1 <= int(si.bits_per_sample) <= 24:
                verdicts[k] = Verdict(False, False, UNSUPPORTED, "the MD5 of more than 24 bits per sample is not checked", n)
            else:
                todo.append((k, si, n, total, at))
    if todo:
        digests = ctx.md5_streams(out, SAMPLE_F32, [at for _, _, _, _, at in todo], [total for _, _, _, total, _ in todo],
                                  [int(si.bits_per_sample) for _, si, _, _, _ in todo])
        for (k, si, n, _, _), dg in zip(todo, digests):
            why, _ = _stream_problem(si, n, dg)
            verdicts[k] = Verdict(why is None, True, OK if why is None else FORMAT_ERROR, why or "", n)
    return verdicts


# ---- mel features ---------------------------------------------------------------------------------------------------------------------

_MEL_MODES = {"power": MEL_POWER, "ln": MEL_LN, "log10": MEL_LOG10}
_MEL_PADS = {"reflect": MEL_PAD_REFLECT, "zeros": MEL_PAD_ZERO}


class _MelOpts(C.Structure):             # clx_mel_opts
    _fields_ = [("center", C.c_uint32), ("pad", C.c_uint32), ("range", C.c_uint32), ("range_width", C.c_float), ("shift", C.c_float),
                ("scale", C.c_float)]


class _MelFrameOpts(C.Structure):        # clx_mel_frame_opts
    _fields_ = [("remove_dc", C.c_uint32), ("whole_frames", C.c_uint32), ("preemph", C.c_float)]


class _MelCepOpts(C.Structure):          # clx_mel_cep_opts
    _fields_ = [("n_ceps", C.c_uint32), ("dct", C.c_void_p), ("lifter", C.c_void_p), ("energy", C.c_uint32), ("energy_scale", C.c_float),
                ("energy_floor", C.c_float)]


def _hz_to_mel(f, scale):
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    lin = f / (200.0 / 3.0)                                  # Slaney: linear below 1 kHz, logarithmic above (27 steps to 6.4 kHz)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (math.log(6.4) / 27.0), lin)


def _mel_to_hz(m, scale):
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp((math.log(6.4) / 27.0) * (np.maximum(m, 15.0) - 15.0)), m * (200.0 / 3.0))


def mel_window(n_fft):
    """The periodic Hann window of n_fft points: 0.5 - 0.5 cos(2 pi n / n_fft) in double, rounded once to float32."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(n_fft), dtype=np.float64) / int(n_fft))).astype(np.float32)


def mel_fbank(sample_rate, n_fft, n_mels, f_min=0.0, f_max=None, mel_scale="htk", norm=None):
    """The triangular filterbank [n_mels, n_fft // 2 + 1] (float32, built in double and rounded once): n_mels + 2 points evenly
    spaced on the mel scale from f_min to f_max (default sample_rate / 2), band m rising from point m to point m + 1 and falling to
    point m + 2, sampled at the bins' frequencies j * sample_rate / n_fft; norm="slaney" scales band m by 2 / (f[m + 2] - f[m]).
    ValueError for a band without a single non-zero bin (too many bands for n_fft), naming it."""
    if mel_scale not in ("htk", "slaney"):
        raise ValueError("mel_fbank: mel_scale must be 'htk' or 'slaney', not %r" % (mel_scale,))
    if norm not in (None, "slaney"):
        raise ValueError("mel_fbank: norm must be None or 'slaney', not %r" % (norm,))
    sample_rate, n_fft, n_mels = float(sample_rate), int(n_fft), int(n_mels)
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    f_min = float(f_min)
    if not (sample_rate > 0 and 0.0 <= f_min < f_max <= sample_rate / 2.0):
        raise ValueError("mel_fbank: need sample_rate > 0 and 0 <= f_min < f_max <= sample_rate / 2")
    if n_fft < 2 or n_mels < 1:
        raise ValueError("mel_fbank: need n_fft >= 2 and n_mels >= 1")
    J = n_fft // 2 + 1
    freqs = np.arange(J, dtype=np.float64) * (sample_rate / n_fft)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(f_min, mel_scale), _hz_to_mel(f_max, mel_scale), n_mels + 2), mel_scale)
    diff = pts[1:] - pts[:-1]
    slopes = pts[:, None] - freqs[None, :]                   # [n_mels + 2, J]
    down = -slopes[:-2] / diff[:-1, None]
    up = slopes[2:] / diff[1:, None]
    fb = np.maximum(0.0, np.minimum(down, up)) + 0.0         # (+ 0.0: no -0.0 in the table)
    if norm == "slaney":
        fb = fb * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    fb = np.ascontiguousarray(fb.astype(np.float32))
    empty = np.nonzero(~np.any(fb != 0, axis=1))[0]
    if empty.size:
        raise ValueError("mel_fbank: band %d (%.1f .. %.1f Hz) has no bin of the %d-point transform at %g Hz"
                         % (int(empty[0]), pts[empty[0]], pts[empty[0] + 2], n_fft, sample_rate))
    return fb


KALDI_WINDOWS = ("povey", "hanning", "hamming", "rectangular")
FLT_EPSILON = float(np.finfo(np.float32).eps)


def mel_window_kaldi(window_type, win_length, scale=1.0):
    """Kaldi's symmetric frame window of win_length points times `scale`, in double, rounded once to float32: "povey"
    (0.5 - 0.5 cos(2 pi n / (win_length - 1))) ^ 0.85, "hanning" (the same without the power), "hamming" 0.54 - 0.46 cos(..) or
    "rectangular"."""
    if window_type not in KALDI_WINDOWS:
        raise ValueError("mel_window_kaldi: window_type must be one of %s, not %r" % (", ".join(KALDI_WINDOWS), window_type))
    Nw = int(win_length)
    if Nw < 1 or (Nw < 2 and window_type != "rectangular"):
        raise ValueError("mel_window_kaldi: a %s window needs at least %d points" % (window_type, 1 if window_type == "rectangular" else 2))
    cosine = np.cos(2.0 * np.pi * np.arange(Nw, dtype=np.float64) / max(Nw - 1, 1))
    w = {"povey": lambda: (0.5 - 0.5 * cosine) ** 0.85, "hanning": lambda: 0.5 - 0.5 * cosine, "hamming": lambda: 0.54 - 0.46 * cosine,
         "rectangular": lambda: np.ones(Nw, dtype=np.float64)}[window_type]()
    return (w * float(scale)).astype(np.float32)


def mel_fbank_kaldi(sample_rate, n_fft, n_mels, low_freq=20.0, high_freq=0.0):
    """Kaldi's mel filterbank [n_mels, n_fft // 2] (float32, built in double and rounded once; the Nyquist bin is not used).  With
    mel(f) = 1127 ln(1 + f / 700), a high_freq <= 0 added to the Nyquist frequency and delta = (mel(high) - mel(low)) / (n_mels + 1),
    band b has left = mel(low) + b delta, centre = left + delta and right = centre + delta: the triangles are linear in mel, not in
    Hz.  Bin i lies at m = mel(i sample_rate / n_fft) and weighs (m - left) / (centre - left) for left < m <= centre,
    (right - m) / (right - centre) for centre < m < right, else 0.  A band without a bin is allowed (with many bands the lowest are
    empty, in Kaldi too)."""
    sample_rate, n_fft, n_mels = float(sample_rate), int(n_fft), int(n_mels)
    nyquist = 0.5 * sample_rate
    low, high = float(low_freq), float(high_freq)
    if high <= 0.0:
        high += nyquist
    if n_fft < 2 or n_mels < 1:
        raise ValueError("mel_fbank_kaldi: need n_fft >= 2 and n_mels >= 1")
    if not (sample_rate > 0 and 0.0 <= low < high <= nyquist):
        raise ValueError("mel_fbank_kaldi: need sample_rate > 0 and 0 <= low_freq < high_freq <= sample_rate / 2 (a high_freq <= 0 counts from there)")
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    mel_lo, mel_hi = float(mel(low)), float(mel(high))
    delta = (mel_hi - mel_lo) / (n_mels + 1)
    left = (mel_lo + np.arange(n_mels, dtype=np.float64) * delta)[:, None]
    centre = left + delta
    right = centre + delta
    m = mel(np.arange(n_fft // 2, dtype=np.float64) * (sample_rate / n_fft))[None, :]
    up, down = (m - left) / (centre - left), (right - m) / (right - centre)
    fb = np.where((m > left) & (m <= centre), up, np.where((m > centre) & (m < right), down, 0.0))
    return np.ascontiguousarray(fb.astype(np.float32))


def mel_dct(n_ceps, n_mels):
    """Kaldi's ComputeDctMatrix [n_ceps, n_mels] (float32, built in double and rounded once): the first n_ceps rows of the
    orthonormal DCT-II -- row 0 is sqrt(1 / n_mels), row k is sqrt(2 / n_mels) cos(pi / n_mels (m + 0.5) k)."""
    n_ceps, n_mels = int(n_ceps), int(n_mels)
    if not 1 <= n_ceps <= n_mels:
        raise ValueError("mel_dct: need 1 <= n_ceps <= n_mels, not %d and %d" % (n_ceps, n_mels))
    k = np.arange(n_ceps, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    d = math.sqrt(2.0 / n_mels) * np.cos((math.pi / n_mels) * (m + 0.5) * k)
    d[0, :] = math.sqrt(1.0 / n_mels)
    return np.ascontiguousarray(d.astype(np.float32))


def mel_lifter_kaldi(n_ceps, Q=22.0):
    """Kaldi's cepstral lifter [n_ceps] (float32, built in double and rounded once): 1 + 0.5 Q sin(pi i / Q).  Q = 0: None, no
    lifter."""
    n_ceps, Q = int(n_ceps), float(Q)
    if n_ceps < 1 or not math.isfinite(Q) or Q < 0:
        raise ValueError("mel_lifter_kaldi: need n_ceps >= 1 and a finite Q >= 0, not %d and %r" % (n_ceps, Q))
    if Q == 0.0:
        return None
    return (1.0 + 0.5 * Q * np.sin(math.pi * np.arange(n_ceps, dtype=np.float64) / Q)).astype(np.float32)


class MelSpec:
    """A feature spec for Context.mel_windows and StreamSet.read_mel (clx_mel_create, claxon_hip.h): frames of n_fft samples every
    `hop`, the periodic Hann window (.window), a triangular mel filterbank (.fbank, [n_mels, n_fft // 2 + 1]: mel_fbank) and the last
    step -- mode "power" (the band sums), "ln" or "log10" (the logarithm of max(band sum, floor)).  Both tables are built with
    numpy in double and rounded once to float32.  The spec owns the library's handle (the DFT basis is built and uploaded here,
    once) until close().  ctx=None builds the tables only.  ValueError for arguments out of range and for a filterbank with an empty
    band.

    center=True frames as torch.stft(center=True) does: frame t is centred on sample t * hop of the window continued by n_fft // 2
    samples on both sides, by reflection about the window's own ends (pad_mode="reflect") or by zeros ("zeros").  top=D (log modes)
    turns range scaling on: every cell is clamped to the window's maximum minus D, then (y + shift) * scale; a frame past the
    window's valid samples then holds the scaled silence value and not zeros.  (clx_mel_create_ex, claxon_hip.h, has both in full.)
    Without them the spec is what it always was.

    MelSpec.framed() builds a spec from a window and a filterbank of the caller's, with a frame shorter than the transform, each
    frame's mean removed and pre-emphasised before the window, a bank over the first bins only and whole frames counted
    (clx_mel_create_framed); MelSpec.kaldi() is Kaldi's fbank that way.  With a DCT, MelSpec.framed() builds a cepstral spec
    (clx_mel_create_cepstral): n_ceps rows of cepstra, liftered, with the frame's log energy in row 0 if asked for; MelSpec.mfcc()
    is Kaldi's MFCC that way.  n_out is the rows of a spec's output: n_ceps of a cepstral spec, n_mels of any other.

    MelSpec.framed(..., reflect_edges=True) builds a reflected spec (clx_mel_create_reflected): Kaldi's snip_edges=false, where
    frame t is centred on sample t * hop + hop // 2 of the window's valid samples, which are continued on both sides by reflection
    with the edge sample repeated, and a window of V valid samples has (V + hop // 2) // hop frames.  MelSpec.kaldi_reflected() and
    MelSpec.mfcc_reflected() are Kaldi's fbank and MFCC that way; reflect_edges is an attribute of every spec."""

    reflect_edges = False
    n_ceps, dct, lifter, energy, energy_scale, energy_floor = None, None, None, False, 1.0, 0.0    # (not cepstral unless framed() says so)

    @property
    def n_out(self):
        return self.n_mels if self.n_ceps is None else self.n_ceps

    def __init__(self, ctx, sample_rate, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=None, mel_scale="htk", norm=None, mode="ln",
                 floor=1e-10, center=False, pad_mode="reflect", top=None, shift=0.0, scale=1.0):
        self.ctx, self._h = ctx, None
        for name, v in (("sample_rate", sample_rate), ("n_fft", n_fft), ("hop", hop), ("n_mels", n_mels)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v:
                raise ValueError("MelSpec: %s must be a whole number, not %r" % (name, v))
        if mode not in _MEL_MODES:
            raise ValueError("MelSpec: mode must be 'ln', 'log10' or 'power', not %r" % (mode,))
        self.sample_rate, self.n_fft, self.hop, self.n_mels = int(sample_rate), int(n_fft), int(hop), int(n_mels)
        if not 2 <= self.n_fft <= 2048 or not 1 <= self.hop < 1 << 32 or not 1 <= self.n_mels <= 256 or self.sample_rate < 1:
            raise ValueError("MelSpec: need n_fft in 2..2048, hop >= 1, n_mels in 1..256 and sample_rate >= 1")
        self.mode, self.floor = mode, float(np.float32(floor))
        if mode != "power" and not self.floor > 0:
            raise ValueError("MelSpec: floor must be greater than 0 in mode %r" % mode)
        if not isinstance(center, (bool, np.bool_)):
            raise ValueError("MelSpec: center must be True or False, not %r" % (center,))
        if pad_mode not in _MEL_PADS:
            raise ValueError("MelSpec: pad_mode must be 'reflect' or 'zeros', not %r" % (pad_mode,))
        self.center, self.pad_mode = bool(center), pad_mode
        self.top = None if top is None else float(np.float32(top))
        self.shift, self.scale = float(np.float32(shift)), float(np.float32(scale))
        if self.top is not None:
            if mode == "power":
                raise ValueError("MelSpec: top needs mode 'ln' or 'log10'")
            if not (math.isfinite(self.top) and self.top > 0):
                raise ValueError("MelSpec: top must be finite and greater than 0, not %r" % (top,))
            if not math.isfinite(self.shift):
                raise ValueError("MelSpec: shift must be finite, not %r" % (shift,))
            if not math.isfinite(self.scale) or self.scale == 0:
                raise ValueError("MelSpec: scale must be finite and not zero, not %r" % (scale,))
        self.win_length, self.n_bins, self.remove_dc, self.preemph, self.whole_frames = self.n_fft, self.n_fft // 2 + 1, False, 0.0, False
        self.window = mel_window(self.n_fft)
        self.fbank = mel_fbank(self.sample_rate, self.n_fft, self.n_mels, f_min, f_max, mel_scale, norm)
        if ctx is not None:
            h = C.c_void_p(None)
            if not self.center and self.top is None:
                ctx._check(lib().clx_mel_create(ctx._h, self.n_fft, self.hop, _np_ptr(self.window), _np_ptr(self.fbank), self.n_mels,
                                                _MEL_MODES[mode], self.floor, C.byref(h)))
            else:
                opts = _MelOpts(int(self.center), _MEL_PADS[pad_mode], int(self.top is not None), self.top or 0.0, self.shift, self.scale)
                ctx._check(lib().clx_mel_create_ex(ctx._h, self.n_fft, self.hop, _np_ptr(self.window), _np_ptr(self.fbank), self.n_mels,
                                                   _MEL_MODES[mode], self.floor, C.byref(opts), C.byref(h)))
            self._h = h

    @classmethod
    def whisper(cls, ctx, n_mels=80):
        """The spec of Whisper's log_mel_spectrogram: 16 kHz, n_fft 400, hop 160, Slaney mel scale with Slaney normalisation up to
        8 kHz, log10 with floor 1e-10, frames centred with reflection, every cell clamped to the window's maximum - 8.0, then
        (y + 4) / 4.  read_mel(ids, starts, 3000, MelSpec.whisper(ctx)) is the encoder's [B, 80, 3000] input for 30 s crops.  The
        filterbank is librosa's by formula (mel_fbank): within half a float32 ulp of WhisperFeatureExtractor's mel_filters for 80
        and 128 bands, cell by cell, and the features are held to that extractor's output (tests/golden/features);
        Whisper's own table file (mel_filters.npz) is not available to this project.  Whisper also drops the last of its 3001
        frames; ask for the frames you want."""
        return cls(ctx, 16000, n_fft=400, hop=160, n_mels=n_mels, f_min=0.0, f_max=8000.0, mel_scale="slaney", norm="slaney", mode="log10",
                   floor=1e-10, center=True, pad_mode="reflect", top=8.0, shift=4.0, scale=0.25)

    @classmethod
    def framed(cls, ctx, sample_rate, n_fft, win_length, hop, window, fbank, mode="ln", floor=1e-10, remove_dc=False, preemph=0.0,
               whole_frames=False, dct=None, lifter=None, energy=False, energy_scale=1.0, energy_floor=0.0, reflect_edges=False):
        """The general framed spec (clx_mel_create_framed, claxon_hip.h): frames of win_length <= n_fft samples every `hop`, each
        with its own mean removed (remove_dc) and pre-emphasised by `preemph` (0: none; the first tap refers to the frame's own first
        sample), then `window` [win_length] and an n_fft-point transform of which the first n_bins bins go through `fbank`
        [n_mels, n_bins], n_bins <= n_fft // 2 + 1; rows of the bank may be all zero.  whole_frames counts only frames that lie
        inside a window's valid samples.  The tables are taken as float32.  ctx=None keeps the tables only.

        With `dct` [n_ceps, n_mels] the spec is cepstral (clx_mel_create_cepstral): row i of the output is dct[i] . (the frame's
        n_mels cells), times lifter[i] if `lifter` [n_ceps] is given; with `energy` row 0 is instead the logarithm of
        energy_scale times the frame's energy -- taken after the mean's removal and before pre-emphasis and the window, floored at
        FLT_EPSILON -- and not less than ln(energy_floor) if that is greater than 0.  A cepstral spec has at most 128 bands and
        256 bins.  Without `dct` the other four must be left alone.

        reflect_edges=True makes it a reflected spec (clx_mel_create_reflected), fbank or cepstral: frame t's tap n is sample
        t * hop + hop // 2 - win_length // 2 + n of the window's `valid` samples continued on both sides by reflection with the edge
        sample repeated (as often as it takes), everything behind the frame as without it, and a window has
        min(n_frames, (valid + hop // 2) // hop) frames.  It cannot be combined with whole_frames=True."""
        for name, v in (("sample_rate", sample_rate), ("n_fft", n_fft), ("win_length", win_length), ("hop", hop)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v:
                raise ValueError("MelSpec.framed: %s must be a whole number, not %r" % (name, v))
        if mode not in _MEL_MODES:
            raise ValueError("MelSpec.framed: mode must be 'ln', 'log10' or 'power', not %r" % (mode,))
        self = cls.__new__(cls)
        self.ctx, self._h = ctx, None
        self.sample_rate, self.n_fft, self.win_length, self.hop = int(sample_rate), int(n_fft), int(win_length), int(hop)
        if not 2 <= self.n_fft <= 2048 or not 1 <= self.win_length <= self.n_fft or not 1 <= self.hop < 1 << 32 or self.sample_rate < 1:
            raise ValueError("MelSpec.framed: need n_fft in 2..2048, win_length in 1..n_fft, hop >= 1 and sample_rate >= 1")
        self.window = np.ascontiguousarray(window, dtype=np.float32)
        self.fbank = np.ascontiguousarray(fbank, dtype=np.float32)
        if self.window.shape != (self.win_length,):
            raise ValueError("MelSpec.framed: window must have win_length = %d points, not shape %r" % (self.win_length, self.window.shape))
        if self.fbank.ndim != 2 or not 1 <= self.fbank.shape[0] <= 256 or not 1 <= self.fbank.shape[1] <= self.n_fft // 2 + 1:
            raise ValueError("MelSpec.framed: fbank must be [n_mels in 1..256, n_bins in 1..n_fft // 2 + 1], not shape %r" % (self.fbank.shape,))
        self.n_mels, self.n_bins = int(self.fbank.shape[0]), int(self.fbank.shape[1])
        self.mode, self.floor = mode, float(np.float32(floor))
        if mode != "power" and not self.floor > 0:
            raise ValueError("MelSpec.framed: floor must be greater than 0 in mode %r" % mode)
        for name, v in (("remove_dc", remove_dc), ("whole_frames", whole_frames), ("reflect_edges", reflect_edges)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("MelSpec.framed: %s must be True or False, not %r" % (name, v))
        if reflect_edges and whole_frames:
            raise ValueError("MelSpec.framed: reflect_edges=True cannot be combined with whole_frames=True (a reflected spec counts (valid + hop // 2) // hop frames)")
        self.reflect_edges = bool(reflect_edges)
        self.remove_dc, self.whole_frames, self.preemph = bool(remove_dc), bool(whole_frames), float(np.float32(preemph))
        if not (math.isfinite(self.preemph) and 0.0 <= self.preemph <= 1.0):
            raise ValueError("MelSpec.framed: preemph must be finite and in 0..1, not %r" % (preemph,))
        self.center, self.pad_mode, self.top, self.shift, self.scale = False, "reflect", None, 0.0, 1.0
        if dct is None:
            if lifter is not None or energy is not False or energy_scale != 1.0 or energy_floor != 0.0:
                raise ValueError("MelSpec.framed: lifter, energy, energy_scale and energy_floor need a dct")
        else:
            self.dct = np.ascontiguousarray(dct, dtype=np.float32)
            if self.n_mels > 128 or self.n_bins > 256:
                raise ValueError("MelSpec.framed: a cepstral spec has at most 128 bands and 256 bins, not %d and %d" % (self.n_mels, self.n_bins))
            if self.dct.ndim != 2 or self.dct.shape[1] != self.n_mels or not 1 <= self.dct.shape[0] <= self.n_mels:
                raise ValueError("MelSpec.framed: dct must be [n_ceps in 1..n_mels, n_mels = %d], not shape %r" % (self.n_mels, self.dct.shape))
            self.n_ceps = int(self.dct.shape[0])
            self.lifter = None if lifter is None else np.ascontiguousarray(lifter, dtype=np.float32)
            if self.lifter is not None and self.lifter.shape != (self.n_ceps,):
                raise ValueError("MelSpec.framed: lifter must have n_ceps = %d entries, not shape %r" % (self.n_ceps, self.lifter.shape))
            if not isinstance(energy, (bool, np.bool_)):
                raise ValueError("MelSpec.framed: energy must be True or False, not %r" % (energy,))
            self.energy, self.energy_scale, self.energy_floor = bool(energy), float(np.float32(energy_scale)), float(np.float32(energy_floor))
            if not (math.isfinite(self.energy_scale) and self.energy_scale > 0):
                raise ValueError("MelSpec.framed: energy_scale must be finite and greater than 0, not %r" % (energy_scale,))
            if not (math.isfinite(self.energy_floor) and self.energy_floor >= 0):
                raise ValueError("MelSpec.framed: energy_floor must be finite and not negative, not %r" % (energy_floor,))
        if ctx is not None and self.reflect_edges:
            h = C.c_void_p(None)
            opts = _MelFrameOpts(int(self.remove_dc), 0, self.preemph)
            cep = None if self.n_ceps is None else _MelCepOpts(self.n_ceps, _np_ptr(self.dct), None if self.lifter is None else _np_ptr(self.lifter),
                                                               int(self.energy), self.energy_scale, self.energy_floor)
            ctx._check(lib().clx_mel_create_reflected(ctx._h, self.n_fft, self.win_length, self.hop, _np_ptr(self.window), _np_ptr(self.fbank),
                                                      self.n_bins, self.n_mels, _MEL_MODES[mode], self.floor, C.byref(opts),
                                                      None if cep is None else C.byref(cep), C.byref(h)))
            self._h = h
        elif ctx is not None and self.n_ceps is not None:
            h = C.c_void_p(None)
            opts = _MelFrameOpts(int(self.remove_dc), int(self.whole_frames), self.preemph)
            cep = _MelCepOpts(self.n_ceps, _np_ptr(self.dct), None if self.lifter is None else _np_ptr(self.lifter), int(self.energy),
                              self.energy_scale, self.energy_floor)
            ctx._check(lib().clx_mel_create_cepstral(ctx._h, self.n_fft, self.win_length, self.hop, _np_ptr(self.window), _np_ptr(self.fbank),
                                                     self.n_bins, self.n_mels, _MEL_MODES[mode], self.floor, C.byref(opts), C.byref(cep),
                                                     C.byref(h)))
            self._h = h
        elif ctx is not None:
            h = C.c_void_p(None)
            opts = _MelFrameOpts(int(self.remove_dc), int(self.whole_frames), self.preemph)
            ctx._check(lib().clx_mel_create_framed(ctx._h, self.n_fft, self.win_length, self.hop, _np_ptr(self.window), _np_ptr(self.fbank),
                                                   self.n_bins, self.n_mels, _MEL_MODES[mode], self.floor, C.byref(opts), C.byref(h)))
            self._h = h
        return self

    _KALDI_REFUSED = dict(dither=0.0, use_energy=False, snip_edges=True, vtln_warp=1.0, htk_compat=False)

    @classmethod
    def kaldi(cls, ctx, sample_rate=16000, n_mels=80, frame_length_ms=25.0, frame_shift_ms=10.0, low_freq=20.0, high_freq=0.0,
              preemphasis=0.97, remove_dc_offset=True, window_type="povey", scale=32768.0, _reflect=False, **refused):
        """Kaldi's fbank (torchaudio.compliance.kaldi.fbank, kaldi-native-fbank, lhotse's Fbank) with its defaults: frames of
        frame_length_ms every frame_shift_ms (400 and 160 samples at 16 kHz), the frame's mean removed, pre-emphasis 0.97, the povey
        window, a transform of the next power of two (512; at most 2048) of which the Nyquist bin is not used, n_mels triangles that
        are linear in mel from low_freq to the Nyquist frequency + high_freq (mel_fbank_kaldi), ln with floor FLT_EPSILON, and only
        whole frames counted (snip_edges).  Kaldi works on samples in the int16 range: the window is multiplied by `scale` (32768)
        in double before its one rounding, and as the conditioning is linear a power-of-two scale gives what Kaldi gives on the
        int16-range input bit for bit.  read_mel(ids, starts, n_frames, MelSpec.kaldi(ctx)) is [B, n_mels, n_frames] ("tc":
        Kaldi's own [n_frames, n_mels]).  dither, use_energy, snip_edges=False, vtln_warp and htk_compat are refused by name (the
        frame's energy is MelSpec.mfcc's use_energy; fbank's energy column is not provided).  The tables, the definition and the
        kernel's output are held to the float64 port of torchaudio's Kaldi code in transformers.audio_utils (tests/golden/features,
        DESIGN.md 4.14); two conventions differ from that port and follow Kaldi: preemphasis is rounded to float32, as Kaldi's
        BaseFloat is (the port keeps the double 0.97), and the transform is not rounded to complex64.  No Kaldi binary itself has
        been run, and windows read at another rate than the stream's (the resampled path) are not covered."""
        who, only = ("MelSpec.kaldi_reflected", dict(cls._KALDI_REFUSED, snip_edges=False)) if _reflect else ("MelSpec.kaldi", cls._KALDI_REFUSED)
        for name, v in refused.items():
            if name not in only:
                raise TypeError("%s: unknown argument %r" % (who, name))
            if isinstance(v, bool) != isinstance(only[name], bool) or v != only[name]:
                raise ValueError("%s: %s=%r is not supported (only %r)" % (who, name, v, only[name]))
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, float, np.integer, np.floating)) or int(sample_rate) != sample_rate or sample_rate < 1:
            raise ValueError("MelSpec.kaldi: sample_rate must be a whole number from 1 up, not %r" % (sample_rate,))
        win_length, hop = int(sample_rate * 0.001 * float(frame_length_ms)), int(sample_rate * 0.001 * float(frame_shift_ms))
        if not 2 <= win_length <= 2048 or hop < 1:
            raise ValueError("MelSpec.kaldi: the frame must be 2..2048 samples and the shift at least 1, not %d and %d" % (win_length, hop))
        n_fft = 1 << (win_length - 1).bit_length()
        if not (math.isfinite(float(scale)) and float(scale) > 0):
            raise ValueError("MelSpec.kaldi: scale must be finite and greater than 0, not %r" % (scale,))
        if not isinstance(remove_dc_offset, (bool, np.bool_)):
            raise ValueError("MelSpec.kaldi: remove_dc_offset must be True or False, not %r" % (remove_dc_offset,))
        window = mel_window_kaldi(window_type, win_length, scale)
        fbank = mel_fbank_kaldi(sample_rate, n_fft, n_mels, low_freq, high_freq)
        return cls.framed(ctx, sample_rate, n_fft, win_length, hop, window, fbank, mode="ln", floor=FLT_EPSILON, remove_dc=bool(remove_dc_offset),
                          preemph=preemphasis, whole_frames=not _reflect, reflect_edges=bool(_reflect))

    @classmethod
    def kaldi_reflected(cls, ctx, *args, **kw):
        """Kaldi's fbank with --snip-edges=false (lhotse's and kaldifeat's default): MelSpec.kaldi's arguments, defaults and tables,
        word for word, on reflected frames.  Frame t is centred on sample t * hop + hop // 2: its tap n is sample
        t * hop + hop // 2 - win_length // 2 + n, and where that lies outside the window's valid samples [0, valid) it is reflected
        with the edge sample repeated (-1 is 0, valid is valid - 1), as often as it takes.  A window of `valid` samples has
        (valid + hop // 2) // hop frames, so the frame count follows the sample count and not the frame length.  The reflection is
        about the crop read_mel cuts, [start, start + valid), not about the stream: Kaldi's features of a whole utterance of T
        samples need start = 0, n_frames >= (T + hop // 2) // hop and length >= T -- read_mel's default length n_frames * hop can be
        shorter than T and would cut the utterance and reflect early.  dither, use_energy, vtln_warp and htk_compat are refused by
        name as for MelSpec.kaldi (snip_edges, if given, must be False).  The reflection and everything behind it are held to numpy's
        symmetric padding in front of the outside fbank of MelSpec.kaldi's comparison (tests/golden/features); the
        frame count and the origin hop // 2 - win_length // 2 are this project's reading of Kaldi's feature-window.cc and have not
        been checked against an outside implementation, and no Kaldi binary itself has been run."""
        if "_reflect" in kw:
            raise TypeError("MelSpec.kaldi_reflected: unknown argument '_reflect'")
        return cls.kaldi(ctx, *args, _reflect=True, **kw)

    _MFCC_REFUSED = dict(dither=0.0, snip_edges=True, vtln_warp=1.0, htk_compat=False, raw_energy=True)

    @classmethod
    def mfcc(cls, ctx, sample_rate=16000, n_ceps=13, n_mels=23, cepstral_lifter=22.0, use_energy=False, energy_floor=0.0, frame_length_ms=25.0,
             frame_shift_ms=10.0, low_freq=20.0, high_freq=0.0, preemphasis=0.97, remove_dc_offset=True, window_type="povey", scale=32768.0,
             _reflect=False, **refused):
        """Kaldi's MFCC (compute-mfcc-feats, torchaudio.compliance.kaldi.mfcc, lhotse's Mfcc) with torchaudio's defaults:
        MelSpec.kaldi's frames, conditioning, window and n_mels = 23 bands by its rules, then the first n_ceps = 13 rows of the
        orthonormal DCT-II of the log-mel cells (mel_dct) and the lifter 1 + 0.5 Q sin(pi i / Q) with Q = cepstral_lifter
        (mel_lifter_kaldi; 0: none).  use_energy puts the frame's log energy in row 0 in place of C0 (Kaldi's raw_energy: before
        pre-emphasis and the window), not less than ln(energy_floor) if that is greater than 0; the samples' int16-range scale enters
        the energy as scale ** 2.  read_mel(ids, starts, n_frames, MelSpec.mfcc(ctx)) is [B, n_ceps, n_frames] ("tc": Kaldi's own
        [n_frames, n_ceps]).  dither, snip_edges=False, vtln_warp, htk_compat and raw_energy=False are refused by name.  The
        cepstra are held to scipy.fft.dct (orthonormal DCT-II) of the outside fbank of MelSpec.kaldi's comparison
        (tests/golden/features); the lifter formula and the energy row are this project's own reading of Kaldi and
        have not been checked against an outside implementation, and no Kaldi binary itself has been run."""
        who, only = ("MelSpec.mfcc_reflected", dict(cls._MFCC_REFUSED, snip_edges=False)) if _reflect else ("MelSpec.mfcc", cls._MFCC_REFUSED)
        for name, v in refused.items():
            if name not in only:
                raise TypeError("%s: unknown argument %r" % (who, name))
            if isinstance(v, bool) != isinstance(only[name], bool) or v != only[name]:
                raise ValueError("%s: %s=%r is not supported (only %r)" % (who, name, v, only[name]))
        for name, v in (("n_ceps", n_ceps), ("n_mels", n_mels)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s: %s must be a whole number, not %r" % (who, name, v))
        if not 1 <= int(n_mels) <= 128 or not 1 <= int(n_ceps) <= int(n_mels):
            raise ValueError("%s: need n_mels in 1..128 and n_ceps in 1..n_mels, not %d and %d" % (who, n_mels, n_ceps))
        if not isinstance(use_energy, (bool, np.bool_)):
            raise ValueError("%s: use_energy must be True or False, not %r" % (who, use_energy,))
        base = cls.kaldi(None, sample_rate=sample_rate, n_mels=int(n_mels), frame_length_ms=frame_length_ms, frame_shift_ms=frame_shift_ms,
                         low_freq=low_freq, high_freq=high_freq, preemphasis=preemphasis, remove_dc_offset=remove_dc_offset,
                         window_type=window_type, scale=scale)
        return cls.framed(ctx, base.sample_rate, base.n_fft, base.win_length, base.hop, base.window, base.fbank, mode="ln", floor=FLT_EPSILON,
                          remove_dc=base.remove_dc, preemph=base.preemph, whole_frames=not _reflect, dct=mel_dct(n_ceps, n_mels),
                          lifter=mel_lifter_kaldi(n_ceps, cepstral_lifter), energy=bool(use_energy), energy_scale=float(scale) ** 2,
                          energy_floor=energy_floor, reflect_edges=bool(_reflect))

    @classmethod
    def mfcc_reflected(cls, ctx, *args, **kw):
        """Kaldi's MFCC with --snip-edges=false: MelSpec.mfcc's arguments, defaults and tables, word for word, on MelSpec.kaldi_reflected's
        frames (its docstring has the placement, the count, what the reflection is about and how to get a whole utterance's
        features from read_mel).  With use_energy the frame's log energy is taken over the reflected, mean-removed frame.  dither,
        vtln_warp, htk_compat and raw_energy=False are refused by name as for MelSpec.mfcc (snip_edges, if given, must be False).  What
        an outside implementation has and has not checked is as for MelSpec.kaldi_reflected and MelSpec.mfcc together."""
        if "_reflect" in kw:
            raise TypeError("MelSpec.mfcc_reflected: unknown argument '_reflect'")
        return cls.mfcc(ctx, *args, _reflect=True, **kw)

    def window_len(self, n_frames):
        """The samples that n_frames frames span: (n_frames - 1) * hop + n_fft (0 for no frame; win_length in place of n_fft for a
        framed spec); n_frames * hop for a centred spec (torch.stft gives 1 + L // hop frames on such a window; read_mel takes the
        first n_frames) and for a reflected spec (whose frame t is centred on sample t * hop + hop // 2)."""
        if int(n_frames) <= 0:
            return 0
        return int(n_frames) * self.hop if self.center or self.reflect_edges else (int(n_frames) - 1) * self.hop + self.win_length

    def valid_frames(self, valid, n_frames):
        """valid_frames of windows with `valid` samples inside their streams (int64 array): min(ceil(valid / hop), n_frames), and
        for a centred spec 0 where valid == 0, else min(ceil((valid + n_fft // 2) / hop), n_frames).  A spec that counts whole
        frames: 0 where valid < win_length, else min(1 + (valid - win_length) // hop, n_frames).  A reflected spec:
        min((valid + hop // 2) // hop, n_frames)."""
        v = np.asarray(valid, dtype=np.int64)
        if self.reflect_edges:
            return np.minimum((v + self.hop // 2) // self.hop, int(n_frames)).astype(np.int64)
        if self.whole_frames:
            return np.where(v < self.win_length, 0, np.minimum(1 + (v - self.win_length) // self.hop, int(n_frames))).astype(np.int64)
        P = self.n_fft // 2 if self.center else 0
        return np.where(v == 0, 0, np.minimum((v + P + self.hop - 1) // self.hop, int(n_frames))).astype(np.int64)

    def close(self):
        if self._h is not None and self.ctx is not None and self.ctx._h:
            lib().clx_mel_destroy(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- per-window normalisation -----------------------------------------------------------------------------------------------------

class _NormOpts(C.Structure):            # clx_norm_opts
    _fields_ = [("mean", C.c_uint32), ("var", C.c_uint32), ("ddof", C.c_uint32), ("eps", C.c_float), ("pad", C.c_float)]


class Norm:
    """What Context.norm_windows and read(..., normalize=) / read_mel(..., normalize=) do to every row of every window, over the
    row's valid cells (clx_norm_windows, claxon_hip.h): subtract the mean (`mean`), divide by sqrt(variance + eps) (`var`; the
    variance about the mean, over n - ddof), and set the padding to `pad`.  A plain value: it owns nothing on the device.
    ValueError for a mean, var or ddof that is not 0 / 1 (or a bool), for mean and var both off, for an eps that is negative or not
    finite and for a pad that is not finite."""

    def __init__(self, mean=True, var=True, ddof=0, eps=0.0, pad=0.0):
        for name, v in (("mean", mean), ("var", var), ("ddof", ddof)):
            if not isinstance(v, (bool, int, np.integer, np.bool_)) or int(v) not in (0, 1):
                raise ValueError("Norm: %s must be 0 or 1, not %r" % (name, v))
        if not mean and not var:
            raise ValueError("Norm: mean and var are both off: nothing to do")
        for name, v in (("eps", eps), ("pad", pad)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) \
                    or abs(float(v)) > float(np.finfo(np.float32).max):
                raise ValueError("Norm: %s must be a finite number, not %r" % (name, v))
        if float(eps) < 0:
            raise ValueError("Norm: eps must not be negative, not %r" % (eps,))
        self.mean, self.var, self.ddof = bool(mean), bool(var), int(ddof)
        self.eps, self.pad = float(np.float32(eps)), float(np.float32(pad))

    @classmethod
    def wav2vec2(cls):
        """Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm (wav2vec 2.0, HuBERT, WavLM): (x - mean) / sqrt(var + 1e-7), padding 0."""
        return cls(eps=1e-7)

    @classmethod
    def cmvn(cls, means=True, vars=True):
        """Speech2TextFeatureExtractor.utterance_cmvn: per band over the valid frames, the variance about the mean with ddof 0 and
        no epsilon, padding 0; normalize_means / normalize_vars as `means` / `vars`."""
        return cls(mean=means, var=vars)

    @classmethod
    def seamless(cls):
        """SeamlessM4TFeatureExtractor's per-band step: (x - mean) / sqrt(var(ddof=1) + 1e-7)."""
        return cls(ddof=1, eps=1e-7)

    def _opts(self):
        return _NormOpts(int(self.mean), int(self.var), self.ddof, self.eps, self.pad)

    def __repr__(self):
        return "Norm(mean=%r, var=%r, ddof=%d, eps=%r, pad=%r)" % (self.mean, self.var, self.ddof, self.eps, self.pad)

    def __eq__(self, other):
        return isinstance(other, Norm) and (self.mean, self.var, self.ddof, self.eps, self.pad) == (other.mean, other.var, other.ddof, other.eps, other.pad)

    def __hash__(self):
        return hash((self.mean, self.var, self.ddof, self.eps, self.pad))


# ---- frame splicing: deltas, context, subsampling, low frame rate ------------------------------------------------------------------

SPLICE_MAX_BLOCKS, SPLICE_MAX_STRIDE, SPLICE_MAX_OFFSET, SPLICE_MAX_HALF, SPLICE_MAX_OUT_ROWS = 32, 64, 64, 16, 8192


class _SpliceOpts(C.Structure):          # clx_splice_opts
    _fields_ = [("n_blocks", C.c_uint32), ("stride", C.c_uint32), ("pad", C.c_float), ("reserved", C.c_uint32)]


def _splice_whole(v, lo, hi, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("Splice: %s must be a whole number in %d..%d, not %r" % (what, lo, hi, v))
    return int(v)


class Splice:
    """What Context.splice_windows and read_mel(..., splice=) do along time to every row of every window (clx_splice_windows,
    claxon_hip.h): `blocks` is a list of (offset, coefs): coefs None is a copy block, output frame u of it is input frame
    u * stride + offset; otherwise an odd number 2m + 1 <= 33 of finite coefficients c[-m .. m], and the frame is the sum over d
    of c[d] times input frame u * stride + offset + d, added up by fused multiply-adds in ascending d.  Every frame index is
    clamped into the window's valid frames, so the first and the last frame repeat.  The K <= 32 blocks stand one behind the other
    in the output's rows: n_out(rows) = K * rows (8192 at most); an input of n frames gives frames_out(n) = ceil(n / stride);
    output frames behind a window's own are `pad`.  A plain value: it owns nothing on the device.  deltas(), context(),
    subsample() and lfr() build the plans of Kaldi's add-deltas, splice-feats and subsample-feats and of FunASR's apply_lfr, as this
    project reads them.  ValueError for what the ranges above exclude."""

    def __init__(self, blocks, stride=1, pad=0.0):
        self.stride = _splice_whole(stride, 1, SPLICE_MAX_STRIDE, "stride")
        if isinstance(pad, bool) or not isinstance(pad, (int, float, np.integer, np.floating)) or not math.isfinite(float(pad)) \
                or abs(float(pad)) > float(np.finfo(np.float32).max):
            raise ValueError("Splice: pad must be a finite number, not %r" % (pad,))
        self.pad = float(np.float32(pad))
        try:
            blocks = [tuple(b) for b in blocks]
        except TypeError:
            blocks = None
        if not blocks or len(blocks) > SPLICE_MAX_BLOCKS or any(len(b) != 2 for b in blocks):
            raise ValueError("Splice: blocks must be a list of 1..%d (offset, coefs or None) pairs" % SPLICE_MAX_BLOCKS)
        out = []
        for off, coefs in blocks:
            off = _splice_whole(off, -SPLICE_MAX_OFFSET, SPLICE_MAX_OFFSET, "an offset")
            if coefs is not None:
                c = np.asarray(coefs)
                if c.ndim != 1 or c.size % 2 != 1 or c.size > 2 * SPLICE_MAX_HALF + 1 or c.dtype.kind not in "fiu":
                    raise ValueError("Splice: a block's coefs must be None or an odd number, at most %d, of numbers" % (2 * SPLICE_MAX_HALF + 1))
                with np.errstate(over="ignore"):
                    c = c.astype(np.float64).astype(np.float32)              # (one rounding of what the caller gave)
                if not np.all(np.isfinite(c)):
                    raise ValueError("Splice: a block's coefs must be finite float32 values")
                coefs = tuple(float(v) for v in c)
            out.append((off, coefs))
        self.blocks = tuple(out)

    @classmethod
    def deltas(cls, order=2, window=2, pad=0.0):
        """Kaldi's add-deltas (DeltaFeatures): the features, then their order-i deltas for i = 1 .. order, each the i-fold
        convolution of [-window .. window] / (2 * sum d^2) with itself over the edge-repeated frames -- one combined filter of
        2 * i * window + 1 taps, clamped once; applying the first-order filter i times is not the same in the edge frames.
        order 0..4 and order * window at most 16.  The coefficients come from clx_splice_deltas: exact whole numerators and
        denominators, divided in double, rounded once to float32."""
        order = _splice_whole(order, 0, 4, "order")
        window = _splice_whole(window, 1 if order else 0, SPLICE_MAX_HALF // order if order else 1 << 30, "window (order * window at most 16)")
        blk = np.zeros((order + 1, 4), dtype=np.int32)
        coefs = np.zeros(max(1, order * (order * window + window + 1)), dtype=np.float32)
        n = C.c_uint32(0)
        if lib().clx_splice_deltas(order, window, _np_ptr(blk), _np_ptr(coefs), C.byref(n)) != OK:
            raise ValueError("Splice.deltas: order %r and window %r are refused" % (order, window))
        return cls([(0, None)] + [(0, coefs[int(b[3]):int(b[3]) + 2 * int(b[1]) + 1]) for b in blk[1:]], 1, pad)

    @classmethod
    def context(cls, left, right, pad=0.0):
        """Kaldi's splice-feats: left + right + 1 copy blocks, the frames at offsets -left .. right."""
        left, right = _splice_whole(left, 0, SPLICE_MAX_OFFSET, "left"), _splice_whole(right, 0, SPLICE_MAX_OFFSET, "right")
        if left + right + 1 > SPLICE_MAX_BLOCKS:
            raise ValueError("Splice: left + right + 1 must be at most %d blocks, not %d" % (SPLICE_MAX_BLOCKS, left + right + 1))
        return cls([(o, None) for o in range(-left, right + 1)], 1, pad)

    @classmethod
    def subsample(cls, n, pad=0.0):
        """Kaldi's subsample-feats: every n-th frame, from frame 0."""
        return cls([(0, None)], _splice_whole(n, 1, SPLICE_MAX_STRIDE, "n"), pad)

    @classmethod
    def lfr(cls, m=7, n=6, pad=0.0):
        """FunASR's apply_lfr (Paraformer, SenseVoice): m frames stacked at a stride of n, the first frame repeated (m - 1) // 2 times
        in front and the last frame repeated behind: m copy blocks at offsets -((m - 1) // 2) .. m - 1 - (m - 1) // 2."""
        m, n = _splice_whole(m, 1, SPLICE_MAX_BLOCKS, "m"), _splice_whole(n, 1, SPLICE_MAX_STRIDE, "n")
        return cls([(o - (m - 1) // 2, None) for o in range(m)], n, pad)

    def n_out(self, rows):
        """Output rows for `rows` input rows."""
        return len(self.blocks) * int(rows)

    def frames_out(self, n):
        """Output frames for n input frames (a number or an array of them): ceil(n / stride)."""
        if isinstance(n, np.ndarray):
            return (n + (self.stride - 1)) // self.stride
        return (int(n) + self.stride - 1) // self.stride

    def _tables(self):
        """(blocks [K, 4] int32: offset, m, copy, first coefficient; coefs float32) for clx_splice_windows."""
        blk = np.zeros((len(self.blocks), 4), dtype=np.int32)
        coefs = []
        for j, (off, c) in enumerate(self.blocks):
            blk[j] = (off, 0, 1, 0) if c is None else (off, len(c) // 2, 0, len(coefs))
            coefs.extend(c or ())
        return blk, np.array(coefs, dtype=np.float32)

    def __repr__(self):
        return "Splice(%r, stride=%d, pad=%r)" % ([(o, None if c is None else list(c)) for o, c in self.blocks], self.stride, self.pad)

    def __eq__(self, other):
        return isinstance(other, Splice) and (self.blocks, self.stride, self.pad) == (other.blocks, other.stride, other.pad)

    def __hash__(self):
        return hash((self.blocks, self.stride, self.pad))


# ---- global and sliding-window CMVN --------------------------------------------------------------------------------------------

CMVN_MAX_ROWS, CMVN_MAX_WINDOW = 8192, 1024


class _CmvnGlobalOpts(C.Structure):      # clx_cmvn_global_opts
    _fields_ = [("pad", C.c_float), ("reserved", C.c_uint32)]


class _CmvnSlidingOpts(C.Structure):     # clx_cmvn_sliding_opts
    _fields_ = [("window", C.c_uint32), ("min_window", C.c_uint32), ("center", C.c_uint32), ("norm_vars", C.c_uint32), ("pad", C.c_float),
                ("reserved", C.c_uint32)]


def _cmvn_pad(pad):
    if isinstance(pad, bool) or not isinstance(pad, (int, float, np.integer, np.floating)) or not math.isfinite(float(pad)) \
            or abs(float(pad)) > float(np.finfo(np.float32).max):
        raise ValueError("Cmvn: pad must be a finite number, not %r" % (pad,))
    return float(np.float32(pad))


def _cmvn_row(v, what, n=None):
    """`v` as a float64 vector of 1..8192 finite numbers (n: of exactly n)."""
    try:
        a = np.asarray(v)
    except Exception:
        a = None
    if a is None or a.ndim != 1 or a.dtype.kind not in "fiu" or not 1 <= a.size <= CMVN_MAX_ROWS or (n is not None and a.size != n):
        raise ValueError("Cmvn: %s must be a vector of %s numbers" % (what, "1..%d" % CMVN_MAX_ROWS if n is None else "%d" % n))
    a = a.astype(np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("Cmvn: %s must be finite" % what)
    return a


def _cmvn_f32(a, what):
    with np.errstate(over="ignore"):
        f = a.astype(np.float32)                             # (one rounding of what the caller gave)
    if not np.all(np.isfinite(f)):
        raise ValueError("Cmvn: %s must be finite float32 values" % what)
    return np.ascontiguousarray(f)


def _cmvn_whole(v, lo, hi, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("Cmvn: %s must be a whole number in %d..%d, not %r" % (what, lo, hi, v))
    return int(v)


def _cmvn_flag(v, what):
    if not isinstance(v, (bool, int, np.integer, np.bool_)) or int(v) not in (0, 1):
        raise ValueError("Cmvn: %s must be 0 or 1, not %r" % (what, v))
    return bool(v)


class Cmvn:
    """What Context.cmvn_windows and read_mel(..., cmvn=) do to every window: cepstral mean and variance normalisation whose
    statistics are not the window's own (that one is Norm).  A plain value: it owns nothing on the device.  Three kinds:

    global     a fixed float32 shift and scale per row: y = (x + shift[r]) * scale[r], two float32 operations, bit for bit what
               numpy or torch give for that expression (clx_cmvn_global_windows; in place).  global_(shift, scale),
               from_mean_std(mean, std) (WeNet's (x - mean) * istd: shift = -mean, scale = float32(1 / float64(std)); ESPnet's
               GlobalMVN divides by std instead, which is not bit-equal) and from_kaldi_stats(stats) (a Kaldi CMVN accumulator,
               [2][rows + 1]: clx_cmvn_from_stats) build one; FunASR's am.mvn is global_(means, vars).  .rows is the row count.
    sliding    the mean (and with norm_vars the standard deviation) of each row over a window of frames around (center) or up to
               (not center) the cell's own frame: Kaldi's apply-cmvn-sliding as this project reads it (clx_cmvn_sliding_windows; out
               of place).  sliding(window, min_window, center, norm_vars) builds one, xvector() is the x-vector recipes'
               sliding(300, 100, True, False).  .rows is None.
    grouped    a shift and scale per row and GROUP of windows (speaker), solved on the device from a CmvnStats accumulator each
               time it is applied: Kaldi's apply-cmvn --utt2spk (clx_cmvn_grouped_windows; in place).  grouped(stats) builds one;
               it holds a reference to the CmvnStats (the one kind that does not stand alone), .rows is the stats' rows, and
               cmvn_windows / read_mel take the windows' groups beside it.  With one group it gives the words of
               stats.cmvn() applied as a global one.

    Frames behind a window's valid ones become `pad`.  ValueError for a shift or scale that is not 1..8192 finite float32 numbers,
    for vectors of different lengths, a std that is not above 0, a stats matrix that is not [2][rows + 1] or whose count is not
    above 0, a window outside 1..1024, a min_window outside 1..window, a flag that is not 0 / 1 and a pad that is not finite."""

    def __init__(self, shift=None, scale=None, window=None, min_window=None, center=False, norm_vars=False, pad=0.0):
        self.pad = _cmvn_pad(pad)
        self._stats = None
        if (shift is None) != (scale is None) or (shift is None) == (window is None):
            raise ValueError("Cmvn: give shift and scale (a global one) or window (a sliding one); see global_() and sliding()")
        if shift is not None:
            self._shift = _cmvn_f32(_cmvn_row(shift, "shift"), "shift")
            self._scale = _cmvn_f32(_cmvn_row(scale, "scale", self._shift.size), "scale")
            self.rows = int(self._shift.size)
            self.window = self.min_window = None
            self.center = self.norm_vars = False
        else:
            self._shift = self._scale = None
            self.rows = None
            self.window = _cmvn_whole(window, 1, CMVN_MAX_WINDOW, "window")
            self.center, self.norm_vars = _cmvn_flag(center, "center"), _cmvn_flag(norm_vars, "norm_vars")
            self.min_window = _cmvn_whole(self.window if min_window is None else min_window, 1, self.window, "min_window (at most window)")

    @classmethod
    def global_(cls, shift, scale, pad=0.0):
        """y = (x + shift[r]) * scale[r] in float32: FunASR's am.mvn is global_(means, vars) behind Splice.lfr()."""
        return cls(shift=shift, scale=scale, pad=pad)

    @classmethod
    def from_mean_std(cls, mean, std, pad=0.0):
        """(x - mean) * (1 / std): shift = float32(-mean), scale = float32(1 / float64(std)); WeNet's global_cmvn with istd = 1 / std."""
        mean = _cmvn_row(mean, "mean")
        std = _cmvn_row(std, "std", mean.size)
        if not np.all(std > 0):
            raise ValueError("Cmvn: std must be above 0")
        return cls(shift=-mean, scale=1.0 / std, pad=pad)

    @classmethod
    def from_kaldi_stats(cls, stats, norm_vars=True, pad=0.0):
        """From a Kaldi CMVN accumulator (compute-cmvn-stats): [2][rows + 1], the sums and the count in row 0, the sums of squares
        in row 1.  clx_cmvn_from_stats: mean = sum / count, var = max(sumsq / count - mean^2, 1e-20), shift = -mean,
        scale = 1 / sqrt(var) (1 without norm_vars), in double, rounded once.  Kaldi's apply-cmvn computes x * scale + offset, a
        different rounding of the same value."""
        norm_vars = _cmvn_flag(norm_vars, "norm_vars")
        try:
            st = np.asarray(stats)
        except Exception:
            st = None
        if st is None or st.ndim != 2 or st.shape[0] != 2 or not 2 <= st.shape[1] <= CMVN_MAX_ROWS + 1 or st.dtype.kind not in "fiu":
            raise ValueError("Cmvn: stats must be a [2][rows + 1] matrix of numbers, rows in 1..%d" % CMVN_MAX_ROWS)
        st = np.ascontiguousarray(st, dtype=np.float64)
        rows = st.shape[1] - 1
        shift, scale = np.zeros(rows, dtype=np.float32), np.zeros(rows, dtype=np.float32)
        if not np.all(np.isfinite(st[0])) or not np.all(np.isfinite(st[1, :rows])) or \
                lib().clx_cmvn_from_stats(_np_ptr(st), rows, int(norm_vars), _np_ptr(shift), _np_ptr(scale)) != OK:
            raise ValueError("Cmvn: stats must be finite, with a count above 0")
        return cls(shift=shift, scale=scale, pad=pad)

    @classmethod
    def sliding(cls, window=600, min_window=100, center=False, norm_vars=False, pad=0.0):
        """Kaldi's apply-cmvn-sliding (its defaults): --cmn-window, --min-cmn-window (only read when not centred; at most window),
        --center, --norm-vars."""
        return cls(window=window, min_window=min_window, center=center, norm_vars=norm_vars, pad=pad)

    @classmethod
    def grouped(cls, stats, norm_vars=True, pad=0.0):
        """Every window by the accumulator of its group: shift = -mean and scale = 1 / sqrt(var) (1 without norm_vars) of group g
        of `stats` (an open CmvnStats), solved on the device when the Cmvn is applied, from what the accumulator holds then."""
        if not isinstance(stats, CmvnStats) or stats._acc is None:
            raise ValueError("Cmvn: grouped() needs an open CmvnStats, not %r" % (stats,))
        self = cls.__new__(cls)
        self.pad = _cmvn_pad(pad)
        self._stats = stats
        self._shift = self._scale = None
        self.rows = stats.rows
        self.window = self.min_window = None
        self.center, self.norm_vars = False, _cmvn_flag(norm_vars, "norm_vars")
        return self

    @classmethod
    def xvector(cls, pad=0.0):
        """The x-vector / speaker-verification recipes' --cmn-window=300 --center=true --norm-vars=false."""
        return cls.sliding(300, 100, True, False, pad)

    @property
    def shift(self):
        return None if self._shift is None else self._shift.copy()

    @property
    def scale(self):
        return None if self._scale is None else self._scale.copy()

    def _sliding_opts(self):
        return _CmvnSlidingOpts(self.window, self.min_window, int(self.center), int(self.norm_vars), self.pad, 0)

    def _key(self):
        if self._stats is not None:
            return ("grouped", id(self._stats), self.norm_vars, self.pad)
        if self.rows is not None:
            return ("global", self._shift.tobytes(), self._scale.tobytes(), self.pad)
        return ("sliding", self.window, self.min_window, self.center, self.norm_vars, self.pad)

    def __repr__(self):
        if self._stats is not None:
            return "Cmvn.grouped(<%d rows, %d groups>, norm_vars=%r, pad=%r)" % (self.rows, self._stats.groups, self.norm_vars, self.pad)
        if self.rows is not None:
            return "Cmvn.global_(<%d rows>, pad=%r)" % (self.rows, self.pad)
        return "Cmvn.sliding(window=%d, min_window=%d, center=%r, norm_vars=%r, pad=%r)" % (self.window, self.min_window, self.center,
                                                                                             self.norm_vars, self.pad)

    def __eq__(self, other):
        return isinstance(other, Cmvn) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())


CMVN_MAX_GROUPS = 65536


class _CmvnStatsOpts(C.Structure):       # clx_cmvn_stats_opts
    _fields_ = [("accumulate", C.c_uint32), ("reserved", C.c_uint32)]


class _CmvnGroupedOpts(C.Structure):     # clx_cmvn_grouped_opts
    _fields_ = [("norm_vars", C.c_uint32), ("pad", C.c_float), ("reserved", C.c_uint32)]


def _cmvn_groups(who, groups, B, n_groups):
    """`groups` as the int32 array the C side is given (None: NULL, every window group 0): B whole numbers in -1..n_groups - 1."""
    if groups is None:
        return None
    try:
        a = np.asarray(groups.cpu() if hasattr(groups, "cpu") else groups)
    except Exception:
        a = None
    if a is None or a.ndim != 1 or a.dtype.kind not in "iu" or a.size != B:
        raise ValueError("%s: groups must be %d whole numbers, one per window" % (who, B))
    a = a.astype(np.int64)
    if a.size and (a.min() < -1 or a.max() >= n_groups):
        raise ValueError("%s: groups must lie in -1..%d" % (who, n_groups - 1))
    return np.ascontiguousarray(a, dtype=np.int32)


class CmvnStats:
    """Kaldi's CMVN accumulator on the device (compute-cmvn-stats): for each of `groups` groups (speakers; 1: a corpus) the sums
    and the sums of squares of every feature row over the live frames it has been given, and their number, as float64
    [groups][2][rows + 1] in Kaldi's layout (clx_cmvn_stats_windows has the definition and the order of the sums: the same calls
    leave the same words).  It owns the accumulator, zeroed at creation, and the shift / scale buffer a Cmvn.grouped(self) solves
    into.  accumulate() and reset() queue on a stream and do not wait; two calls on one CmvnStats must be ordered by the caller (one
    stream, or events).  numpy() is the one method that waits."""

    def __init__(self, ctx, rows, groups=1):
        import torch
        if not isinstance(ctx, Context) or ctx._h is None:
            raise ValueError("CmvnStats: ctx must be an open Context")
        self.ctx = ctx
        self.rows = _cmvn_whole(rows, 1, CMVN_MAX_ROWS, "rows")
        self.groups = _cmvn_whole(groups, 1, CMVN_MAX_GROUPS, "groups")
        dev = torch.device("cuda", int(ctx.device))
        self._acc = torch.zeros((self.groups, 2, self.rows + 1), dtype=torch.float64, device=dev)
        self._ss = None                                      # [groups][2][rows] float32, made by the first grouped apply
        torch.cuda.current_stream(dev).synchronize()         # (the zeros stand before any stream's first call)

    def _open(self, who):
        if self._acc is None:
            raise ValueError("CmvnStats: %s on a closed CmvnStats" % who)

    def _shift_scale(self):
        if self._ss is None:
            import torch
            self._ss = torch.empty((self.groups, 2, self.rows), dtype=torch.float32, device=self._acc.device)
        return self._ss

    def accumulate(self, data, valid, layout, groups=None, stream=None):
        """clx_cmvn_stats_windows, accumulating: adds the first valid[k] frames of every window of the dense float32 batch `data`
        -- [B, rows, T] (WINDOW_CT) or [B, T, rows] (WINDOW_TC), a CUDA tensor or a (pointer, B, rows, T) tuple -- to the
        accumulator of group groups[k] (None: group 0; -1: the window takes no part).  `data` is only read.  Asynchronous on
        `stream` as gather_windows is.  Returns self."""
        self._open("accumulate()")
        d_ptr, B, rows, T, valid, handle = self.ctx._feature_batch("CmvnStats.accumulate", data, valid, layout, stream)
        if rows != self.rows:
            raise ValueError("CmvnStats.accumulate: the CmvnStats has %d rows, the batch %d" % (self.rows, rows))
        g = _cmvn_groups("CmvnStats.accumulate", groups, B, self.groups)
        opts = _CmvnStatsOpts(1, 0)
        self.ctx._check(lib().clx_cmvn_stats_windows(self.ctx._h, d_ptr, B, rows, T, _np_ptr(valid), int(layout), _np_ptr(g) if g is not None else None,
                                                     self.groups, self._acc.data_ptr(), C.byref(opts), handle))
        return self

    def reset(self, stream=None):
        """Zeroes the accumulator: clx_cmvn_stats_windows over no window with accumulate = 0, queued on `stream` and not waited for.
        stream=None is torch's current stream of the accumulator's device -- the stream accumulate() and read_mel(stats=) take for
        a tensor when they are given none, so reset() followed by either, with no stream named, is ordered.  (As with every call
        here, torch's DEFAULT stream stands for the context's own stream.)"""
        self._open("reset()")
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self._acc.device)
        handle = getattr(stream, "cuda_stream", stream)
        opts = _CmvnStatsOpts(0, 0)
        self.ctx._check(lib().clx_cmvn_stats_windows(self.ctx._h, None, 0, self.rows, 0, None, WINDOW_CT, None, self.groups, self._acc.data_ptr(),
                                                     C.byref(opts), C.c_void_p(handle) if handle else None))
        return self

    def numpy(self):
        """The accumulator on the host, float64 [2, rows + 1] for one group, else [groups, 2, rows + 1].  WAITS for the device."""
        self._open("numpy()")
        import torch
        torch.cuda.synchronize(self._acc.device)
        a = self._acc.cpu().numpy()
        return a[0].copy() if self.groups == 1 else a

    def add_(self, array):
        """Adds another accumulator of the same shape (another rank's numpy(), a Kaldi stats file) on the host and uploads the sum.
        Waits, as numpy() does.  Returns self."""
        self._open("add_()")
        import torch
        mine = self.numpy()
        try:
            a = np.asarray(array, dtype=np.float64)
        except Exception:
            a = None
        if a is None or a.shape != mine.shape:
            raise ValueError("CmvnStats.add_: the array must be float64 of shape %r" % (mine.shape,))
        total = (mine + a).reshape(self.groups, 2, self.rows + 1)
        self._acc.copy_(torch.from_numpy(np.ascontiguousarray(total)))
        torch.cuda.synchronize(self._acc.device)
        return self

    def cmvn(self, norm_vars=True, pad=0.0):
        """Cmvn.from_kaldi_stats(self.numpy(), ...): a global Cmvn, a plain value that no longer reads this object.  One group only."""
        if self.groups != 1:
            raise ValueError("CmvnStats.cmvn: needs groups == 1; Cmvn.grouped(stats) is the one for %d groups" % self.groups)
        return Cmvn.from_kaldi_stats(self.numpy(), norm_vars=norm_vars, pad=pad)

    def as_wenet(self):
        """WeNet's global_cmvn statistics: {"mean_stat": the sums, "var_stat": the sums of squares, "frame_num": the count}, as
        lists (json.dump them).  One group only."""
        if self.groups != 1:
            raise ValueError("CmvnStats.as_wenet: needs groups == 1")
        a = self.numpy()
        return {"mean_stat": a[0, :-1].tolist(), "var_stat": a[1, :-1].tolist(), "frame_num": int(a[0, -1])}

    def close(self):
        self._acc = self._ss = None

    def __repr__(self):
        return "CmvnStats(<%d rows, %d groups>%s)" % (self.rows, self.groups, "" if self._acc is not None else ", closed")


# ---- energy VAD and frame selection ------------------------------------------------------------------------------------------------

VAD_MAX_CONTEXT, VAD_MAX_ROWS = 128, 8192


class _VadOpts(C.Structure):             # clx_vad_opts
    _fields_ = [("energy_threshold", C.c_float), ("energy_mean_scale", C.c_float), ("frames_context", C.c_uint32),
                ("proportion_threshold", C.c_float), ("row", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class _SelectOpts(C.Structure):          # clx_select_opts
    _fields_ = [("pad", C.c_float), ("reserved", C.c_uint32 * 3)]


def _vad_f32(v, what):
    """`v` as the float32 value the C side is given: a finite number."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) \
            or abs(float(v)) > float(np.finfo(np.float32).max):
        raise ValueError("Vad: %s must be a finite number, not %r" % (what, v))
    return float(np.float32(v))


def _vad_whole(v, lo, hi, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("Vad: %s must be a whole number in %d..%d, not %r" % (what, lo, hi, v))
    return int(v)


class Vad:
    """What Context.vad_windows and read_mel(..., vad=) decide for every frame: Kaldi's energy VAD (compute-vad) as this project
    reads it.  A plain value: it owns nothing on the device.  A frame's cell e of row `row` (0: C0, or the log energy, of
    MelSpec.mfcc) is above when e > energy_threshold + energy_mean_scale * (the mean of that row over the window's valid frames);
    the frame is voiced when at least proportion_threshold of the frames within frames_context of it (cut at the window's ends)
    are above.  The defaults are Kaldi's (5.0, 0.5, 0, 0.6); voxceleb() is conf/vad.conf of the VoxCeleb and SRE16 recipes (5.5,
    0.5, 2, 0.12).  select (read_mel only): keep the voiced frames alone, moved to the front (select-voiced-frames), the frames
    behind them set to pad; select=False only decides.  ValueError for an energy_threshold, energy_mean_scale or pad that is not a
    finite float32 number, a frames_context outside 0..128, a proportion_threshold that is not above 0 and below 1, a row outside
    0..8191 and a select that is not 0 / 1."""

    def __init__(self, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6, row=0, select=True, pad=0.0):
        self.energy_threshold = _vad_f32(energy_threshold, "energy_threshold")
        self.energy_mean_scale = _vad_f32(energy_mean_scale, "energy_mean_scale")
        self.frames_context = _vad_whole(frames_context, 0, VAD_MAX_CONTEXT, "frames_context")
        if isinstance(proportion_threshold, (bool, np.bool_)) or not isinstance(proportion_threshold, (int, float, np.integer, np.floating)) \
                or not 0.0 < float(np.float32(proportion_threshold)) < 1.0:
            raise ValueError("Vad: proportion_threshold must be above 0 and below 1, not %r" % (proportion_threshold,))
        self.proportion_threshold = float(np.float32(proportion_threshold))
        self.row = _vad_whole(row, 0, VAD_MAX_ROWS - 1, "row")
        if not isinstance(select, (bool, int, np.integer, np.bool_)) or int(select) not in (0, 1):
            raise ValueError("Vad: select must be 0 or 1, not %r" % (select,))
        self.select = bool(select)
        self.pad = _vad_f32(pad, "pad")

    @classmethod
    def voxceleb(cls, row=0, select=True, pad=0.0):
        """conf/vad.conf of Kaldi's VoxCeleb and SRE16 recipes: --vad-energy-threshold=5.5 --vad-energy-mean-scale=0.5
        --vad-frames-context=2 --vad-proportion-threshold=0.12."""
        return cls(5.5, 0.5, 2, 0.12, row, select, pad)

    def _opts(self):
        return _VadOpts(self.energy_threshold, self.energy_mean_scale, self.frames_context, self.proportion_threshold, self.row,
                        (C.c_uint32 * 3)(0, 0, 0))

    def _key(self):
        return (self.energy_threshold, self.energy_mean_scale, self.frames_context, self.proportion_threshold, self.row, self.select, self.pad)

    def __repr__(self):
        return "Vad(energy_threshold=%r, energy_mean_scale=%r, frames_context=%d, proportion_threshold=%r, row=%d, select=%r, pad=%r)" % self._key()

    def __eq__(self, other):
        return isinstance(other, Vad) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())


# ---- SpecAugment ----------------------------------------------------------------------------------------------------------------

SPECAUG_MAX_MASKS = 32


class _SpecAugOpts(C.Structure):         # clx_specaug_opts
    _fields_ = [("n_freq_masks", C.c_uint32), ("n_time_masks", C.c_uint32), ("fill_mean", C.c_uint32), ("fill", C.c_float), ("reserved", C.c_uint32)]


def _specaug_fill(fill, who):
    """(the fill is the mean, the constant as a float32 value) of a fill argument: "mean" or a finite number."""
    if isinstance(fill, str):
        if fill != "mean":
            raise ValueError("%s: fill must be 'mean' or a finite number, not %r" % (who, fill))
        return True, 0.0
    if isinstance(fill, bool) or not isinstance(fill, (int, float, np.integer, np.floating)) or not math.isfinite(float(fill)) \
            or abs(float(fill)) > float(np.finfo(np.float32).max):
        raise ValueError("%s: fill must be 'mean' or a finite number, not %r" % (who, fill))
    return False, float(np.float32(fill))


def _specaug_table(a, B, name, pairs=True):
    """A warp ([B, 2]) or mask ([B, n, 2]) argument as a contiguous uint32 array, None for None or a table without entries."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.size == 0:
        return None
    if a.dtype.kind not in "iu" or (a.dtype.kind == "i" and a.min() < 0) or int(a.max()) >= 1 << 32:
        raise ValueError("specaug: %s must hold whole numbers from 0 up" % name)
    if (a.ndim != 3 if pairs else a.ndim != 2) or a.shape[0] != B or a.shape[-1] != 2:
        raise ValueError("specaug: %s must be [%d, %s2], not %r" % (name, B, "n, " if pairs else "", tuple(a.shape)))
    if pairs and a.shape[1] > SPECAUG_MAX_MASKS:
        raise ValueError("specaug: %s has %d masks a window, more than %d" % (name, a.shape[1], SPECAUG_MAX_MASKS))
    return np.ascontiguousarray(a, dtype=np.uint32)


def _specaug_fit(plan, valid_frames, rows, n_frames, who):
    """ValueError unless `plan` fits a batch of len(valid_frames) windows of `rows` rows and `n_frames` frames: as many windows; every
    warp (0, 0) or within 1 .. valid_frames[k] - 1; every mask that masks something (width > 0) starting inside the batch, below
    `rows` or `n_frames`.  A mask of width 0 masks nothing wherever it starts, and one that runs past the rows, the frames or
    valid_frames[k] is clipped there, as clx_specaug_windows clips it."""
    V = np.asarray(valid_frames, dtype=np.int64).reshape(-1)
    if len(plan) != V.size:
        raise ValueError("%s: augment is a plan of %d windows for a batch of %d" % (who, len(plan), V.size))
    for name, m, limit, what in (("frequency", plan.freq_masks, rows, "rows"), ("time", plan.time_masks, n_frames, "frames")):
        if np.any((m[..., 1] > 0) & (m[..., 0] >= limit)):
            raise ValueError("%s: a %s mask of augment starts behind the batch's %d %s" % (who, name, limit, what))
    c, w = plan.warp[:, 0], plan.warp[:, 1]
    if np.any(((c != 0) | (w != 0)) & ((c < 1) | (w < 1) | (c >= V) | (w >= V))):
        raise ValueError("%s: a warp of augment is neither (0, 0) nor within 1 .. valid_frames - 1" % who)


class SpecAugmentPlan:
    """What one SpecAugment.draw gave, a plain value: warp [B, 2] (c, w), freq_masks [B, F, 2] (first row, width), time_masks
    [B, M, 2] (first output frame, width), int64 arrays, and the fill ("mean" or a float) -- the arguments of
    Context.specaug_windows, and what read_mel(..., augment=) takes in place of a policy."""

    def __init__(self, warp, freq_masks, time_masks, fill="mean"):
        self.warp = np.ascontiguousarray(warp, dtype=np.int64).reshape(-1, 2)
        B = self.warp.shape[0]
        self.freq_masks = np.ascontiguousarray(freq_masks, dtype=np.int64)
        self.time_masks = np.ascontiguousarray(time_masks, dtype=np.int64)
        for name, a in (("freq_masks", self.freq_masks), ("time_masks", self.time_masks)):
            if a.ndim != 3 or a.shape[0] != B or a.shape[2] != 2:
                raise ValueError("SpecAugmentPlan: %s must be [%d, n, 2], not %r" % (name, B, tuple(a.shape)))
        if self.freq_masks.shape[1] > SPECAUG_MAX_MASKS or self.time_masks.shape[1] > SPECAUG_MAX_MASKS:
            raise ValueError("SpecAugmentPlan: more than %d masks a window" % SPECAUG_MAX_MASKS)
        if min(self.warp.min(initial=0), self.freq_masks.min(initial=0), self.time_masks.min(initial=0)) < 0:
            raise ValueError("SpecAugmentPlan: a negative entry")
        mean, value = _specaug_fill(fill, "SpecAugmentPlan")
        self.fill = "mean" if mean else value

    def __len__(self):
        return self.warp.shape[0]

    def __repr__(self):
        return "SpecAugmentPlan(%d windows, %d frequency masks, %d time masks, fill=%r)" % (
            len(self), self.freq_masks.shape[1], self.time_masks.shape[1], self.fill)

    def __eq__(self, other):
        return isinstance(other, SpecAugmentPlan) and self.fill == other.fill and np.array_equal(self.warp, other.warp) \
            and np.array_equal(self.freq_masks, other.freq_masks) and np.array_equal(self.time_masks, other.time_masks)

    __hash__ = None


class SpecAugment:
    """The SpecAugment policy of read_mel(..., augment=): a time warp, frequency masks and time masks per window, drawn on the host
    by numpy from `seed` and applied by one clx_specaug_windows call (claxon_hip.h has what a warp and a mask do to the cells).
    A plain value; draw() gives the SpecAugmentPlan of one batch.  The rule is this library's own, in the spirit of lhotse's
    SpecAugment (whose defaults these are); it is not lhotse's random stream and gives other draws from the same seed.

    draw(valid_frames, rows): a Generator, numpy.random.default_rng(seed), made once by the constructor, gives for every window
    in turn, V its valid frames, 3 + 2 freq_masks + 2 time_masks uniform doubles u in [0, 1) in this order, all of them whether
    they are used or not (so a window's draws do not depend on the windows before it being short):
      skip      u0 >= p: the window is left alone -- warp (0, 0), every mask of width 0.
      warp      W = time_warp.  W == 0 or V < 2 W + 2: the window is too short, no warp.  Otherwise c = W + 1 + floor(u1 (V - 2 W - 1))
                lies in [W + 1, V - W - 1] and w = c - W + floor(u2 (2 W + 1)) in [c - W, c + W], hence both in [1, V - 1].  (w == c
                is a warp that copies.)
      freq      mask i: width = floor(u (min(freq_width, rows) + 1)) in [0, min(freq_width, rows)], then first =
                floor(u' (rows - width + 1)) in [0, rows - width].
      time      a budget of floor(max_time_fraction V) frames.  Mask i: width = floor(u (min(time_width, V) + 1)), cut to what is
                left of the budget, which it then uses up; first = floor(u' (V - width + 1)) in [0, V - width].  The widths of a
                window's time masks therefore add up to at most max_time_fraction V frames, and so do the frames they cover.
    ValueError for counts outside 0..32, negative widths, a p or max_time_fraction outside [0, 1] and a fill that is neither
    "mean" nor a finite number."""

    def __init__(self, time_warp=80, freq_masks=2, freq_width=27, time_masks=10, time_width=100, max_time_fraction=0.15, p=0.9, fill="mean",
                 seed=None):
        for name, v, hi in (("time_warp", time_warp, (1 << 30) - 1), ("freq_masks", freq_masks, SPECAUG_MAX_MASKS), ("freq_width", freq_width, (1 << 31) - 1),
                            ("time_masks", time_masks, SPECAUG_MAX_MASKS), ("time_width", time_width, (1 << 31) - 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= hi:
                raise ValueError("SpecAugment: %s must be a whole number in 0..%d, not %r" % (name, hi, v))
        for name, v in (("max_time_fraction", max_time_fraction), ("p", p)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
                raise ValueError("SpecAugment: %s must be a number in [0, 1], not %r" % (name, v))
        mean, value = _specaug_fill(fill, "SpecAugment")
        self.time_warp, self.freq_masks, self.freq_width = int(time_warp), int(freq_masks), int(freq_width)
        self.time_masks, self.time_width = int(time_masks), int(time_width)
        self.max_time_fraction, self.p = float(max_time_fraction), float(p)
        self.fill = "mean" if mean else value
        self.seed = seed
        self._rng = np.random.default_rng(seed)

    def __repr__(self):
        return "SpecAugment(time_warp=%d, freq_masks=%d, freq_width=%d, time_masks=%d, time_width=%d, max_time_fraction=%r, p=%r, fill=%r, seed=%r)" % (
            self.time_warp, self.freq_masks, self.freq_width, self.time_masks, self.time_width, self.max_time_fraction, self.p, self.fill, self.seed)

    def draw(self, valid_frames, rows):
        """The plan of one batch: valid_frames [B] whole numbers from 0 up, rows the batch's rows (1..256)."""
        vf = np.asarray(valid_frames).reshape(-1)
        if vf.size and (vf.dtype.kind not in "iu" or int(vf.min()) < 0 or int(vf.max()) >= 1 << 31):
            raise ValueError("SpecAugment.draw: valid_frames must hold whole numbers in 0..2^31 - 1")
        if isinstance(rows, bool) or int(rows) != rows or not 1 <= int(rows) <= 256:
            raise ValueError("SpecAugment.draw: rows must be 1..256, not %r" % (rows,))
        rows, B, F, M, W = int(rows), vf.size, self.freq_masks, self.time_masks, self.time_warp
        warp = np.zeros((B, 2), dtype=np.int64)
        fm = np.zeros((B, F, 2), dtype=np.int64)
        tm = np.zeros((B, M, 2), dtype=np.int64)
        for k in range(B):
            V = int(vf[k])
            u = self._rng.random(3 + 2 * F + 2 * M)
            if u[0] >= self.p:
                continue
            if W > 0 and V >= 2 * W + 2:
                c = W + 1 + int(u[1] * (V - 2 * W - 1))
                warp[k] = (c, c - W + int(u[2] * (2 * W + 1)))
            for i in range(F):
                width = int(u[3 + 2 * i] * (min(self.freq_width, rows) + 1))
                fm[k, i] = (int(u[4 + 2 * i] * (rows - width + 1)), width)
            left = int(self.max_time_fraction * V)
            for i in range(M):
                width = min(int(u[3 + 2 * F + 2 * i] * (min(self.time_width, V) + 1)), left)
                left -= width
                tm[k, i] = (int(u[4 + 2 * F + 2 * i] * (V - width + 1)), width)
        return SpecAugmentPlan(warp, fm, tm, self.fill)


# ---- a second recording behind the windows ----------------------------------------------------------------------------------------

class Add:
    """What read(..., add=) and read_mel(..., add=) mix into their windows (clx_add_windows, claxon_hip.h): window k receives the
    samples of stream stream_ids[k] of `source` from sample starts[k] on (counted as read() counts them, at the call's sample
    rate), scaled so that the window's mean power over its valid samples lies snr_db[k] dB above the mean power of the noise
    samples inside them.  `source` is a StreamSet of the reading set's context, None the reading set itself; a stream id of -1
    gives that window no noise; snr_db is a scalar or one value per window, finite within -200 .. 200 or +inf (nothing added).
    A noise stream that ends inside the window is added as far as it goes and counted over that part only; it is not repeated.
    A plain value: it owns nothing on the device.  ValueError for arrays that differ in length, an id below -1, a negative start
    and a snr_db that is NaN, -inf or beyond 200 in magnitude; the read refuses lengths that differ from its own, an id the source
    does not have, a closed source and a source of another context.

    offsets (a scalar or one value per window, >= 0, in samples at the call's rate) is the window sample at which the noise enters:
    a foreground noise dropped in along the utterance.  tile (a bool, or one per window) repeats the noise from its live end --
    the noise window's valid length, min(what the stream has from starts[k] on, the call's length) -- over the rest of the window:
    music or background noise looped under the whole utterance.  The gain then counts the noise over the samples it sounds on, as
    often as they sound (clx_addn_windows, claxon_hip.h).  An Add with an offset or a tile, and every Add in a list
    (add=[Add, ...]: babble, several foreground noises), goes through clx_addn_windows; a plain one alone goes through
    clx_add_windows as ever.  ValueError also for a negative offset and for offsets or tile of another length."""

    def __init__(self, stream_ids, starts, snr_db, source=None, offsets=0, tile=False):
        if source is not None and not isinstance(source, StreamSet):
            raise ValueError("Add: source must be a StreamSet or None, not %r" % (source,))
        self.stream_ids = np.array(stream_ids, dtype=np.int64).reshape(-1)
        self.starts = np.array(starts, dtype=np.int64).reshape(-1)
        if self.stream_ids.size != self.starts.size:
            raise ValueError("Add: stream_ids and starts differ in length")
        snr = np.array(snr_db, dtype=np.float32)
        if snr.ndim == 0:
            snr = np.full(self.stream_ids.size, snr, dtype=np.float32)
        self.snr_db = snr.reshape(-1)
        if self.snr_db.size != self.stream_ids.size:
            raise ValueError("Add: snr_db must be a scalar or one value per window")
        if self.stream_ids.size and self.stream_ids.min() < -1:
            raise ValueError("Add: a stream id is below -1")
        if np.any((self.starts < 0) & (self.stream_ids >= 0)):
            raise ValueError("Add: a noise window starts before its stream")
        if np.any(np.isnan(self.snr_db) | (np.isinf(self.snr_db) & (self.snr_db < 0)) | (np.isfinite(self.snr_db) & (np.abs(self.snr_db) > 200))):
            raise ValueError("Add: snr_db must be within -200 .. 200, or +inf")
        off = np.array(offsets)
        if off.dtype.kind not in "iu" or off.ndim > 1:
            raise ValueError("Add: offsets must be a whole number or one per window")
        off = off.astype(np.int64)
        self.offsets = np.full(self.stream_ids.size, off, dtype=np.int64) if off.ndim == 0 else off
        til = np.array(tile)
        if til.dtype.kind != "b" or til.ndim > 1:
            raise ValueError("Add: tile must be a bool or one per window")
        self.tile = np.full(self.stream_ids.size, til, dtype=bool) if til.ndim == 0 else til
        if self.offsets.size != self.stream_ids.size or self.tile.size != self.stream_ids.size:
            raise ValueError("Add: offsets and tile must be scalars or one value per window")
        if self.offsets.size and self.offsets.min() < 0:
            raise ValueError("Add: an offset is negative")
        self.source = source

    @property
    def plain(self):
        """Whether clx_add_windows can take it: every offset 0, no tile."""
        return not (np.any(self.offsets != 0) or np.any(self.tile))

    def __len__(self):
        return int(self.stream_ids.size)

    def __repr__(self):
        return "Add(%d windows, %d with noise, source=%s)" % (len(self), int((self.stream_ids >= 0).sum()), "None" if self.source is None else "StreamSet")

    def _plan(self, reader, B, ch, channels, who):
        """The refusals of a read of B windows with `ch` channels: (source, the windows with noise)."""
        src = reader if self.source is None else self.source
        if src._descs is None:
            raise ValueError("%s: add's source is closed" % who)
        if src.ctx is not reader.ctx:
            raise ValueError("%s: add's source belongs to another context" % who)
        if len(self) != B:
            raise ValueError("%s: add has %d windows, the call %d" % (who, len(self), B))
        sel = np.nonzero(self.stream_ids >= 0)[0]
        if sel.size and self.stream_ids.max() >= len(src):
            raise ValueError("%s: add names a stream its source does not have" % who)
        if channels is None:
            for k in sel.tolist():
                s = int(self.stream_ids[k])
                if src.problems[s] is None and src.channels[s] != ch:
                    raise ValueError("%s: noise stream %d has %d channels, the windows %d (window %d); channels= brings them together"
                                     % (who, s, src.channels[s], ch, k))
        return src, sel


def _adds_of(add, who):
    """add= as a list of Adds: None, one Add, or a list or tuple of 1..16 of them."""
    if add is None:
        return []
    if isinstance(add, Add):
        return [add]
    if isinstance(add, (list, tuple)) and 1 <= len(add) <= ADDN_MAX_TERMS and all(isinstance(a, Add) for a in add):
        return list(add)
    raise ValueError("%s: add must be an Add, a list of 1..%d Adds or None, not %r" % (who, ADDN_MAX_TERMS, add))


# ---- room impulse responses over the windows ------------------------------------------------------------------------------------

REVERB_TAPS_LIMIT = 1 << 16            # the most taps of a response: clx_reverb_windows' K


class _ReverbOpts(C.Structure):          # clx_reverb_opts
    _fields_ = [("keep_power", C.c_uint32), ("reserved", C.c_uint32)]


class _ReverbFftOpts(C.Structure):       # clx_reverb_fft_opts
    _fields_ = [("keep_power", C.c_uint32), ("reserved", C.c_uint32 * 3)]


REVERB_METHODS = ("direct", "fft", "auto")      # clx_reverb_windows, clx_reverb_windows_fft, the choice between them by the taps
# method="auto" takes the FFT form from this many taps on: the smallest probed tap count from which read(reverb=, method="fft") is
# faster than the direct form's read by more than the run-to-run spread (profiles/reverb_fft_probe.txt: at 800 taps 3.64 ms against
# 3.62 ms, no gain; at 4 000 taps 3.60 ms against 4.98 ms, the slowest FFT read faster than the fastest direct one)
REVERB_FFT_TAPS = 4000


def _reverb_method(method, who):
    if not isinstance(method, str) or method not in REVERB_METHODS:
        raise ValueError("%s: method must be one of %s, not %r" % (who, ", ".join(repr(m) for m in REVERB_METHODS), method))
    return method


def reverb_method_for(method, taps):
    """The method a call with responses of `taps` taps (clx_reverb_windows' K) runs: "auto" is "fft" from REVERB_FFT_TAPS on."""
    method = _reverb_method(method, "reverb_method_for")
    return method if method != "auto" else ("fft" if int(taps) >= REVERB_FFT_TAPS else "direct")


class Reverb:
    """What read(..., reverb=) and read_mel(..., reverb=) convolve their windows with (clx_reverb_windows, claxon_hip.h): window k
    is convolved with stream stream_ids[k] of `source`, a StreamSet of the reading set's context that holds mono impulse responses;
    a stream id of -1 leaves that window as it is.  The response is read from sample starts[k] on (a scalar or one value per
    window, counted as read() counts them, at the call's sample rate: a caller skips the pre-delay with it) and truncated to `taps`
    samples; taps=None takes the longest named response at that rate.  keep_power=True rescales every reverberated window to the
    power of its dry signal.  method="direct" (the default) convolves with clx_reverb_windows, method="fft" with
    clx_reverb_windows_fft, the partitioned FFT form for long responses, method="auto" with the latter from REVERB_FFT_TAPS taps on
    (the taps of the call: `taps`, or the longest named response).  The window is the crop: what the stream held before it leaves no tail in it.  A plain value: it owns
    nothing on the device.  ValueError for a source that is no StreamSet, arrays that differ in length, an id below -1, a negative
    start, taps outside 1 .. 65536 and a method that is neither; the read refuses lengths that differ from its own, an id the source does not have, a
    response stream that is not mono, a closed source and a source of another context."""

    def __init__(self, stream_ids, source, starts=0, taps=None, keep_power=True, method="direct"):
        self.method = _reverb_method(method, "Reverb")
        if not isinstance(source, StreamSet):
            raise ValueError("Reverb: source must be a StreamSet, not %r" % (source,))
        self.stream_ids = np.array(stream_ids, dtype=np.int64).reshape(-1)
        st = np.array(starts, dtype=np.int64)
        if st.ndim == 0:
            st = np.full(self.stream_ids.size, st, dtype=np.int64)
        self.starts = st.reshape(-1)
        if self.stream_ids.size != self.starts.size:
            raise ValueError("Reverb: starts must be a scalar or one value per window")
        if self.stream_ids.size and self.stream_ids.min() < -1:
            raise ValueError("Reverb: a stream id is below -1")
        if np.any((self.starts < 0) & (self.stream_ids >= 0)):
            raise ValueError("Reverb: a response starts before its stream")
        if taps is not None:
            if isinstance(taps, bool) or int(taps) != taps or not 1 <= int(taps) <= REVERB_TAPS_LIMIT:
                raise ValueError("Reverb: taps must be None or a whole number in 1 .. %d, not %r" % (REVERB_TAPS_LIMIT, taps))
            taps = int(taps)
        self.taps = taps
        self.keep_power = bool(keep_power)
        self.source = source

    def __len__(self):
        return int(self.stream_ids.size)

    def __repr__(self):
        return "Reverb(%d windows, %d with a response, taps=%s, keep_power=%s, method=%r)" % (len(self), int((self.stream_ids >= 0).sum()), self.taps,
                                                                                              self.keep_power, self.method)

    def _plan(self, reader, B, sample_rate, who):
        """The refusals of a read of B windows at sample_rate (None: the streams' own): (the windows with a response, taps)."""
        src = self.source
        if src._descs is None:
            raise ValueError("%s: reverb's source is closed" % who)
        if src.ctx is not reader.ctx:
            raise ValueError("%s: reverb's source belongs to another context" % who)
        if len(self) != B:
            raise ValueError("%s: reverb has %d windows, the call %d" % (who, len(self), B))
        sel = np.nonzero(self.stream_ids >= 0)[0]
        if sel.size and self.stream_ids.max() >= len(src):
            raise ValueError("%s: reverb names a stream its source does not have" % who)
        for k in sel.tolist():
            s = int(self.stream_ids[k])
            if src.problems[s] is None and src.channels[s] != 1:
                raise ValueError("%s: response stream %d has %d channels, not one (window %d)" % (who, s, src.channels[s], k))
        taps = self.taps
        if taps is None and sel.size:                        # the longest named response, from its start on, at the call's rate
            ids = self.stream_ids[sel]
            named = [int(s) for s in ids.tolist() if src.problems[int(s)] is None]
            if sample_rate is None:
                lens = src._lengths[ids]
            else:
                _, pairs = src._check_rate(sample_rate, set(named), who)
                lens = np.array([0 if src.problems[int(s)] is not None else
                                 (int(src._lengths[int(s)]) * pairs[src.sample_rates[int(s)]][1] + pairs[src.sample_rates[int(s)]][0] - 1)
                                 // pairs[src.sample_rates[int(s)]][0] for s in ids.tolist()], dtype=np.int64)
            taps = int(np.clip(lens - self.starts[sel], 0, None).max())
            if taps > REVERB_TAPS_LIMIT:
                raise ValueError("%s: the longest response has %d samples, more than %d; taps= truncates it" % (who, taps, REVERB_TAPS_LIMIT))
        return sel, int(taps or 0)


# ---- sample windows from resident streams -----------------------------------------------------------------------------------------

_LAYOUTS = {"tc": WINDOW_TC, "ct": WINDOW_CT}
RESAMPLE_RATE_LIMIT = 1 << 20          # rates are 1 .. 2^20 - 1: the width of STREAMINFO's field
RESAMPLE_TABLE_LIMIT = 1 << 18         # the most entries of a rate pair's [n, 2W] coefficient table


def resample_pair(src_rate, out_rate):
    """(o, n, W) of the fixed resampler (claxon_hip.h, clx_resample_windows) for src_rate -> out_rate: the reduced pair and the
    filter's half width in source samples; W = 0 for equal rates, where a window is a plain copy."""
    g = math.gcd(int(src_rate), int(out_rate))
    o, n = int(src_rate) // g, int(out_rate) // g
    return (o, n, 0) if o == n else (o, n, int(math.ceil(6 * o / (min(o, n) * 0.99))))


class StreamSet:
    """FLAC streams resident on the GPU, uploaded and indexed once (open_streams), from which read() draws batches of fixed-length
    sample windows by decoding only the frames that cover them.  Per stream: lengths (int64 tensor, samples per channel: the sum of
    the indexed block sizes, load()'s T), channels, sample_rates, bits_per_sample, and problems -- None, or the ClaxonError that keeps
    the stream from being read (0 / None in the other lists).  frames_decoded counts the frames read() has handed to the decoder."""

    def __init__(self, ctx, streams):
        import torch
        self.ctx = ctx
        arrs = [_u8(s) for s in streams]
        n, short = len(arrs), []
        self._arena, self._arena_len, entries = _index_streams(ctx, arrs, short)
        short = dict(short)
        self.problems, self.channels, self.sample_rates, self.bits_per_sample = [None] * n, [0] * n, [0] * n, [0] * n
        lengths = np.zeros(n, dtype=np.int64)
        self._first = np.zeros(n + 1, dtype=np.int64)         # stream k's frames are rows _first[k] .. _first[k + 1] of the tables below
        self._base = np.zeros(n + 1, dtype=np.int64)          # ... and its samples sit at _base[k] .. in the set's one sample axis
        descs = []
        for k, e in enumerate(entries):
            if isinstance(e, ClaxonError):
                self.problems[k] = e
            elif k in short:
                self.problems[k] = ClaxonError(FORMAT_ERROR, 0, "the frame index stops at byte %d of %d" % (short[k], arrs[k].size))
            elif e[0].size and np.any(e[0]["n_channels"] != e[2]):
                self.problems[k] = ClaxonError(FORMAT_ERROR, 0, "the stream's frames differ in their channel count")
            else:
                d, self.sample_rates[k], self.channels[k], si = e
                self.bits_per_sample[k] = int(d["bps"][0]) if d.size else int(si.bits_per_sample)
                lengths[k] = int(d["block_size"].astype(np.int64).sum())
                descs.append(d)
            self._first[k + 1] = self._first[k] + (descs[-1].size if self.problems[k] is None else 0)
            self._base[k + 1] = self._base[k] + lengths[k]
        self._descs = np.concatenate(descs) if descs else np.zeros(0, dtype=FRAME_DESC_DTYPE)
        bs = self._descs["block_size"].astype(np.int64)
        self._start = np.cumsum(bs) - bs                      # a frame's first sample in the set's sample axis (load()'s count: by block size)
        self._local = self._start - np.repeat(self._base[:-1], np.diff(self._first))      # ... and within its own stream
        self._lengths = lengths
        self.lengths = torch.from_numpy(lengths.copy())
        self.frames_decoded = 0

    def __len__(self):
        return len(self.problems)

    def close(self):
        """Drops the arena (the device memory goes back to torch's allocator); the set reads nothing afterwards."""
        self._arena = None
        self._descs = None

    def _check_rate(self, sample_rate, streams, who):
        """sample_rate as an int, after the refusals: {stream's rate: (o, n, W)} for the rates of `streams`."""
        if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate:
            raise ValueError("%s: sample_rate must be a whole number" % who)
        R = int(sample_rate)
        if not 0 < R < RESAMPLE_RATE_LIMIT:
            raise ValueError("%s: sample_rate must be 1 .. %d, not %d" % (who, RESAMPLE_RATE_LIMIT - 1, R))
        pairs = {}
        for fs in {self.sample_rates[s] for s in streams if self.problems[s] is None}:
            if not 0 < fs < RESAMPLE_RATE_LIMIT:
                raise ValueError("%s: a stream's sample rate is %d" % (who, fs))
            pairs[fs] = o, n, W = resample_pair(fs, R)
            if n * 2 * W > RESAMPLE_TABLE_LIMIT:
                raise ValueError("%s: resampling %d Hz to %d Hz needs a coefficient table of %d x %d entries, more than %d"
                                 % (who, fs, R, n, 2 * W, RESAMPLE_TABLE_LIMIT))
        return R, pairs

    def lengths_at(self, sample_rate):
        """Every stream's length in samples per channel after resampling to sample_rate, ceil(T * n / o), as an int64 tensor (0 for a
        problem stream): what read(..., sample_rate=sample_rate) counts starts and valid against."""
        import torch
        R, pairs = self._check_rate(sample_rate, range(len(self)), "lengths_at")
        out = np.zeros(len(self), dtype=np.int64)
        for s in range(len(self)):
            if self.problems[s] is None:
                o, n, _ = pairs[self.sample_rates[s]]
                out[s] = (int(self._lengths[s]) * n + o - 1) // o
        return torch.from_numpy(out)

    def read(self, stream_ids, starts, length, layout="tc", sample_rate=None, channels=None, normalize=None, add=None, return_gains=False,
             reverb=None):
        """A batch of windows: window k is samples [starts[k], starts[k] + length) of stream stream_ids[k], positions counted as load()
        counts them (by cumulative block size in frame order; the frame headers' sample numbers are not consulted).  Returns (float32
        tensor on the context's GPU, contiguous: [B, length, C] for layout "tc", [B, C, length] for "ct"; valid): valid[k] =
        clamp(lengths[s] - starts[k], 0, length) as an int64 tensor, the rest of a window is zeros, and a window that starts at or
        behind its stream's end is all zeros and decodes nothing.  Only the frames that cover a window are decoded, with one plan
        (OUT_F32 | VERIFY_CRC16) and one run for the call, into a scratch tensor where each window's frames sit back to back from a
        multiple of 8 floats; one clx_gather_windows launch then cuts the windows out of it.  Frames shared by overlapping windows are
        decoded once per window.  Raises ValueError for a negative start or length, an unknown stream id or layout, or windows whose
        streams differ in channel count; the stream's `problems` entry when a window names a problem stream; ClaxonError with a
        failing frame's status and message, " (window k, stream s)" appended.  The result is ready on the current torch stream.

        With sample_rate=R the windows are read at R Hz whatever rate each stream has: starts and length count samples at R, window k
        is outputs [starts[k], starts[k] + length) of its stream resampled by the fixed windowed-sinc resampler of
        clx_resample_windows (claxon_hip.h), zero padding at both ends of the stream, and valid[k] =
        clamp(lengths_at(R)[s] - starts[k], 0, length).  The frames decoded are those that cover the filter's source span
        [max(0, floor(m0*o/n) - W + 1), min(T, floor(m1*o/n) + W + 1)) of the window's first and last live output m0 and m1; one
        clx_resample_windows launch takes the place of the gather.  Streams of different rates may share a call; a window of a stream
        whose rate is R is the copy that read() without sample_rate gives.  ValueError for a sample_rate that is not 1 .. 2^20 - 1 and
        for a rate pair whose coefficient table would have more than 2^18 entries (44100 -> 16001).

        With channels=K (1..8) every window has K channels whatever its stream has -- the result is [B, length, K] / [B, K, length] --
        and streams of different channel counts share the call: a stream of K channels is read as ever, a multi-channel stream is
        averaged to K == 1 (the float32 mean of clx_mix_windows, claxon_hip.h; before the resampler when sample_rate is given) and a
        mono stream is copied to each of the K channels.  valid, the frames decoded, the plan and the run do not change; where some
        window's stream has another count than K, one clx_mix_windows launch takes the place of the gather or the resampler.
        ValueError for a K that is not a whole number in 1..8 and for a window whose stream has neither K channels nor one, with K not
        1.

        With normalize=Norm(...) every window is then normalised per channel over its valid[k] samples (after resampling and
        channels=): one clx_norm_windows call on the result, queued behind the launch that cut the windows; the samples from valid[k]
        on become the Norm's pad.  The return value is the same pair.  ValueError for a normalize that is not a Norm.

        With add=Add(...) a second recording is mixed into every window at a signal-to-noise ratio, before normalize=: a second
        read() on the Add's source (this set when it names none) for the windows whose noise stream id is not -1, with this call's
        length, layout, sample_rate and channels -- the source's frames_decoded counts its frames --, then one clx_add_windows call
        behind both (claxon_hip.h has the gain: the ratio of mean powers over each side's live samples).  valid is the signal's; a
        noise stream that ends inside a window is added as far as it goes.  With channels=None the noise streams must have the
        windows' channel count.  return_gains=True appends the windows' gains (float32 [B] on the GPU, 0 where nothing was added) to
        the return value.  ValueError for an add that is not an Add, whose length is not this call's, that names a stream its
        source does not have, or whose source is closed or of another context.  Other gain rules are not offered.

        add= also takes a list of 1..16 Adds -- babble, several foreground noises, music under speech and a noise on top -- and
        Adds with offsets= (the noise enters at that window sample) or tile= (the noise is looped from its live end over the rest
        of the window).  All of them go through ONE clx_addn_windows call (claxon_hip.h), which passes over the batch once: every
        gain is taken against the signal as it arrives, not against what an earlier Add left, and a cell receives its terms in
        list order.  One noise read() per distinct source that some window names (None counts as this set), the windows of the
        Adds that share a source stacked in one read, with this call's length, layout, sample_rate and channels: a looped
        noise's period is its noise window's valid length, min(what the stream has from starts[k] on, length).  An Add whose
        stream id is -1 for a window adds
        nothing there.  With a list return_gains=True appends float32 [B, S], 0 where nothing was added; with a single Add it stays
        [B].  A single Add with every offset 0 and no tile, not in a list, goes to clx_add_windows exactly as before.  The refusals
        above apply to each Add; ValueError also for a list that is empty, longer than 16 or holds something else, and for more
        than 8 distinct sources.

        With reverb=Reverb(...) every window is convolved with a room impulse response between the crop (resampling and channels=
        included) and add=, so that noise is added to the reverberant signal and normalize= sees both: one
        source.read(ids, starts, taps, "ct", sample_rate=sample_rate, channels=None) on the Reverb's source for the windows whose
        response id is not -1 -- the source's frames_decoded counts its frames --, then one clx_reverb_windows call behind both
        (claxon_hip.h has the cells: an ascending chain of fused multiply-adds over the window, which is the crop; with keep_power
        the window is then rescaled to its dry power).  Every channel of a window gets the same response.  valid is unchanged: the
        tail past the window's end is cut.  return_gains keeps its meaning for add.  ValueError for a reverb that is not a Reverb,
        whose length is not this call's, that names a stream its source does not have or one that is not mono, or whose source is
        closed or of another context.  reverb=None is the call without the argument."""
        if normalize is not None and not isinstance(normalize, Norm):
            raise ValueError("read: normalize must be a Norm or None, not %r" % (normalize,))
        adds = _adds_of(add, "read")
        if reverb is not None and not isinstance(reverb, Reverb):
            raise ValueError("read: reverb must be a Reverb or None, not %r" % (reverb,))
        import torch
        if self._descs is None:
            raise ValueError("read: the stream set is closed")
        if layout not in _LAYOUTS:
            raise ValueError("read: layout must be 'tc' or 'ct', not %r" % (layout,))
        length = int(length)
        if length < 0:
            raise ValueError("read: length must not be negative")
        sid = np.asarray(stream_ids, dtype=np.int64).reshape(-1)
        st = np.asarray(starts, dtype=np.int64).reshape(-1)
        if sid.size != st.size:
            raise ValueError("read: stream_ids and starts differ in length")
        if sid.size and (sid.min() < 0 or sid.max() >= len(self)):
            raise ValueError("read: unknown stream id")
        if st.size and st.min() < 0:
            raise ValueError("read: a window starts before its stream")
        for s in sid.tolist():
            if self.problems[s] is not None:
                raise self.problems[s]
        cw = np.array([self.channels[s] for s in sid.tolist()], dtype=np.int64)         # each window's stream's channel count
        if channels is None:
            chans = {self.channels[s] for s in set(sid.tolist())} or {c for c, p in zip(self.channels, self.problems) if p is None}
            if len(chans) > 1 and sid.size:
                raise ValueError("read: the windows' streams differ in their channel count (%s)" % sorted(chans))
            ch = chans.pop() if len(chans) == 1 else 0
        else:
            if isinstance(channels, bool) or not isinstance(channels, (int, float, np.integer, np.floating)) or int(channels) != channels \
                    or not 1 <= int(channels) <= 8:
                raise ValueError("read: channels must be a whole number in 1..8, not %r" % (channels,))
            ch = int(channels)
            odd = np.nonzero((cw != ch) & (cw != 1) & (ch != 1))[0]
            if odd.size:
                k = int(odd[0])
                raise ValueError("read: no rule brings the %d channels of stream %d to %d (window %d)" % (int(cw[k]), int(sid[k]), ch, k))
        mixed = bool(np.any(cw != ch))                       # (only with channels=K: some window is reduced or replicated)
        add_plans = [a._plan(self, sid.size, ch, channels, "read") for a in adds]
        if len({id(src) for src, sel in add_plans if sel.size}) > ADDN_MAX_BATCHES:
            raise ValueError("read: add names more than %d distinct sources" % ADDN_MAX_BATCHES)
        if reverb is not None:
            rv_sel, rv_taps = reverb._plan(self, sid.size, sample_rate, "read")
        B, dev = sid.size, "cuda:%d" % self.ctx.device
        if sample_rate is None:
            valid = np.clip(self._lengths[sid] - st, 0, length)
        else:
            R, pairs = self._check_rate(sample_rate, set(sid.tolist()), "read")
            onw = np.array([pairs[self.sample_rates[s]] for s in sid.tolist()], dtype=np.int64).reshape(-1, 3)
            o, n, W = onw[:, 0], onw[:, 1], onw[:, 2]
            valid = np.clip((self._lengths[sid] * n + o - 1) // o - st, 0, length)
        shape = (B, length, ch) if layout == "tc" else (B, ch, length)
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        if B == 0 or length == 0:
            return (out, torch.from_numpy(valid)) + ((torch.zeros(B if isinstance(add, Add) or not adds else (B, len(adds)), dtype=torch.float32, device=dev),)
                                                     if return_gains else ())
        live = np.nonzero(valid > 0)[0]
        # a live window's source span [lo, hi) in its stream's samples: the window itself, or what the filter reaches from it
        lo, hi = st[live], st[live] + valid[live]
        if sample_rate is not None:
            ol, nl, Wl = o[live], n[live], W[live]
            copy = Wl == 0
            lo = np.where(copy, lo, np.maximum(lo * ol // nl - Wl + 1, 0))
            hi = np.where(copy, hi, np.minimum((hi - 1) * ol // nl + Wl + 1, self._lengths[sid[live]]))
        cl = cw[live]
        # the covering frames: a searchsorted on the cumulative sample starts (one axis for the whole set: a live window lies inside its stream)
        f0 = np.searchsorted(self._start, self._base[sid[live]] + lo, side="right") - 1
        f1 = np.searchsorted(self._start, self._base[sid[live]] + hi - 1, side="right") - 1
        cnt = f1 - f0 + 1
        ends = np.cumsum(cnt)
        rows = np.repeat(f0 - (ends - cnt), cnt) + np.arange(int(ends[-1]) if live.size else 0)
        span = (self._start[f1] + self._descs["block_size"][f1].astype(np.int64) - self._start[f0]) * cl      # floats of a window's frames
        room = (span + 7) // 8 * 8
        base = np.cumsum(room) - room
        out_offs = np.repeat(base - self._start[f0] * cl, cnt) + self._start[rows] * np.repeat(cl, cnt)
        src_first = np.zeros(B, dtype=np.uint64)
        src_first[live] = base + (lo - self._local[f0]) * cl
        scratch = torch.empty(max(int(room.sum()), 8), dtype=torch.float32, device=dev)
        if rows.size:
            res = _decode_f32(self.ctx, self._arena, self._arena_len, self._descs[rows], out_offs.astype(np.uint64), scratch)
            self.frames_decoded += int(rows.size)
            bad = np.nonzero(np.asarray(res["status"]) != OK)[0]
            if bad.size:
                k = int(live[int(np.searchsorted(ends, int(bad[0]), side="right"))])
                _raise_first_failure(res, " (window %d, stream %d)" % (k, int(sid[k])))
        if sample_rate is None and not mixed:
            self.ctx.gather_windows(scratch, src_first, valid, length, ch, _LAYOUTS[layout], out)
        else:
            src_t0, src_n = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.uint32)
            src_t0[live], src_n[live] = lo, hi - lo
            if sample_rate is None:                          # (mixed at the native rate: every window a copy, "rate 1 to rate 1")
                rates, R = np.ones(B, dtype=np.uint32), 1
            else:
                rates = np.array([self.sample_rates[s] for s in sid.tolist()], dtype=np.uint32)
            if mixed:
                self.ctx.mix_windows(scratch, src_first, src_t0, src_n, np.where(valid > 0, st, 0), valid, rates, cw, R, length, ch,
                                     _LAYOUTS[layout], out)
            else:
                self.ctx.resample_windows(scratch, src_first, src_t0, src_n, np.where(valid > 0, st, 0), valid, rates, R, length, ch,
                                          _LAYOUTS[layout], out)
        if reverb is not None and ch > 0 and rv_sel.size > 0 and rv_taps > 0:
            ir, ir_len = reverb.source.read(reverb.stream_ids[rv_sel], reverb.starts[rv_sel], rv_taps, "ct", sample_rate=sample_rate, channels=None)
            index = np.full(B, -1, dtype=np.int32)
            index[rv_sel] = np.arange(rv_sel.size, dtype=np.int32)
            # (out of place; the dry batch stays alive beside `ir` until the call returns, as the noise of add= does)
            dry, out = out, self.ctx.reverb_windows(out, valid, ir.view(rv_sel.size, rv_taps), ir_len.numpy(), index, _LAYOUTS[layout],
                                                    keep_power=reverb.keep_power, method=reverb.method)
        mixing = ch > 0 and any(sel.size > 0 for _, sel in add_plans)
        listed, S = not isinstance(add, Add), len(adds)
        # the gains: clx_add_windows and clx_addn_windows write every one of them when they run, so they need no fill then -- a fill
        # would run on torch's stream, unordered against the context's own stream that the launches go to when torch's current
        # stream is the default one
        gains = None if not return_gains else (torch.empty if mixing else torch.zeros)((B, S) if listed and S else B, dtype=torch.float32, device=dev)
        if mixing and not listed and add.plain:
            add_src, add_sel = add_plans[0]
            noise, noise_valid = add_src.read(add.stream_ids[add_sel], add.starts[add_sel], length, layout, sample_rate=sample_rate, channels=channels)
            index = np.full(B, -1, dtype=np.int32)
            index[add_sel] = np.arange(add_sel.size, dtype=np.int32)
            self.ctx.add_windows(out, valid, noise, noise_valid.numpy(), index, add.snr_db, _LAYOUTS[layout], gains=gains)
        elif mixing:
            # one noise read per distinct source, the windows of the Adds that share it stacked in list order; then S terms a window
            # in list order (an Add whose stream id is -1 there gives a term that adds nothing), all in one clx_addn_windows call
            sources, noises, noise_valids = [], [], []
            batch, index = np.zeros((B, S), dtype=np.int32), np.full((B, S), -1, dtype=np.int32)
            for s_, (src, sel) in enumerate(add_plans):
                if sel.size and not any(src is o for o in sources):      # (a source none of whose Adds names a stream is not read)
                    sources.append(src)
            for b, src in enumerate(sources):
                mine = [s_ for s_, (o, _) in enumerate(add_plans) if o is src]
                ids = np.concatenate([adds[s_].stream_ids[add_plans[s_][1]] for s_ in mine])
                sts = np.concatenate([adds[s_].starts[add_plans[s_][1]] for s_ in mine])
                at = 0
                for s_ in mine:
                    sel = add_plans[s_][1]
                    batch[:, s_] = b
                    index[sel, s_] = at + np.arange(sel.size, dtype=np.int32)
                    at += sel.size
                noise, noise_valid = src.read(ids, sts, length, layout, sample_rate=sample_rate, channels=channels)
                noises.append(noise)
                noise_valids.append(noise_valid.numpy())
            offset = np.stack([np.minimum(a.offsets, length) for a in adds], axis=1)     # (at or behind the window's end: an empty cover)
            loop = np.stack([a.tile for a in adds], axis=1)
            snr = np.stack([a.snr_db for a in adds], axis=1)
            self.ctx.addn_windows(out, valid, noises, np.concatenate(noise_valids), np.arange(B + 1, dtype=np.int64) * S, batch.reshape(-1),
                                  index.reshape(-1), offset.reshape(-1), loop.reshape(-1), snr.reshape(-1), _LAYOUTS[layout], gains=gains)
        if normalize is not None and ch > 0:
            self.ctx.norm_windows(out, valid, _LAYOUTS[layout], normalize)
        return (out, torch.from_numpy(valid)) + ((gains,) if return_gains else ())


    def read_mel(self, stream_ids, starts, n_frames, spec, layout="ct", length=None, normalize=None, add=None, reverb=None, augment=None, splice=None, cmvn=None, vad=None, return_vad=False, stats=None, groups=None):
        """A batch of feature windows: for window k, n_frames frames of `spec` (a MelSpec of this set's context) over the samples from
        starts[k] on of stream stream_ids[k], counted at spec.sample_rate and brought to one channel.  Exactly
        read(stream_ids, starts, L, "ct", sample_rate=spec.sample_rate, channels=1) -- its refusals, its frames decoded -- followed by
        one clx_mel_windows call on that [B, L] batch, with L = spec.window_len(n_frames): (n_frames - 1) * hop + n_fft, and for a
        centred spec `length` or n_frames * hop (the crop the frames are centred on and reflected at; it must be longer than
        n_fft // 2 and hold the frames: (n_frames - 1) * hop + n_fft <= length + 2 * (n_fft // 2)).  For an uncentred spec `length`
        must be None or that L -- unless the spec is reflected (MelSpec.kaldi_reflected, MelSpec.mfcc_reflected, reflect_edges=True):
        then L is `length`, any whole number from 0 up, or n_frames * hop.  A reflected spec's frames are reflected about the crop
        [starts[k], starts[k] + valid[k]), valid[k] being the part of the L samples inside the stream, and never reach the stream's
        samples outside it.  Kaldi's snip_edges=false features of a whole utterance of T samples therefore need starts[k] = 0,
        n_frames >= (T + hop // 2) // hop and length >= T: the default length n_frames * hop can be shorter than T, and the crop would
        then be cut there and reflected early.  Returns (float32 tensor on the context's GPU: [B, n_out, n_frames] for layout "ct",
        [B, n_frames, n_out] for "tc", n_out = spec.n_out: n_mels, or n_ceps of a cepstral spec; valid_frames): valid_frames[k] (int64 tensor) = spec.valid_frames(valid[k], n_frames) with
        valid[k] the window's samples inside its stream; a frame from there on is zeros, whatever the mode -- the scaled silence value
        for a spec with top.  The launches are queued behind read()'s, on the stream read() uses (gather_windows has the rule).

        With normalize=Norm(...) the features are then normalised per output row over the window's valid_frames[k] frames, in either
        layout (utterance CMVN): one clx_norm_windows call behind the spec's own steps, a ranged spec's range step included; the
        frames from valid_frames[k] on become the Norm's pad.  ValueError for a normalize that is not a Norm.

        With add=Add(...) the Add goes to that read() (starts counted at spec.sample_rate, every noise stream brought to one
        channel): the features are those of the noisy waveform, for every spec -- a centred or reflected spec reflects the noisy
        crop.  valid and valid_frames are the signal's.  add= takes what read()'s takes: one Add, also with offsets= or tile=, or a
        list of 1..16 of them (one clx_addn_windows call; offsets counted at spec.sample_rate).

        With reverb=Reverb(...) the Reverb goes to that read() too (starts and taps counted at spec.sample_rate), in front of the
        Add: the features are those of the reverberant, then noisy, waveform.

        With augment=SpecAugment(...) or a SpecAugmentPlan the features are then warped in time and masked (SpecAugment): one
        clx_specaug_windows call, the last step -- behind the spec's own launches, a ranged spec's range step and normalize=, so
        that a CMVN batch masked with fill=0.0 is masked with its mean.  A policy is drawn from the call's valid_frames and
        n_out rows (SpecAugment.draw); a plan must have B windows, warps that are (0, 0) or within 1 .. valid_frames[k] - 1, and
        every mask of a width above 0 must start below n_out rows or n_frames frames (a width of 0 masks nothing wherever it starts;
        a mask that runs past the end is clipped): ValueError otherwise, and for an augment that is neither.  The step is out of
        place: the tensor returned is a second one, and the one it was made from is released when the call returns, like read()'s
        scratch.  As with every launch here, on torch's default stream the work goes to the context's own stream, which torch's
        stream is not ordered against: wait (torch.cuda.synchronize()) before the next torch operation on the device.
        valid_frames does not change, and the frames behind them keep what they held.  augment=None is the call without the argument.

        With splice=Splice(...) the features are spliced along time (Kaldi's add-deltas, splice-feats and subsample-feats, FunASR's
        low-frame-rate stacking): one clx_splice_windows call behind the spec's own launches, a ranged spec's range step included,
        and in front of normalize= and augment=, which then see splice.n_out(n_out) rows, splice.frames_out(n_frames) frames and
        valid_frames' = splice.frames_out(valid_frames) -- FunASR's order: stacking, then CMVN, then masking.  The tensor returned
        is [B, splice.n_out(n_out), splice.frames_out(n_frames)] ("ct") or the same transposed ("tc"), with valid_frames'; the
        frames behind them are splice.pad unless a later step says otherwise.  A later step that refuses the row count raises its
        own error: normalize= and augment= take 256 rows at most, so not the 560 of seven stacked 80-band frames; cmvn= takes up
        to 8192 and is the route for more.  The step is out of place and the tensor it was made from is released on return, like
        read()'s scratch.  Whoever wants CMVN in front of the deltas calls read_mel(normalize=) or read_mel(cmvn=) and then
        Context.splice_windows.  splice=None is the call without the argument.

        With cmvn=Cmvn... the features are normalised by statistics that are not the window's own: a global Cmvn (a fixed shift and
        scale per row from a stats file: WeNet's global_cmvn, FunASR's am.mvn behind Splice.lfr()) by one clx_cmvn_global_windows
        call in place, a sliding one (Kaldi's apply-cmvn-sliding; Cmvn.xvector() over MelSpec.mfcc is the x-vector front end) by one
        clx_cmvn_sliding_windows call.  Either runs behind splice= and in front of augment=, over valid_frames' frames, and sets
        the frames behind them to cmvn.pad; valid_frames and the shape do not change.  A global Cmvn's rows must be the call's row
        count behind splice= (ValueError otherwise).  cmvn= and normalize= exclude each other (ValueError): one normaliser a call.
        The sliding step is out of place and the tensor it was made from is released on return, like splice='s.  cmvn=None is the
        call without the argument.

        With vad=Vad(...) the frames are judged voiced or not by Kaldi's energy VAD (compute-vad; Vad.voxceleb() over MelSpec.mfcc
        with cmvn=Cmvn.xvector() is the x-vector front end): one clx_vad_windows call over row vad.row of the batch as it stands
        behind splice= and IN FRONT OF normalize= / cmvn= -- Kaldi computes the VAD on the raw MFCCs -- over valid_frames' frames.
        With vad.select (the default) the voiced frames alone are then kept, moved to the front (select-voiced-frames): one
        clx_select_windows call BEHIND normalize= / cmvn= -- apply-cmvn-sliding runs over all frames, then the selection -- and
        in front of augment=.  The tensor returned is the selected one, of the same shape: its valid_frames are the numbers of
        voiced frames (0 for a window without one: Kaldi skips such an utterance, here it is all pad), the frames behind them are
        vad.pad, augment= draws its plan from those counts, and the tensor it was made from is released on return.  THE CALL THEN
        WAITS for the device once, for B words (the counts): the one step of read_mel whose result the host needs.  With
        select=False the features and valid_frames are untouched and nothing waits.  return_vad=True appends the mask (uint8
        [B, n_frames] on the GPU) to the return value: its time axis is the one before the selection, and its bytes from
        valid_frames on are 0.  ValueError for a vad that is not a Vad, a vad.row that is not below the row count behind splice=,
        and return_vad=True without vad=.  vad=None is the call without the argument.

        With stats=CmvnStats the batch is also ADDED to that accumulator (compute-cmvn-stats): one clx_cmvn_stats_windows call
        exactly where cmvn= would read the batch -- behind splice= and the VAD decision, in front of normalize= / cmvn=, over
        valid_frames' frames and before any selection.  The tensors returned do not change, and nothing waits: a whole corpus
        pass can be queued and stats.numpy() asked at the end.  groups= is B whole numbers, window k's group (speaker) in
        0..groups - 1 or -1 for a window that takes no part: shared by stats= and a grouped cmvn= (Cmvn.grouped(other_stats):
        apply-cmvn --utt2spk).  ValueError for a stats that is not an open CmvnStats of the set's context, rows that are not the
        call's row count behind splice=, groups of the wrong length or range, groups= with neither consumer, a grouped cmvn=
        without groups= when its stats have more than one group, and stats= being the object the call's grouped cmvn= reads:
        accumulate in one pass, apply in the next.  stats=None, groups=None is the call without the arguments."""
        if normalize is not None and not isinstance(normalize, Norm):
            raise ValueError("read_mel: normalize must be a Norm or None, not %r" % (normalize,))
        if augment is not None and not isinstance(augment, (SpecAugment, SpecAugmentPlan)):
            raise ValueError("read_mel: augment must be a SpecAugment, a SpecAugmentPlan or None, not %r" % (augment,))
        if splice is not None and not isinstance(splice, Splice):
            raise ValueError("read_mel: splice must be a Splice or None, not %r" % (splice,))
        if cmvn is not None and not isinstance(cmvn, Cmvn):
            raise ValueError("read_mel: cmvn must be a Cmvn or None, not %r" % (cmvn,))
        if cmvn is not None and normalize is not None:
            raise ValueError("read_mel: cmvn and normalize exclude each other: one normaliser a call")
        if vad is not None and not isinstance(vad, Vad):
            raise ValueError("read_mel: vad must be a Vad or None, not %r" % (vad,))
        if return_vad and vad is None:
            raise ValueError("read_mel: return_vad=True needs vad=")
        _adds_of(add, "read_mel")
        if reverb is not None and not isinstance(reverb, Reverb):
            raise ValueError("read_mel: reverb must be a Reverb or None, not %r" % (reverb,))
        if stats is not None and (not isinstance(stats, CmvnStats) or stats._acc is None or stats.ctx is not self.ctx):
            raise ValueError("read_mel: stats must be an open CmvnStats of the set's context or None, not %r" % (stats,))
        cmvn_stats = cmvn._stats if cmvn is not None else None
        if cmvn_stats is not None and cmvn_stats._acc is None:
            raise ValueError("read_mel: the grouped Cmvn's CmvnStats is closed")
        if groups is not None and stats is None and cmvn_stats is None:
            raise ValueError("read_mel: groups= needs stats= or a grouped cmvn=")
        if stats is not None and stats is cmvn_stats:
            raise ValueError("read_mel: stats= is the CmvnStats the grouped cmvn= reads: accumulate in one pass, apply in the next")
        if groups is None and cmvn_stats is not None and cmvn_stats.groups > 1:
            raise ValueError("read_mel: the grouped Cmvn's CmvnStats has %d groups: give groups=" % cmvn_stats.groups)
        import torch
        if layout not in _LAYOUTS:
            raise ValueError("read_mel: layout must be 'tc' or 'ct', not %r" % (layout,))
        if not isinstance(spec, MelSpec) or spec._h is None or spec.ctx is not self.ctx:
            raise ValueError("read_mel: spec must be an open MelSpec of the set's context")
        if stats is not None and stats.rows != (spec.n_out if splice is None else splice.n_out(spec.n_out)):
            raise ValueError("read_mel: the CmvnStats has %d rows, the features %d" % (stats.rows, spec.n_out if splice is None else splice.n_out(spec.n_out)))
        if groups is not None:
            for who in (stats, cmvn_stats):
                if who is not None:
                    _cmvn_groups("read_mel", groups, int(np.asarray(stream_ids).size), who.groups)
        if cmvn is not None and cmvn.rows is not None and cmvn.rows != (spec.n_out if splice is None else splice.n_out(spec.n_out)):
            raise ValueError("read_mel: the Cmvn has %d rows, the features %d" % (cmvn.rows, spec.n_out if splice is None else splice.n_out(spec.n_out)))
        if vad is not None and vad.row >= (spec.n_out if splice is None else splice.n_out(spec.n_out)):
            raise ValueError("read_mel: the Vad reads row %d, the features have %d" % (vad.row, spec.n_out if splice is None else splice.n_out(spec.n_out)))
        if isinstance(n_frames, bool) or int(n_frames) != n_frames or int(n_frames) < 0:
            raise ValueError("read_mel: n_frames must be a whole number, not negative")
        n_frames = int(n_frames)
        L = spec.window_len(n_frames)
        if length is not None:
            if isinstance(length, bool) or int(length) != length or int(length) < 0:
                raise ValueError("read_mel: length must be a whole number, not negative")
            if not spec.center and not spec.reflect_edges and int(length) != L:
                raise ValueError("read_mel: length must be None or %d ((n_frames - 1) * hop + n_fft) for a spec that is not centred, not %r" % (L, length))
            L = int(length)
        if spec.center and n_frames > 0:
            P = spec.n_fft // 2
            if P >= L:
                raise ValueError("read_mel: a centred spec needs length greater than n_fft // 2 = %d, not %d" % (P, L))
            if (n_frames - 1) * spec.hop + spec.n_fft > L + 2 * P:
                raise ValueError("read_mel: length %d holds %d centred frames, not %d" % (L, 1 + (L + 2 * P - spec.n_fft) // spec.hop, n_frames))
        audio, valid = self.read(stream_ids, starts, L, "ct", sample_rate=spec.sample_rate, channels=1, add=add, reverb=reverb)
        B = int(audio.shape[0])
        out = torch.empty((B, spec.n_out, n_frames) if layout == "ct" else (B, n_frames, spec.n_out), dtype=torch.float32,
                          device=audio.device)
        valid = valid.numpy()
        self.ctx.mel_windows(spec, audio.view(B, L), valid, n_frames, _LAYOUTS[layout], out)
        vf = spec.valid_frames(valid, n_frames)
        rows = spec.n_out
        if splice is not None:
            out = self.ctx.splice_windows(out, vf, _LAYOUTS[layout], splice)
            rows, n_frames, vf = splice.n_out(rows), splice.frames_out(n_frames), splice.frames_out(vf)
        mask = None
        if vad is not None:                                  # (queued in front of the normaliser, which may work in place)
            mask = self.ctx.vad_windows(out, vf, _LAYOUTS[layout], vad)
        if stats is not None:                                # (where cmvn= reads the batch; nothing of it is written)
            stats.accumulate(out, vf, _LAYOUTS[layout], groups)
        if normalize is not None:
            self.ctx.norm_windows(out, vf, _LAYOUTS[layout], normalize)
        if cmvn is not None:
            out = self.ctx.cmvn_windows(out, vf, _LAYOUTS[layout], cmvn, groups=groups if cmvn_stats is not None else None)
        if vad is not None and vad.select:
            out, vf = self.ctx.select_windows(out, vf, mask, _LAYOUTS[layout], vad.pad)
        if augment is not None:
            plan = augment.draw(vf, rows) if isinstance(augment, SpecAugment) else augment
            _specaug_fit(plan, vf, rows, n_frames, "read_mel")
            if B and n_frames:
                out = self.ctx.specaug_windows(out, vf, _LAYOUTS[layout], plan.warp, plan.freq_masks, plan.time_masks, plan.fill)
        return (out, torch.from_numpy(vf)) + ((mask,) if return_vad else ())


def open_streams(ctx, streams):
    """Whole FLAC streams (bytes-like) made resident for StreamSet.read: one arena, uploaded once and indexed with one
    Context.index_streams pass; the arena and the per-stream frame index stay alive in the returned StreamSet.  Like verify() it never
    raises for a bad stream: StreamSet.problems[k] holds the ClaxonError of a stream with a header error, an index that stops short of
    the stream's end, frames that differ in channel count or a frame header without bits per sample."""
    return StreamSet(ctx, streams)
