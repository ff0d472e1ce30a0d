/*
 * claxon_hip.h -- C ABI of the MI355X (gfx950) batched FLAC frame decoder.
 *
 * This is the drop-in boundary for ONE path of ruuda/claxon: per-subframe
 * decode (src/subframe.rs) plus stereo decorrelation (src/frame.rs), executed
 * for a whole batch of independent frames by hand-written HIP kernels.
 * Every entry point below names the reference interface it replaces
 * (file:line into the claxon v0.4.3 tree).  Plain pointers and sizes only;
 * no exceptions, panics or C++/torch types cross this boundary.
 *
 * Threading: a clx_ctx / clx_batch is NOT thread safe (the reference takes
 * `&mut self` everywhere, frame.rs:667); distinct contexts (one per GPU / per
 * HIP stream) may be used concurrently.
 *
 * Memory: "device" pointers are HIP device pointers on the context's GPU.
 * A device arena must be 16-byte aligned and its ALLOCATION must cover
 * arena_len + 16 bytes rounded up to a multiple of 16 (the kernels read the
 * bitstream in aligned 8/16-byte granules; bytes past arena_len are never
 * interpreted).
 */
#ifndef CLAXON_HIP_H
#define CLAXON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLX_VERSION_MAJOR 0
#define CLX_VERSION_MINOR 2
#define CLX_VERSION_PATCH 0

/* ------------------------------------------------------------------------
 * Error convention.  Replaces `claxon::Error` (error.rs:18-32):
 *   IoError(io::Error) | FormatError(&'static str) | Unsupported(&'static str)
 * Equality in the reference is variant + string (error.rs:34-45) and its tests
 * compare strings (tests/testsamples.rs:412), so the strings are API: each
 * clx_msg maps 1:1 to the reference's message (clx_message()).
 * ---------------------------------------------------------------------- */
typedef enum clx_status {
    CLX_OK          = 0,
    CLX_IO_ERROR    = 1,  /* Error::IoError(UnexpectedEof): bits ran out mid-frame (input.rs:139-142, 242) */
    CLX_FORMAT_ERROR= 2,  /* Error::FormatError(msg) */
    CLX_UNSUPPORTED = 3,  /* Error::Unsupported(msg) */
    CLX_END_OF_STREAM = 4,/* Ok(None): EOF before the two sync bytes (frame.rs:140-143) */
    CLX_API_ERROR   = 5   /* bad argument / HIP failure; no reference analogue */
} clx_status;

typedef enum clx_msg {
    CLX_MSG_NONE = 0,
    CLX_MSG_UNEXPECTED_EOF,              /* io::ErrorKind::UnexpectedEof */
    /* subframe.rs */
    CLX_MSG_SUBFRAME_HEADER_INVALID,     /* subframe.rs:32  */
    CLX_MSG_SUBFRAME_HEADER_RESERVED,    /* subframe.rs:47,55 */
    CLX_MSG_WASTED_BITS_EXCEED_31,       /* subframe.rs:83  */
    CLX_MSG_NO_NON_WASTED_BITS,          /* subframe.rs:199 */
    CLX_MSG_RESIDUAL_RESERVED,           /* subframe.rs:245 */
    CLX_MSG_INVALID_PARTITION_ORDER,     /* subframe.rs:263 */
    CLX_MSG_INVALID_RESIDUAL,            /* subframe.rs:276 */
    CLX_MSG_FIXED_ORDER_GT_BLOCK,        /* subframe.rs:500 */
    CLX_MSG_LPC_ORDER_GT_BLOCK,          /* subframe.rs:663 */
    CLX_MSG_QLP_PRECISION_INVALID,       /* subframe.rs:674 */
    CLX_MSG_UNENCODED_BINARY,            /* subframe.rs:318,366 (Unsupported) */
    CLX_MSG_NEGATIVE_QLP_SHIFT,          /* subframe.rs:688-690 (Unsupported) */
    /* frame.rs */
    CLX_MSG_FRAME_CRC_MISMATCH,          /* frame.rs:761 */
    CLX_MSG_FRAME_HEADER_CRC_MISMATCH,   /* frame.rs:300 */
    CLX_MSG_FRAME_SYNC_MISSING,          /* frame.rs:148 */
    CLX_MSG_FRAME_HEADER_RESERVED,       /* frame.rs:157,177,224,236,241 */
    CLX_MSG_FRAME_HEADER_INVALID,        /* frame.rs:210 */
    CLX_MSG_FRAME_NUMBER_TOO_LARGE,      /* frame.rs:255 */
    CLX_MSG_BLOCK_SIZE_EXCEEDS_65535,    /* frame.rs:273 */
    CLX_MSG_INVALID_VARINT,              /* frame.rs:82,98 */
    CLX_MSG_NO_BPS_IN_HEADER,            /* frame.rs:691 (Unsupported) */
    /* lib.rs / metadata.rs (stream open; host only) */
    CLX_MSG_INVALID_STREAM_HEADER,       /* lib.rs:200 */
    CLX_MSG_ID3_HEADER,                  /* lib.rs:198 */
    CLX_MSG_STREAMINFO_MISSING,          /* lib.rs:247 */
    CLX_MSG_SECOND_STREAMINFO,           /* lib.rs:268 */
    CLX_MSG_STREAMINFO_LENGTH,           /* metadata.rs:272 */
    CLX_MSG_INVALID_METADATA_BLOCK_TYPE, /* metadata.rs:305 */
    CLX_MSG_MIN_BLOCK_GT_MAX_BLOCK,      /* metadata.rs:361 */
    CLX_MSG_BLOCK_SIZE_LT_16,            /* metadata.rs:364 */
    CLX_MSG_MIN_FRAME_GT_MAX_FRAME,      /* metadata.rs:367 */
    CLX_MSG_INVALID_SAMPLE_RATE,         /* metadata.rs:373 */
    CLX_MSG_APPLICATION_BLOCK_TOO_SHORT, /* metadata.rs:527 */
    CLX_MSG_APPLICATION_BLOCK_TOO_LARGE, /* metadata.rs:534 (Unsupported) */
    /* VORBIS_COMMENT (FLAC tags), metadata.rs:402-513 */
    CLX_MSG_VC_TOO_SHORT,                /* metadata.rs:406 */
    CLX_MSG_VC_TOO_LARGE,                /* metadata.rs:423 (Unsupported) */
    CLX_MSG_VC_VENDOR_TOO_LONG,          /* metadata.rs:431 */
    CLX_MSG_VC_TOO_MANY_ENTRIES,         /* metadata.rs:448 */
    CLX_MSG_VC_COMMENT_TOO_LONG,         /* metadata.rs:462 */
    CLX_MSG_VC_NAME_INVALID_BYTE,        /* metadata.rs:491 */
    CLX_MSG_VC_NO_EQUALS,                /* metadata.rs:498 */
    CLX_MSG_VC_EXCESS_DATA,              /* metadata.rs:503 */
    CLX_MSG_VC_WRONG_COUNT,              /* metadata.rs:507 */
    CLX_MSG_VC_NOT_UTF8,                 /* error.rs:92 */
    CLX_MSG_SECOND_VORBIS_COMMENT,       /* lib.rs:258 */
    CLX_MSG_COUNT
} clx_msg;

/* The reference's exact message string for `msg` ("" for CLX_MSG_NONE). */
const char* clx_message(uint32_t msg);
/* The status (error variant) the reference attaches to `msg`. */
int clx_message_status(uint32_t msg);
/* (major<<16)|(minor<<8)|patch */
uint32_t clx_version(void);

/* ------------------------------------------------------------------------
 * Frame headers (host).  Replaces `read_frame_header_or_eof` (frame.rs:131-316)
 * and `read_var_length_int` (frame.rs:64-105), incl. the CRC-8 check
 * (crc.rs:62-93) -- byte-aligned, ~6-16 bytes per frame, not accelerated.
 * ---------------------------------------------------------------------- */
enum { CLX_CH_INDEPENDENT = 0, CLX_CH_LEFT_SIDE = 1, CLX_CH_RIGHT_SIDE = 2, CLX_CH_MID_SIDE = 3 };

typedef struct clx_frame_header {
    uint64_t time;               /* first sample number: block_size*frame_number or sample number (frame.rs:771-774) */
    uint32_t sample_rate;        /* 0 = "get from streaminfo" (frame.rs:193) */
    uint32_t frame_or_sample_lo; /* low 32 bits of the coded number */
    uint16_t block_size;
    uint16_t header_bytes;       /* bytes consumed incl. the CRC-8 */
    uint8_t  n_channels;
    uint8_t  channel_assignment; /* CLX_CH_* */
    uint8_t  bps;                /* 0 = "get from streaminfo" -> Unsupported at decode (frame.rs:687-692) */
    uint8_t  variable_blocking;
} clx_frame_header;

/* Parse one frame header from `p[0..avail)`.  Returns a clx_status; on error
 * *msg holds the clx_msg.  CLX_END_OF_STREAM iff fewer than 2 bytes are
 * available (frame.rs:140-143).  `check_crc`=0 mirrors cfg(fuzzing). */
int clx_parse_frame_header(const uint8_t* p, size_t avail, int check_crc,
                           clx_frame_header* out, uint32_t* msg);

/* CRC helpers (crc.rs:89-113): CRC-8 poly 0x07, CRC-16 poly 0x8005, init 0, MSB first. */
uint8_t  clx_crc8(const uint8_t* p, size_t n);
uint16_t clx_crc16(const uint8_t* p, size_t n);

/* ------------------------------------------------------------------------
 * Batch decode (device).  Replaces, for n frames at once, the body of
 * `FrameReader::read_next_or_eof` between header parse and footer
 * (frame.rs:699-750): `subframe::decode` per channel on one bit cursor
 * (subframe.rs:184-228, called from frame.rs:708,715,716,725,726,734,735)
 * and `decode_left_side/right_side/mid_side` (frame.rs:319-389).
 * ---------------------------------------------------------------------- */
typedef struct clx_frame_desc {
    uint64_t byte_off;      /* frame start (sync code) in the arena */
    uint32_t max_bytes;     /* bytes readable from byte_off (rest of stream, or packet length) */
    uint16_t header_bytes;  /* first subframe starts at byte_off+header_bytes, bit 0 */
    uint16_t block_size;    /* 1..65535 */
    uint8_t  n_channels;    /* 1..8 */
    uint8_t  channel_assignment; /* CLX_CH_* */
    uint8_t  bps;           /* header bps (side channels decode at bps+1 on device) */
    uint8_t  reserved[5];
} clx_frame_desc;           /* 24 bytes */

typedef struct clx_frame_result {
    int32_t  status;        /* clx_status */
    uint32_t msg;           /* clx_msg */
    uint64_t end_bit;       /* bit offset (from byte_off) just past the last subframe;
                               the CRC-16 sits at byte ceil(end_bit/8) (frame.rs:744-754) */
} clx_frame_result;         /* 16 bytes */

typedef struct clx_ctx   clx_ctx;
typedef struct clx_batch clx_batch;

/* Create a context bound to HIP device `device`.  Fails (CLX_API_ERROR) when no
 * gfx950 device / HIP runtime is usable: there is NO CPU fallback. */
int  clx_create(int device, clx_ctx** out);
void clx_destroy(clx_ctx* ctx);
/* Human-readable text of the last CLX_API_ERROR on this context. */
const char* clx_last_error(const clx_ctx* ctx);

/* Flags for clx_decode_frames */
enum {
    CLX_ARENA_ON_DEVICE = 1u << 0,   /* arena is a device pointer (else host; copied H2D) */
    CLX_OUT_ON_DEVICE   = 1u << 1,   /* out is a device pointer (else host; copied D2H)   */
    CLX_VERIFY_CRC16    = 1u << 2,   /* also verify each frame's CRC-16 footer on device
                                        (frame.rs:752-763); mismatch -> CLX_MSG_FRAME_CRC_MISMATCH.
                                        Without it the footer is still read, as the reference does
                                        under cfg(fuzzing) (frame.rs:754): a frame whose two footer
                                        bytes lie beyond max_bytes fails with CLX_MSG_UNEXPECTED_EOF */
    /* Kernel path.  Default (neither bit): chosen from the batch shape.
     * WAVES: one wavefront per frame, wave-parallel Rice decode (lowest latency for a few frames).
     * LANES: one lane per subframe, lane-serial fused decode (highest throughput for many frames;
     *        needs arena_len < 4 GiB: an explicit CLX_PATH_LANES fails beyond, the default falls back to WAVES). */
    CLX_PATH_WAVES      = 1u << 3,
    CLX_PATH_LANES      = 1u << 4,
    CLX_PCM_ON_DEVICE   = 1u << 5,   /* clx_interleave: `pcm` is a device pointer (else host; copied D2H) */
    /* Build of the lane path's decode kernel (with CLX_PATH_LANES; default: by batch size): the fused one-wave
     * kernel (throughput), or the two-wave split kernel (latency). */
    CLX_LANES_FUSED     = 1u << 6,
    CLX_LANES_SPLIT     = 1u << 7,
    /* Build of the wave path's predictor kernel (default: by batch size): the multi-wave latency build
     * (clx_k_predict) or the one-wave throughput build (clx_k_predict_1w / _1w_hi). */
    CLX_K2_LATENCY      = 1u << 8,
    CLX_K2_THROUGHPUT   = 1u << 9,
    /* The fused lane build runs clx_k_lean first (the 16-bit tier: waves of <= 16-bit FIXED / LPC subframes of at most 12 taps in
     * aligned rows), then clx_k_lean24 (the split tier: <= 24 bits, <= 32 taps) when the batch holds frames of more than 16 bits,
     * and the general kernels on the groups those leave.  This flag leaves the tiers out: every group goes through the general
     * kernels (test and comparison target). */
    CLX_LANES_GENERAL   = 1u << 10,
    /* Waves composed by content (fused lane build; round 4).  A wave of 64 subframes runs the predictor build of its HIGHEST order,
     * the masked form of its turns when ONE lane holds a constant or verbatim subframe, the generic stereo form unless ALL its
     * pairs are mid/side -- so behind the scan a small kernel (clx_k_compose) re-deals the frames of a window (up to 16 384 stereo
     * frames of one block size) to the lanes by class: predictor order <= 4 / <= 8 / <= 12 / more, constant or verbatim subframes,
     * channel assignment.  Which frame a lane decodes changes, nothing else: every frame still goes to its own place in `out`.
     * Default: on for windows whose descriptors differ in their channel assignment (streams as encoders write them), off where
     * every descriptor is the same (synthetic batches of one shape).  These flags force it on / off. */
    CLX_COMPOSE         = 1u << 11,
    CLX_NO_COMPOSE      = 1u << 12,
    /* Narrow output straight from the decode (planned batches: clx_batch_create + clx_batch_run / clx_batch_submit; round 5).  The
     * batch's `d_out` buffers then hold channel-interleaved little-endian 16-bit PCM -- what lib.rs:473-520 (FlacSamples) walks and
     * examples/decode.rs:48-62 writes to a .wav -- instead of planar i32: `d_out` points to int16_t, indexed by the SAME sample
     * offsets (frame i's block starts at int16 index out_sample_offsets[i]; sample t of channel c at + t * n_channels + c), each
     * sample's low 16 bits as clx_batch_interleave(.., 2) gives them.  Every frame must have at most 16 bits per sample.  The
     * lean decode kernel writes a stereo frame's 32 samples as one 128-byte line from the tiles it stages anyway (half the bytes
     * through the write path), and a mono frame's as 64 bytes (round 6); whatever it leaves -- more channels, odd block sizes, waves that
     * give up -- the general kernels decode into staging rows of their workgroup's own and narrow row by row (one allocation per
     * internal stream, sized by what the descriptors say is left: round 5's planar scratch per run in flight is gone).  Failed frames'
     * bytes are unspecified, as the planar output's are.  Always the lane kernels, fused build. */
    CLX_OUT_PCM16       = 1u << 13,
    /* Pipelined submissions of the fused lane build, another launch form (round 6; off by default: measured slower, DESIGN.md
     * section 4.4): a merged launch's scan waves and 16-bit-tier decode waves as TICKETS taken off a counter by one grid of waves
     * that stay resident (clx_k_pool) instead of two kernels of one workgroup per wave (clx_k_scan, clx_k_lean).  Bit-exact like the
     * default.  (Batches whose waves are composed by content keep the two kernels anyway.) */
    CLX_POOL            = 1u << 14,
    /* The same as CLX_OUT_PCM16 with packed little-endian 24-bit samples (3 bytes each; round 6): `d_out` points to bytes, frame i's
     * block starts at byte 3 * out_sample_offsets[i], sample t of channel c at + 3 * (t * n_channels + c): what clx_batch_interleave(.., 3)
     * gives.  Every frame must have at most 24 bits per sample.  The split tier (clx_k_lean24, which takes the batch's 16-bit frames too
     * in this mode) writes a stereo frame's 32 sample pairs as twelve 16-byte pieces from the tiles it stages anyway (blocks that start on 16 bytes: out_sample_offsets[i] a multiple of 16); mono and
     * multi-channel frames, odd block sizes and waves that give up go through the general kernels' staging rows. */
    CLX_OUT_PCM24       = 1u << 15,
    /* Normalized float output straight from the decode (planned batches: clx_batch_create + clx_batch_run / clx_batch_submit): `d_out`
     * points to channel-interleaved IEEE float32, addressed as CLX_OUT_PCM16 with 4-byte samples -- frame i's block starts at float
     * index out_sample_offsets[i], sample t of channel c at + t * n_channels + c (lib.rs:473-520's order).  Sample v of a frame whose
     * header says `bps` bits becomes (float)v * 2^-(bps-1): round-to-nearest-even int -> float, then an exact power-of-two scale --
     * in numpy v.astype(np.float32) * np.float32(2.0 ** (1 - bps)).  For every valid stream (|v| < 2^23) the value is exact and lies
     * in [-1, 1), the convention of torchaudio and libsndfile; out-of-range values (runaway mid/side streams) convert by the same
     * formula, with no clamping.  Every frame width the decoder takes is allowed.  Excludes CLX_OUT_PCM16 / CLX_OUT_PCM24; refused
     * with CLX_PATH_WAVES / CLX_LANES_SPLIT / CLX_LANES_GENERAL; CLX_POOL is ignored.  The tiers (clx_k_lean_f32 for waves of
     * <= 16-bit stereo or mono frames, clx_k_lean24_f32 for stereo frames up to 24 bits and 16-bit ones of more than 12 taps) write
     * whole lines of floats from the tiles they stage, for blocks that start on 32 bytes (out_sample_offsets[i] a multiple of 8);
     * the rest -- more channels, odd block sizes, mono frames of more than 16 bits, waves that give up -- goes through the general
     * kernels' staging rows.  Failed frames' bytes are unspecified. */
    CLX_OUT_F32         = 1u << 16
};
/* Sample format for clx_interleave, clx_batch_interleave and clx_decode_frames_stream, next to sample_bytes 1..4: the floats of
 * CLX_OUT_F32, 4 bytes per sample, frame i at byte 4 * out_sample_offsets[i]. */
#define CLX_SAMPLE_F32 0x104u

/* One-shot convenience: plan + run + fetch results.  `out` is planar i32
 * (channel c of frame i at out[out_sample_offsets[i] + c*block_size ...),
 * frame.rs:409-410,477-481).  `results[i]` receives frame i's status. */
int clx_decode_frames(clx_ctx* ctx, const uint8_t* arena, size_t arena_len,
                      const clx_frame_desc* frames, size_t n,
                      int32_t* out, const uint64_t* out_sample_offsets,
                      clx_frame_result* results, uint32_t flags);

/* The same with several contexts -- one per GPU (or several on one GPU): the batch is cut into contiguous frame ranges of
 * near-equal algorithmic weight, context c decodes range c on a host thread of its own and receives only that range's slice
 * of the arena; nothing is exchanged between the devices (frames are independent: frame.rs:667-779 touches only its own bytes
 * and buffer; the reference's counterpart is one FrameReader per thread).  Host buffers only; frames in increasing,
 * non-overlapping output order (else the whole batch goes to ctxs[0]). */
int clx_decode_frames_multi(clx_ctx* const* ctxs, size_t n_ctx, const uint8_t* arena, size_t arena_len,
                            const clx_frame_desc* frames, size_t n, int32_t* out, const uint64_t* out_sample_offsets,
                            clx_frame_result* results, uint32_t flags);

/* Host-to-host decode as a pipeline (what a caller without device-resident data uses): the batch is cut into chunks of
 * frames; one chunk's compressed bytes travel to the device while the previous chunk is decoded and the one before that
 * returns its PCM.  Device buffers and plans live in the context and are reused from call to call.
 *   sample_bytes == 0: `out` is planar int32_t, as clx_decode_frames
 *   sample_bytes 1..4: `out` receives the narrow stage's channel-interleaved little-endian PCM (clx_batch_interleave), frame i
 *                      at byte out_sample_offsets[i] * sample_bytes -- what callers of the reference write out
 *                      (examples/decode.rs:48-62), half the bytes over the link for 16-bit audio
 *   out == NULL      : nothing is copied back but the results (decode throughput with the upload included)
 * Frames in increasing, non-overlapping output order; they may leave gaps.  `out` is written whole from the first frame's block to
 * the end of the last one's: samples of failed frames read as zeros, and so does every gap between two blocks (the chunks come back
 * as whole slices; a gap that falls between two chunks is cleared on the host, by the calling thread, so very large gaps cost host
 * time).  Nothing in front of the first block or behind the last one is written.  Buffers from clx_host_alloc
 * (pinned) make the copies asynchronous at link speed; any host memory works. */
int   clx_decode_frames_stream(clx_ctx* ctx, const uint8_t* arena, size_t arena_len, const clx_frame_desc* frames, size_t n,
                               void* out, uint32_t sample_bytes, const uint64_t* out_sample_offsets,
                               clx_frame_result* results, uint32_t flags);
/* Frames per chunk of clx_decode_frames_stream on this context; 0 (the default) = a third of the batch, 256 .. 8192: a chunk's
 * decode lasts at least as long as the predictor kernel's serial chain, so few large chunks beat many small ones. */
void  clx_set_stream_chunk(clx_ctx* ctx, size_t frames_per_chunk);
void* clx_host_alloc(size_t bytes);      /* pinned host memory (hipHostMalloc); NULL on failure */
void  clx_host_free(void* p);

/* One-shot interleave / narrow stage (see clx_batch_interleave).  `planar` follows CLX_OUT_ON_DEVICE, `pcm`
 * CLX_PCM_ON_DEVICE; `results` (may be NULL) marks frames to skip (status != CLX_OK). */
int clx_interleave(clx_ctx* ctx, const int32_t* planar, const clx_frame_desc* frames, size_t n,
                   const uint64_t* out_sample_offsets, const clx_frame_result* results,
                   void* pcm, uint32_t sample_bytes, uint32_t flags);

/* Config-2 entry: n independent byte-aligned SUBFRAMES (no frame header):
 * subframe i starts at arena[byte_offs[i]], decoded at bps[i] into
 * out[out_sample_offsets[i] .. +block_size[i]).  = `subframe::decode` (subframe.rs:184). */
int clx_decode_subframes(clx_ctx* ctx, const uint8_t* arena, size_t arena_len,
                         const uint64_t* byte_offs, const uint16_t* block_sizes,
                         const uint8_t* bps, size_t n,
                         int32_t* out, const uint64_t* out_sample_offsets,
                         clx_frame_result* results, uint32_t flags);

/* Planned batch: descriptors uploaded once, then run any number of times on
 * device-resident data (what bench.py times).  `stream` is a hipStream_t
 * (NULL = the context's own stream). */
int  clx_batch_create(clx_ctx* ctx, const clx_frame_desc* frames, size_t n,
                      const uint64_t* out_sample_offsets, uint32_t flags, clx_batch** out);
/* Where a planned batch writes (clx_batch_run, clx_batch_submit; every kernel path and every CLX_OUT_* mode; tests/placement_cases.py
 * holds the kernels to it, element by element):
 *   - Frame i's block is the n_channels * block_size elements (CLX_OUT_PCM24: three bytes each) from out_sample_offsets[i] on.  The
 *     blocks may lie anywhere in `d_out`, in any order, with gaps of any length between them and more than 4 GiB apart; they must not
 *     overlap.  All offsets are 64-bit.
 *   - `d_out` needs the alignment of its element type and no more: 4 bytes for planar int32_t and CLX_OUT_F32, 2 for CLX_OUT_PCM16,
 *     none for CLX_OUT_PCM24.
 *   - Nothing outside the blocks is written: not the bytes in front of the first block or behind the last, not a gap, not the tail of
 *     a 16-byte or 128-byte line a block ends in.  The buffer needs no slack behind its last block.  (Inside the block of a frame that
 *     FAILS the content is unspecified.)
 *   - Placement costs speed, never correctness.  The fast tiers take a wave of 64 subframes when every row of it starts on 16 ADDRESS
 *     bytes (CLX_OUT_F32: on 32) and lies within 4 GiB of the wave's lowest row; everything else goes through the general kernels,
 *     which store a row that is off 16 bytes sample by sample.  With `d_out` itself on 32 bytes (any device allocation) that means:
 *     planar, every out_sample_offsets[i] a multiple of 4 and block sizes a multiple of 16; CLX_OUT_PCM16 and CLX_OUT_F32, offsets a
 *     multiple of 8; CLX_OUT_PCM24, a multiple of 16.  The wave path's vector row stores want rows on 16 address bytes too (offsets
 *     and block sizes a multiple of 4); its kernels test the address, so a `d_out` that is off 16 bytes only takes the slower stores. */
int  clx_batch_run(clx_batch* b, const uint8_t* d_arena, size_t arena_len,
                   int32_t* d_out, void* stream);
/* Pipelined submission: the same work and the same results as clx_batch_run, with several submissions in flight (the reference
 * has no counterpart: one FrameReader decodes one frame at a time, frame.rs:667).  Which kernels a batch's submissions use is
 * chosen for throughput (clx_batch_submit_lanes):
 *   - usually the lane kernels, fused build.  One run of those is a serial chain per subframe on a fraction of the machine, and
 *     the machine runs only a handful of kernels from different queues side by side -- so consecutive submissions are MERGED:
 *     they wait until a few of them are there (or until somebody flushes / asks for results) and go out as ONE grid whose second
 *     dimension is the submission, on two internal streams in turn (the scan stage of one launch overlaps the decode stage of
 *     another).  Every submission has its own scratch buffers and results.  No environment variable is involved: two internal
 *     streams fit HIP's default number of hardware queues.
 *   - the wave kernels, four in flight on internal streams of their own: only when CLX_PATH_WAVES asks for them or the arena is
 *     4 GiB or more (the merged lane launches are ahead at every batch size measured).
 * A submission starts no earlier than everything queued on `stream` when it (or a later one merged with it) was submitted.  Give
 * the submissions in flight different `d_out` buffers, i.e. rotate over clx_batch_submit_depth(b) of them (re-using a buffer is
 * legal: the submission then goes out after the earlier one that writes it).  Submissions may stay pending until
 * clx_batch_flush: work enqueued on `stream` after it sees every submission finished; clx_batch_results and
 * clx_batch_interleave flush by themselves; clx_batch_results returns the LAST submission's results.
 * One batch, one caller stream at a time: a batch's submissions and runs come in on ONE `stream` until a clx_batch_flush /
 * clx_batch_results on that stream (submissions that arrive on another stream are not merged with pending ones, but what is
 * already in flight is ordered against the stream it came in on only; distinct batches and contexts are independent).
 * Output buffers are told apart by their BASE address: two submissions with the same `d_out` are ordered (the later one goes out
 * behind the earlier one), two whose buffers overlap but start at different addresses are NOT -- hand over buffers that are either
 * identical or disjoint.
 * Pending submissions are not forgotten: re-planning or destroying a batch launches what is still pending first.  A merged launch
 * that cannot be made (a HIP error) drops ITS submissions: the call that triggered the launch returns CLX_API_ERROR, and so does,
 * once, the next clx_batch_flush / clx_batch_results / clx_batch_interleave of the batch (clx_last_error says which).  A batch
 * that still holds pending submissions should be flushed or destroyed BEFORE its context: clx_batch_destroy then drains the device
 * instead of ordering the launch behind the (possibly gone) stream the submissions came in on. */
#ifndef CLX_SUBMIT_DEPTH
#define CLX_SUBMIT_DEPTH 24     /* the most submissions any batch keeps in flight */
#endif
int  clx_batch_submit(clx_batch* b, const uint8_t* d_arena, size_t arena_len,
                      int32_t* d_out, void* stream);
/* How many submissions THIS batch keeps in flight, i.e. how many output buffers to rotate over: 4 for the wave kernels, 24 for
 * the lane kernels (two merged launches of twelve), 1 where a submission is a plain run. */
int  clx_batch_submit_depth(const clx_batch* b);
int  clx_batch_submit_lanes(const clx_batch* b);      /* 1: its pipelined submissions run the fused lane kernels */
int  clx_batch_submit_merge(const clx_batch* b);      /* how many consecutive submissions go out as one launch (1: none are merged) */
int  clx_batch_flush(clx_batch* b, void* stream);
/* Blocks until the last run finished, then copies the per-frame results to host. */
int  clx_batch_results(clx_batch* b, clx_frame_result* results);
/* Interleave / narrow output stage on the planned frames (what callers of the reference do next: FlacSamples,
 * lib.rs:473-520; Block::stereo_samples -> i16 WAV, examples/decode.rs:48-62).  Frame i's planar samples
 * d_planar[off_i + c*bs + s] become little-endian two's-complement PCM of `sample_bytes` (1..4) bytes at byte
 * (off_i + s*channels + c) * sample_bytes of d_pcm -- channel-interleaved, the order the STREAMINFO MD5 is defined
 * over (metadata.rs:52-53).  Frames whose last run failed are skipped.  Async on `stream`, after clx_batch_run. */
int  clx_batch_interleave(clx_batch* b, const int32_t* d_planar, void* d_pcm, uint32_t sample_bytes, void* stream);
/* FLAC audio MD5 (the STREAMINFO signature, metadata.rs:52-53) of many streams in one launch, one GPU lane per stream.  d_samples
 * is a device buffer of channel-interleaved samples in `sample_format`: 1..4 (little-endian two's-complement PCM of that many bytes)
 * or CLX_SAMPLE_F32 (floats, scaled back exactly as v = f * 2^(bps-1)).  Stream k is the n_samples[k] samples from sample index
 * first_sample[k] on (byte first_sample[k] * width); each is hashed as its low ceil(bps[k] / 8) bytes, the FLAC rule, and the 16
 * bytes of its digest go to digests[16 * k] (host memory).  Which source each output holds:
 *   CLX_OUT_PCM16 -> 2, CLX_OUT_PCM24 -> 3, CLX_OUT_F32 -> CLX_SAMPLE_F32, clx_batch_interleave(.., sb) -> sb.
 * Planar i32 output has no source format: interleave it first.  No sample byte past a stream's last is read, at any alignment.
 * Queued on `stream` (NULL: the context's) after what is already there, e.g. a clx_batch_run; returns when the digests are in
 * host memory.  CLX_API_ERROR (clx_last_error says why) for a bad format, bps outside 1..32, ceil(bps / 8) wider than the
 * source's samples, CLX_SAMPLE_F32 with bps > 24, or a null pointer when n_streams > 0; n_streams == 0 succeeds.
 * One stream hashes at a single lane's rate: the device wins by the number of streams (README: measured rates). */
int  clx_md5_streams(clx_ctx* ctx, const void* d_samples, uint32_t sample_format, const uint64_t* first_sample,
                     const uint64_t* n_samples, const uint8_t* bps, size_t n_streams, uint8_t* digests, void* stream);
/* A dense batch of fixed-length sample windows gathered from decoded audio on the device, in one launch (clx_k_window).  d_src is a
 * device buffer of channel-interleaved float32, what CLX_OUT_F32 writes, `channels` (1..8) floats per sample.  Window k is the
 * valid[k] <= window_len samples per channel from float index src_first[k] on (the window's first sample, channel 0; no alignment
 * beyond 4 bytes).  d_out (device, n_windows * window_len * channels floats) gets
 *   CLX_WINDOW_TC: out[k][t][c] = d_src[src_first[k] + t*channels + c]        a [B, L, C] tensor
 *   CLX_WINDOW_CT: out[k][c][t] = the same value                              a [B, C, L] tensor (channels first)
 * and 0.0f for every t >= valid[k]: the call writes all of d_out, which need not be cleared.  No float of d_src outside
 * [src_first[k], src_first[k] + valid[k]*channels) is read.  All offsets are 64-bit.  src_first and valid are host arrays, copied
 * before the call returns into scratch that the context owns (grown, when it must, before anything is queued; released by
 * clx_destroy).  Asynchronous: queued on `stream` (NULL: the context's) after what is already there, e.g. the clx_batch_run that
 * decodes d_src; d_src and d_out stay valid until that stream has passed the call.  CLX_API_ERROR (clx_last_error says why) for
 * channels outside 1..8, an unknown layout, a valid[k] above window_len, or a null pointer while n_windows * window_len > 0;
 * n_windows == 0 or window_len == 0 succeeds and launches nothing. */
enum { CLX_WINDOW_TC = 0, CLX_WINDOW_CT = 1 };
int  clx_gather_windows(clx_ctx* ctx, const void* d_src, const uint64_t* src_first, const uint32_t* valid,
                        size_t n_windows, uint32_t window_len, uint32_t channels, uint32_t layout,
                        void* d_out, void* stream);
/* clx_gather_windows at a target sample rate: a dense batch of fixed-length windows of the audio resampled to `out_rate`, computed
 * while they are cut out of d_src, in one launch (clx_k_resample).  The resampler is fixed and has no tunables: band-limited
 * interpolation with a Hann-windowed sinc, filter width 6 and rolloff 0.99 (torchaudio.functional.resample's defaults).  For
 * fs = src_rate[k]: g = gcd(fs, out_rate), o = fs / g, n = out_rate / g, base = min(o, n) * 0.99, W = ceil(6 * o / base), and
 *   y[m] = sum over s of x[s] * h(s - m*o/n),   h(d) = sinc(t) * cos^2(pi*t/12) * base/o with t = d*base/o, 0 where |t| >= 6,
 * x = 0 outside the stream; only the 2W taps s = floor(m*o/n) - W + 1 + k, k = 0 .. 2W - 1, can be non-zero.  The coefficients are
 * computed in double, rounded once to float32 and kept on the context, one table per (o, n); the kernel accumulates in float32,
 * taps in ascending order.  d_src is channel-interleaved float32 as for clx_gather_windows.  Window k's source span is the src_n[k]
 * samples per channel from float index src_first[k] on, the first of them stream sample src_t0[k]; a tap outside
 * [src_t0[k], src_t0[k] + src_n[k]) counts as zero, and no float of d_src outside [src_first[k], src_first[k] + src_n[k]*channels)
 * is read.  The window is outputs out_t0[k] .. out_t0[k] + valid[k] - 1 of the resampled stream, then zeros up to window_len, laid
 * out as CLX_WINDOW_TC / CLX_WINDOW_CT: the call writes all of d_out.  Where src_rate[k] == out_rate the window is a plain copy
 * (output m is source sample m, bit for bit), not a pass through a filter; one call may mix rates and copies.  The host arrays are
 * copied before the call returns into scratch that the context owns (grown, when it must, before anything is queued; released by
 * clx_destroy).  Asynchronous on `stream` like clx_gather_windows, except that the first call with a new rate pair uploads its
 * table with a synchronous copy.  CLX_API_ERROR (clx_last_error says why) for a null pointer while n_windows * window_len > 0,
 * channels outside 1..8, an unknown layout, a valid[k] above window_len, a rate of 0 or >= 2^20 (the width of STREAMINFO's field),
 * a rate pair whose [n][2W] table would have more than 2^18 entries (44100 -> 16001), an out_t0[k] of 2^43 or more, or too many
 * windows for one grid; n_windows == 0 or window_len == 0 succeeds and launches nothing. */
int  clx_resample_windows(clx_ctx* ctx, const void* d_src, const uint64_t* src_first, const int64_t* src_t0, const uint32_t* src_n,
                          const uint64_t* out_t0, const uint32_t* valid, const uint32_t* src_rate, size_t n_windows,
                          uint32_t out_rate, uint32_t window_len, uint32_t channels, uint32_t layout, void* d_out, void* stream);
/* clx_resample_windows with every window brought to out_channels (K, 1..8) channels while it is cut, in one launch (clx_k_mix): one
 * dense [B, L, K] / [B, K, L] batch from streams that differ in channel count as well as in rate.  src_channels[k] (Cs, 1..8, a
 * host array) is the channel count of window k's source: its span is src_n[k] samples of Cs interleaved floats from float
 * src_first[k] on, and no float outside [src_first[k], src_first[k] + src_n[k]*Cs) is read.  One of three rules applies:
 *   identity   Cs == K       exactly what clx_gather_windows / clx_resample_windows give, bit for bit;
 *   reduce     K == 1 < Cs   the mean of the channels in float32, in this order: s = x[t][0]; s = s + x[t][1]; ...;
 *                            s = s + x[t][Cs-1], each add rounded to nearest, then s * r with r the float32 nearest to 1/Cs;
 *   replicate  Cs == 1 < K   the mono sample goes to each of the K channels.
 * Any other (Cs, K) is refused: there is no one downmix matrix everybody expects.  Where src_rate[k] == out_rate the window is
 * that mix of source samples out_t0[k] .. (identity and replicate move 32-bit words).  Otherwise the mix comes first and the
 * resampler of clx_resample_windows is applied to the mixed float32 signal: a tap outside the span counts as zero and none of its
 * Cs floats is loaded, the sum runs in float32, taps ascending, one fmaf each with the mixed value as the multiplicand; replicated
 * channels are bitwise equal.  The call writes all of d_out, +0.0 from valid[k] on.  Rate pairs and their tables are shared with
 * clx_resample_windows (a pair built by either call serves both), and so are the scratch, the stream rules and every refusal;
 * CLX_API_ERROR also for out_channels or a src_channels[k] outside 1..8 and for a (Cs, K) that no rule covers.  n_windows == 0 or
 * window_len == 0 succeeds and launches nothing. */
int  clx_mix_windows(clx_ctx* ctx, const void* d_src, const uint64_t* src_first, const int64_t* src_t0, const uint32_t* src_n,
                     const uint64_t* out_t0, const uint32_t* valid, const uint32_t* src_rate, const uint8_t* src_channels,
                     size_t n_windows, uint32_t out_rate, uint32_t window_len, uint32_t out_channels, uint32_t layout, void* d_out,
                     void* stream);
/* Mel filterbank features of a dense mono batch, in one launch (clx_k_mel).
 *
 * A spec is (n_fft N, hop H, a float32 window w[N], a float32 filterbank fb[n_mels][J], mode, floor) with N in 2..2048,
 * J = floor(N/2) + 1, H any whole number from 1 up (H > N is allowed) and n_mels in 1..256.  For a batch a[B][L] (float32) with
 * valid[k] <= L:
 *   frames     frame t of window k is x[n] = a[k][t*H + n], n = 0..N-1: no centring, no reflection.  The caller guarantees
 *              (n_frames-1)*H + N <= L (checked), and that the samples at or past valid[k] are zero (not checked and not
 *              re-masked: StreamSet.read and the window readers above write them as zero).
 *   basis      c[j][n] = fl32(w[n] * cos(2 pi ((j n) mod N) / N)), s[j][n] = fl32(-w[n] * sin(2 pi ((j n) mod N) / N)): built on
 *              the host in double, rounded once, once per spec, kept on the context.
 *   power      re_j = sum_n x[n] c[j][n], im_j = sum_n x[n] s[j][n], P_j = re_j^2 + im_j^2, M_m = sum_j fb[m][j] P_j, all in
 *              float32.  The order of the sums is the kernel's and it uses fused multiply-adds; for ANY order
 *              |M_m - exact| <= dM_m with, u = 2^-24 and g(k) = k u / (1 - k u): dre_j = g(N+2) sum_n |x[n] w[n] cos|, dim_j
 *              likewise, E_j = 2|re_j| dre_j + dre_j^2 + 2|im_j| dim_j + dim_j^2, dP_j = E_j + g(3)(P_j + E_j),
 *              dM_m = sum_j fb[m][j] dP_j + g(J_m + 1) sum_j fb[m][j](P_j + dP_j), J_m the row's bin count.
 *   rows       a filterbank row is summed only from its first to its last non-zero bin (the library finds them in the dense
 *              table); an all-zero row gives 0.
 *   mode       CLX_MEL_POWER: M_m.  CLX_MEL_LN: logf(max(M_m, floor)).  CLX_MEL_LOG10: log10f(max(M_m, floor)).  The modes
 *              differ in that last step only: M_m is bitwise the same in all three (and in both layouts).
 *   validity   valid_frames[k] = clamp(ceil(valid[k] / H), 0, n_frames).  A frame at or past it is written as +0.0 in every
 *              mode and its DFT is not computed.  The call writes all of d_out.
 *   layout     CLX_WINDOW_CT: out[k][m][t], a [B, n_mels, n_frames] tensor.  CLX_WINDOW_TC: out[k][t][m], [B, n_frames, n_mels]:
 *              the bands take the channels' place.
 * No float of d_audio outside [0, B*L) is read (none outside a frame below valid_frames[k], in fact).
 *
 * clx_mel_create checks the ranges, builds the basis, uploads it with the filterbank and the rows' ends (it synchronises) and
 * returns a handle owned by the context: clx_destroy frees what clx_mel_destroy did not.  CLX_API_ERROR (clx_last_error says
 * why) for a null argument, n_fft, hop or n_mels out of range, an unknown mode, and a floor that is not > 0 in a log mode (in
 * CLX_MEL_POWER the floor is not used).  clx_mel_destroy waits for the launches that use the handle. */
enum { CLX_MEL_POWER = 0, CLX_MEL_LN = 1, CLX_MEL_LOG10 = 2 };
typedef struct clx_mel_spec clx_mel_spec;
int  clx_mel_create(clx_ctx* ctx, uint32_t n_fft, uint32_t hop, const float* window, const float* fbank, uint32_t n_mels,
                    uint32_t mode, float floor, clx_mel_spec** spec);
/* Centred frames and per-window range scaling (clx_k_mel_c, clx_k_mel_range).  clx_mel_create_ex is
 * clx_mel_create with options; opts == NULL or all zero is clx_mel_create itself: the same tables, kernel and words.
 *
 *   center, pad   With P = n_fft / 2 (integer division) frame t of window k is x[n] = p[t*H + n - P], n = 0..N-1, where p
 *              continues the dense window a[k][0 .. L) on both sides:  p[i] = a[k][i] for 0 <= i < L;  for i < 0, p[i] = a[k][-i]
 *              (CLX_MEL_PAD_REFLECT) or 0 (CLX_MEL_PAD_ZERO);  for i >= L, p[i] = a[k][2(L-1) - i] (reflect) or 0 (zero).  The
 *              reflection is about the window's own ends 0 and L-1, not about valid[k]: what a model sees on a crop that was
 *              zero-padded to L (torch.stft(center=True) on that crop).  Everything after x[n] is the definition above, in the
 *              kernel's same order of sums, so a centred call is bit-equal to the uncentred one on the batch padded by P on both
 *              sides on the host (with valid[k] + P for valid[k] > 0).  clx_mel_windows requires P < window_len and
 *              (n_frames-1)*H + N <= window_len + 2P -- torch.stft's frame count, n_frames <= 1 + floor(L / H) for even N -- in
 *              place of the uncentred condition.
 *   validity   valid_frames[k] = 0 if valid[k] == 0, else min(n_frames, ceil((valid[k] + P) / H)): the frames with
 *              t*H - P < valid[k].  A frame at or past it is dead: not computed, whatever a reflection would bring into it.
 *   loads      Zero mode: a tap outside [0, valid[k]) is taken as +0.0 and not loaded (the window is zeros from valid[k] on, so
 *              this changes no word).  Reflect mode: a live frame may load any float of [0, L).  Nothing outside the [B, L]
 *              batch is read in either mode.
 *   range      Log modes only.  Let y be the mode's output of a live cell, and let a dead cell take y0 = logf(floor) /
 *              log10f(floor) as the device computes it for M = 0 (a dead frame and a computed frame of zeros are the same
 *              words).  max_k is the maximum of y over all n_frames * n_mels cells of window k, dead ones included.  Then
 *              out = fl32(fl32(max(y, fl32(max_k - range_width)) + shift) * scale): the subtract, the add and the multiply are
 *              each rounded once, nothing is contracted.  A ranged call writes no +0.0 padding frames: a dead cell holds the
 *              scaled silence value.  Whisper: log10, floor 1e-10, range_width 8, shift 4, scale 0.25; AmplitudeToDB(top_db=80)
 *              on power: log10, range_width 8, shift 0, scale 10.  The maximum is found by the feature launch itself (one
 *              unsigned atomicMax per block on an order-preserving encoding: order independent, hence deterministic) and applied
 *              by a second launch behind it on the same stream, in place.  With range == 0 nothing of the last step changes.
 *
 * CLX_API_ERROR also for: center or range other than 0 or 1, an unknown pad, and with range == 1: CLX_MEL_POWER, a range_width
 * that is not finite and > 0, a shift that is not finite, a scale that is not finite or is zero. */
enum { CLX_MEL_PAD_REFLECT = 0, CLX_MEL_PAD_ZERO = 1 };
typedef struct { uint32_t center, pad, range; float range_width, shift, scale; } clx_mel_opts;
int  clx_mel_create_ex(clx_ctx* ctx, uint32_t n_fft, uint32_t hop, const float* window, const float* fbank, uint32_t n_mels,
                       uint32_t mode, float floor, const clx_mel_opts* opts, clx_mel_spec** spec);
/* Framed specs: a frame shorter than the transform, conditioned before the window, over the first n_bins bins, counted in whole
 * frames (clx_k_mel_f).  This is what Kaldi's fbank needs (torchaudio.compliance.kaldi.fbank, kaldi-native-fbank):
 * 400 samples padded at the end to 512, each frame's own mean removed and a pre-emphasis applied whose first tap refers to the
 * frame's own first sample, 256 of 257 bins, snip_edges.  The spec is (n_fft N in 2..2048, win_length Nw in 1..N, a float32 window
 * w[Nw], n_bins in 1..N/2+1, a float32 filterbank fb[n_mels][n_bins], and hop, n_mels, mode, floor as clx_mel_create), with
 * opts == NULL meaning all zero: remove_dc and whole_frames are 0 or 1, preemph is finite and in [0, 1], 0 meaning none.  The handle
 * is an ordinary clx_mel_spec for clx_mel_windows and clx_mel_destroy.  A framed spec is uncentred and unranged.
 *
 *   frame      frame t of window k is x[n] = a[k][t*H + n], n = 0..Nw-1.  clx_mel_windows requires (n_frames-1)*H + Nw <= L.
 *   conditioning  All in float32, each operation rounded once, none contracted.  If remove_dc: S = sum_n x[n] in the kernel's
 *              order (8 partial sums over n = i, i+8, .. ascending, folded pairwise), mu = fl32(S / (float)Nw) and
 *              d[n] = fl32(x[n] - mu); otherwise d = x.  If preemph = c > 0: y[n] = fl32(d[n] - fl32(c d[n-1])) for n >= 1 and
 *              y[0] = fl32(d[0] - fl32(c d[0])) -- Kaldi's in-place loop; otherwise y = d.
 *   basis      c[j][n] = fl32(w[n] cos(2 pi ((j n) mod N) / N)), s[j][n] = fl32(-w[n] sin(..)) for j < n_bins and n < Nw, built in
 *              double and rounded once as for clx_mel_create.  A tap n >= Nw does not exist (the padding to N is zeros and is
 *              not multiplied).
 *   the rest   re_j, im_j, P_j, M_m and the mode are clx_mel_create's with y in place of x and n_bins in place of J.  A
 *              filterbank row may be all zero (with many bands Kaldi's lowest ones are): it gives finish(0), i.e. 0, logf(floor)
 *              or log10f(floor).
 *   bound      For ANY order of the sums, with mean|x| = sum_n |x[n]| / Nw, x[n'] the sample in front of x[n] (x[0] for n = 0)
 *              and y* the exact conditioning of the float32 samples:  dmu = g(Nw+1) mean|x|;
 *              dy[n] = (1+c) dmu + g(3)(|x[n]| + c|x[n']| + (1+c)(|mu| + dmu));
 *              dre_j = g(Nw+2) sum_n (|y*[n]| + dy[n]) |c[j][n]| + sum_n dy[n] |c[j][n]|, dim_j likewise; from dre and dim to dM
 *              as for clx_mel_create.  Without remove_dc the dmu and mu terms drop, without pre-emphasis the c terms.
 *   validity   whole_frames = 0: valid_frames[k] = clamp(ceil(valid[k] / H), 0, n_frames) as ever.  whole_frames = 1:
 *              valid_frames[k] = valid[k] < Nw ? 0 : min(n_frames, 1 + (valid[k] - Nw) / H), Kaldi's snip_edges count: a
 *              half-empty frame with its mean removed is not silence.  A dead frame is +0.0 and is not computed; no float
 *              outside a live frame is read.
 *
 * With remove_dc == 0 and preemph == 0 the launch is clx_k_mel on the spec's tables, and with Nw == N and n_bins == N/2+1 as well
 * the tables are clx_mel_create's, word for word.  CLX_API_ERROR for clx_mel_create's refusals and for a win_length outside 1..n_fft,
 * n_bins outside 1..n_fft/2+1, remove_dc or whole_frames other than 0 or 1, and a preemph that is not finite or not in [0, 1].
 * The definition restates Kaldi's; it has not been compared with a Kaldi binary. */
typedef struct { uint32_t remove_dc, whole_frames; float preemph; } clx_mel_frame_opts;
int  clx_mel_create_framed(clx_ctx* ctx, uint32_t n_fft, uint32_t win_length, uint32_t hop, const float* window /*[win_length]*/,
                           const float* fbank /*[n_mels][n_bins]*/, uint32_t n_bins, uint32_t n_mels, uint32_t mode, float floor,
                           const clx_mel_frame_opts* opts, clx_mel_spec** spec);
/* Cepstral specs: a framed spec whose log-mel cells go through a DCT and a lifter inside the feature kernel, with the frame's log
 * energy in row 0 if asked for (clx_k_mel_q).  This is Kaldi's MFCC (compute-mfcc-feats,
 * torchaudio.compliance.kaldi.mfcc): 23 bands, 13 coefficients, the orthonormal DCT-II, the lifter 1 + 11 sin(pi i / 22), and
 * use_energy with raw_energy.  The spec is clx_mel_create_framed's (opts == NULL meaning all zero, as there) and cep, which is
 * required: n_ceps in 1..n_mels, a float32 dct[n_ceps][n_mels], a float32 lifter[n_ceps] or NULL for none, energy 0 or 1,
 * energy_scale finite and > 0, energy_floor finite and >= 0 (0: none).  The handle is an ordinary clx_mel_spec for clx_mel_windows
 * and clx_mel_destroy; the output has n_ceps rows in place of n_mels: [B, n_ceps, n_frames] (CLX_WINDOW_CT) or [B, n_frames, n_ceps]
 * (CLX_WINDOW_TC).
 *
 *   log-mel    Y[f][m] = finish(M_m) of frame f is clx_mel_create_framed's, word for word: the same frames, conditioning, basis,
 *              sums in the same order and the same last step (mode and floor; CLX_MEL_POWER gives the DCT of the band sums).
 *   cepstrum   C[f][i] = sum_m dct[i][m] Y[f][m] as one fmaf chain in float32, m ascending, from +0.0.  With a lifter
 *              C[f][i] = fl32(C[f][i] * lifter[i]), rounded once and not contracted (Kaldi's MulElements behind its GEMV).
 *   energy     (energy == 1; Kaldi's use_energy with raw_energy=true.)  d[n] is the frame after the mean's removal (if remove_dc:
 *              d[n] = fl32(x[n] - mu), mu as above) and before pre-emphasis and the window.  e_i = fmaf(d[n], d[n], e_i) over
 *              n = i, i+8, .. ascending for i = 0..7, from +0.0; e = ((e_0 + e_4) + (e_2 + e_6)) + ((e_1 + e_5) + (e_3 + e_7)), each sum
 *              rounded once; E = fl32(e * energy_scale) (a window in the int16 range carries 32768, the energy needs its
 *              square, a power of two); le = logf(max(E, FLT_EPSILON)); if energy_floor > 0 and le < logf(energy_floor),
 *              le = logf(energy_floor).  Row 0 of the output is le in place of C[f][0]; it is not liftered.
 *   bound      With dY_m the bound of Y_m (dM through the logarithm), for ANY order of the sum:
 *              dC_i = sum_m |dct[i][m]| dY_m + g(n_mels+1) sum_m |dct[i][m] Y_m|, and one more rounding for the lifter.
 *   validity   clx_mel_create_framed's rules.  A dead frame is +0.0 in all n_ceps rows and is not computed; no float outside a
 *              live frame is read; the call writes all of d_out.
 *
 * Every cepstral spec runs clx_k_mel_q, whether it conditions its frames or not.  A lane of that kernel keeps its share of a frame
 * group's log-mel cells in 16 registers until the group's power spectrum has been read, hence n_mels <= 128; and a spec of more
 * than one pass of 256 bins parks its partial band sums in the output's rows, which a cepstral output does not have, hence
 * n_bins <= 256.  CLX_API_ERROR, each by a text of its own, for clx_mel_create_framed's refusals and for cep == NULL, n_mels > 128,
 * n_bins > 256, n_ceps outside 1..n_mels, dct == NULL, energy other than 0 or 1, an energy_scale that is not finite or not > 0 and
 * an energy_floor that is not finite or negative.  The definition restates Kaldi's; it has not been compared with a Kaldi binary. */
typedef struct { uint32_t n_ceps; const float* dct /*[n_ceps][n_mels]*/; const float* lifter /*[n_ceps] or NULL*/; uint32_t energy;
                 float energy_scale, energy_floor; } clx_mel_cep_opts;
int  clx_mel_create_cepstral(clx_ctx* ctx, uint32_t n_fft, uint32_t win_length, uint32_t hop, const float* window /*[win_length]*/,
                             const float* fbank /*[n_mels][n_bins]*/, uint32_t n_bins, uint32_t n_mels, uint32_t mode, float floor,
                             const clx_mel_frame_opts* opts, const clx_mel_cep_opts* cep, clx_mel_spec** spec);
/* Reflected specs: Kaldi's snip_edges=false (feature-window.cc: NumFrames and ExtractWindow, restated), which lhotse's extractors and
 * icefall's kaldifeat set-ups use, so that an utterance of T samples has (T + hop/2) / hop frames whatever the frame length is
 * (clx_k_mel_fr, clx_k_mel_qr).  A reflected spec is clx_mel_create_framed's spec, or with cep != NULL
 * clx_mel_create_cepstral's: the same arguments, tables, conditioning, basis, band sums, logarithm, DCT, lifter and raw-energy row,
 * word for word.  Three things differ.  Below V = valid[k], H = hop, Nw = win_length, and every division is the integer division of
 * non-negative numbers.
 *
 *   count      window k has valid_frames[k] = min(n_frames, (V + H/2) / H) live frames: none for V = 0, none for 0 < V < H - H/2.
 *              whole_frames does not apply and must be 0.
 *   placement  tap n of frame t is index i = t*H + H/2 - Nw/2 + n of the window, a signed 64-bit number: negative for the first
 *              frames when Nw > H, and from V up for the last ones.
 *   edge rule  the tap's value is x[n] = a[k][r(i)], r being Kaldi's loop: while i < 0 or i >= V, i = -i - 1 if i < 0, else
 *              i = 2V - 1 - i.  This is reflection with the edge sample repeated (.. a[1] a[0] | a[0] a[1] .. a[V-1] | a[V-1]
 *              a[V-2] ..), iterated, so that a window shorter than a frame is folded as often as it takes; equivalently
 *              j = i mod 2V (non-negative) and r = j < V ? j : 2V - 1 - j.  The reflection is about V and not about window_len, and
 *              no float outside [0, V) of a window is read.
 *
 * Everything behind it sees the frame x[n] = a[k][r(i_n)]: the mean is summed in the stated lane order (lane i of 8 adds n = i,
 * i+8, .., then the partial sums are folded 4, 2, 1); the pre-emphasis tap is x[n-1], the mapped neighbour, and x[0] itself for
 * n = 0; the raw energy of a cepstral spec is taken over the mapped, mean-removed frame.  A dead frame is +0.0 in every row and is
 * not computed; the call writes all of d_out.  clx_mel_windows puts no condition between window_len and n_frames on a reflected
 * spec: valid[k] <= window_len is all.  Hence: the reflected spec's live cells of window k are, word for word, the cells of the
 * whole-frame spec with the same tables on the window p[i] = a[k][r(i + H/2 - Nw/2)], i < (T-1)*H + Nw, T the live frame count.
 *
 * Every reflected spec runs clx_k_mel_fr, or clx_k_mel_qr if it is cepstral, whether it conditions its frames or not; the limits
 * are the siblings' (a cepstral one: n_mels <= 128, n_bins <= 256).  CLX_API_ERROR, each by a text of its own, for every refusal of
 * clx_mel_create_framed, with cep != NULL every refusal of clx_mel_create_cepstral, and for opts->whole_frames != 0.  The count
 * and the origin H/2 - Nw/2 restate Kaldi's code; they have not been compared with a Kaldi binary or another implementation. */
int  clx_mel_create_reflected(clx_ctx* ctx, uint32_t n_fft, uint32_t win_length, uint32_t hop, const float* window /*[win_length]*/,
                              const float* fbank /*[n_mels][n_bins]*/, uint32_t n_bins, uint32_t n_mels, uint32_t mode, float floor,
                              const clx_mel_frame_opts* opts, const clx_mel_cep_opts* cep /* NULL: fbank rows */, clx_mel_spec** spec);
void clx_mel_destroy(clx_ctx* ctx, clx_mel_spec* spec);
/* The features of d_audio [n_windows][window_len] (device, float32) into d_out (device, float32), asynchronously on `stream`
 * (NULL: the context's).  valid is a host array; it is staged like the window table of clx_gather_windows: pinned staging, a
 * table that has to grow is replaced before anything is queued, one event behind the upload and one behind the launch, so the
 * call returns without waiting for the device and valid may be reused at once.  CLX_API_ERROR for a null argument, a spec of
 * another context, window_len < (n_frames-1)*hop + n_fft, a valid[k] > window_len and an unknown layout.  n_windows == 0 or
 * n_frames == 0 succeeds and launches nothing.  The spec decides the kernel, the length condition and the valid_frames rule: a
 * centred or ranged spec runs clx_k_mel_c (its table also carries, per window, the end of what may be loaded and the encoded
 * maximum, initialised by the upload), a ranged one clx_k_mel_range behind it; a framed spec is held to win_length in place of
 * n_fft and to its own valid_frames rule, and runs clx_k_mel_f if it conditions its frames; a cepstral spec is a framed spec that
 * runs clx_k_mel_q and writes n_ceps rows in place of n_mels; a reflected spec is held to valid[k] <= window_len alone and to its
 * own count, runs clx_k_mel_fr or (cepstral) clx_k_mel_qr, and its table also carries valid[k] per window. */
int  clx_mel_windows(clx_ctx* ctx, const clx_mel_spec* spec, const void* d_audio, size_t n_windows, uint32_t window_len,
                     const uint32_t* valid, uint32_t n_frames, uint32_t layout, void* d_out, void* stream);
/* Per-window mean and variance normalisation of a dense float32 batch, in place on the device: what wav2vec 2.0 / HuBERT / WavLM do
 * to a waveform (zero mean, unit variance over the valid samples) and what utterance CMVN does to a feature matrix (per band over
 * the valid frames).  d_data is [n_windows][rows][T] (CLX_WINDOW_CT) or [n_windows][T][rows] (CLX_WINDOW_TC); window k has
 * n = valid[k] <= T live time steps, the rest is padding.  For window k and row r, with x[t] the row's cells, t < n:
 *
 *   S          the sum of (double)x[t] in double, each addition rounded once, in the ORDER below.
 *   m          (float)(S / n): a double division, then one rounding to float32.  m = +0.0 for n == 0.
 *   d[t]       fl32(x[t] - m): one float32 subtraction, rounded to nearest.
 *   Q          the sum of (double)d[t] * (double)d[t] in double (the product is exact in double), in the same ORDER.  The
 *              variance is always taken about the mean, whatever `mean` is (Speech2Text with normalize_means=False does the same).
 *   v          (float)(Q / (n - ddof)), and +0.0 where n <= ddof.
 *   s          sqrtf(fl32(v + eps)): the float32 addition and the square root are both correctly rounded.  With var == 0 the
 *              second pass is skipped and s counts as 1.
 *   cell       y = mean ? d[t] : x[t]; then var ? fl32(y / s) : y, the division correctly rounded float32.
 *   padding    every cell at t >= n becomes `pad`, whatever it held (it is not read by the sums); a window with n == 0 is all `pad`.
 *   zero       a row with v + eps == 0 gives what IEEE gives: 0 / 0 = NaN, or +-Inf where the row is not centred, as numpy does.
 *   stats      d_stats (may be NULL) is [n_windows][rows][2] float32 and receives (m, s) of every row, so that a caller can undo
 *              the step: x = y * s + m.  (n == 0: (0, sqrtf(eps)); var == 0: s = 1.)
 *
 *   ORDER      a function of (t, n) alone -- never of the layout, the grid, rows or r -- so CT and TC of the same data give the
 *              same m, s and cells bit for bit.  The time axis is cut into chunks of 4096 steps: chunk c holds t in
 *              [4096 c, min(4096 (c + 1), n)).  Inside a chunk there are 64 strands: strand i adds the chunk's cells with
 *              t = i mod 64 in ascending t, from +0.0.  The 64 strand sums are folded by an xor tree in six steps, d = 32, 16,
 *              8, 4, 2, 1: a[i] = a[i] + a[i ^ d] for every i at once; a[0] is the chunk's partial sum.  The row's sum is the
 *              partials of the chunks with a live cell added in ascending c, from +0.0.  No floating-point atomics.
 *   bound      the S and Q computed are within n * 2^-53 (relative to the sum of the magnitudes) of the exact sums of the same
 *              terms; DESIGN.md 4.15 carries that through to the cells.
 *
 * opts: mean, var and ddof are 0 or 1 and not mean == var == 0; eps is finite and >= 0; pad is finite.  rows is 1..256: the 1..8
 * channels of a window batch and every n_out a mel spec can have (n_mels <= 256).  valid is a host array, staged as
 * clx_mel_windows stages it (pinned staging, tables that have to grow are replaced before anything is queued, one event behind
 * the upload and one behind the last launch), so the call is asynchronous on `stream` (NULL: the context's), returns without
 * waiting for the device and valid may be reused at once.  The sums wait between the launches in a per-call table of
 * n_windows * rows * 2 * ceil(T / 4096) doubles that the context keeps.  CLX_API_ERROR, each with a clx_last_error text of its
 * own, for opts == NULL, a mean, var or ddof other than 0 or 1, mean == var == 0, an eps that is negative or not finite, a pad that
 * is not finite, an unknown layout, rows outside 1..256, a null d_data or valid, a valid[k] > T and a call with more than 2^31 - 1
 * chunks.  n_windows == 0 or T == 0 succeeds and launches nothing. */
typedef struct { uint32_t mean, var, ddof; float eps, pad; } clx_norm_opts;
int  clx_norm_windows(clx_ctx* ctx, void* d_data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                      const clx_norm_opts* opts, void* d_stats, void* stream);
/* A second batch of windows added to a dense float32 batch at a target signal-to-noise ratio, in place on the device: noise or
 * music behind speech, a second speaker, babble.  d_data is [n_windows][rows][T] (CLX_WINDOW_CT) or [n_windows][T][rows]
 * (CLX_WINDOW_TC), rows in 1..8, and is modified; d_noise is [n_noise][rows][T] in the same layout and is never written.
 * noise_index[k] = j names the noise window added to signal window k, -1 none; several k may name one j.  For window k, with
 * x[r][t] its cells and n[r][t] those of noise window j:
 *
 *   Vs, Vn     Vs = valid[k]; Vn = min(noise_valid[j], Vs): the noise samples that fall inside the signal's live part.
 *   Es         the sum over the rows r ascending, from +0.0, of the row sum of (double)x[r][t] * (double)x[r][t] over t < Vs (the
 *              product is exact in double); each row sum in clx_norm_windows' ORDER with n = Vs: chunks of 4096, 64 strands, the xor
 *              fold, the chunks' partials ascending from +0.0; every addition a double addition rounded once.
 *   En         the same over n[r][t], t < Vn (ORDER with n = Vn).  The ORDER is a function of (t, count) alone, so CT and TC of the
 *              same data give the same Es, En, g and cells bit for bit.
 *   q          pow(10.0, -(double)snr_db[k] / 10.0), computed by the host's libm in double and handed to the device as a double in
 *              the per-call table; q = 0 for snr_db[k] = +inf.  Nothing transcendental runs on the device.
 *   g          (float)sqrt((Es * (double)Vn * q) / (En * (double)Vs)): double multiplications left to right in each bracket, one
 *              double division, one correctly rounded double square root, one rounding to float32.  This is the ratio of MEAN
 *              powers, each signal counted over its own live samples: 10 log10((Es / Vs) / (g^2 En / Vn)) = snr_db.  Where the
 *              noise covers the window (Vn == Vs) it is the gain of torchaudio.functional.add_noise.
 *              g = +0.0 where noise_index[k] < 0, Vs == 0, Vn == 0, Es == 0, En == 0 or q == 0.
 *   range      nothing is clamped.  The double arithmetic cannot overflow on finite cells (a square is below 2^256, q below 2^67),
 *              but the rounding to float32 can: a ratio beyond FLT_MAX (a loud signal over a noise of a few subnormal cells at
 *              snr_db near -200) gives g = +inf, one far below the subnormals g = +0.0 (the window is then not rewritten).  With
 *              g = +inf the cells are what IEEE gives: +-inf where n is not zero, NaN where it is.  Cells that are inf or NaN
 *              themselves make Es or En inf or NaN, and g and the window's cells follow by the same rules; other windows do not.
 *   cell       for t < Vn: fmaf(g, n[r][t], x[r][t]), one rounding.  Cells with Vn <= t < Vs and cells with t >= Vs (padding) keep
 *              their words, whatever the noise holds there; a window with g == +0.0 is not rewritten at all; no noise cell with
 *              t >= Vn is read, no data cell with t >= Vs.
 *   gains      d_gains (may be NULL) is [n_windows] float32 and receives g of every window of a call that launches.
 *
 * opts is NULL or all zero (room for later).  valid, noise_valid, noise_index and snr_db are host arrays, staged as
 * clx_norm_windows stages valid -- one pinned table a call (q, Vs, Vn, j per window), tables that have to grow replaced before
 * anything is queued, one event behind the upload and one behind the last launch -- so the call is asynchronous on `stream`
 * (NULL: the context's), returns without waiting for the device and the arrays may be reused at once.  The partial sums wait
 * between the launches in a table of n_windows * 2 * rows * ceil(T / 4096) doubles that the context keeps, g in one of n_windows
 * floats.  No floating-point atomics.  CLX_API_ERROR, each with a clx_last_error text of its own, for opts that are not zero, an
 * unknown layout, rows outside 1..8, a null valid, noise_index or snr_db, a valid[k] > T, a noise_index[k] outside -1 ..
 * n_noise - 1, a snr_db[k] that is NaN, one that is -inf or beyond 200 in magnitude, and -- where some noise_index[k] >= 0 -- a
 * null d_data, d_noise or noise_valid and a noise_valid[j] > T.  n_windows == 0, T == 0 or every noise_index[k] == -1 succeeds,
 * launches nothing and leaves d_gains alone.  Not here: tiling a short noise over a long window and several noises in one call
 * (both are clx_addn_windows below), other gain rules (peak, loudness). */
typedef struct { uint32_t reserved; } clx_add_opts;
int  clx_add_windows(clx_ctx* ctx, void* d_data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                     const void* d_noise, size_t n_noise, const uint32_t* noise_valid, const int32_t* noise_index,
                     const float* snr_db, uint32_t layout, const clx_add_opts* opts, void* d_gains, void* stream);
/* Several noises added to a dense float32 batch in one pass, each placed at an offset or looped over the window, each at its own
 * signal-to-noise ratio against the signal AS IT ARRIVES: the MUSAN half of "MUSAN + RIR" -- music or background noise looped over
 * the utterance (wav-reverberate --duration), babble (several speakers summed), foreground noises dropped in at start times
 * (--additive-signals --start-times --snrs).  d_data is [n_windows][rows][T] (CLX_WINDOW_CT) or [n_windows][T][rows]
 * (CLX_WINDOW_TC), rows in 1..8, Vs = valid[k], and is modified in place.
 *
 *   noise      n_batches <= 8 noise batches: d_noise[b] (a HOST array of device pointers) is [n_noise[b]][rows][T] or
 *              [n_noise[b]][T][rows], with the data's layout, rows and T.  noise_valid is one host array, concatenated over the
 *              batches in order (n_noise[0] + .. + n_noise[n_batches - 1] entries).  No noise batch is ever written; one that
 *              overlaps d_data is the caller's error and undefined.
 *   terms      M = term_first[n_windows] terms in CSR form: window k has terms term_first[k] .. term_first[k + 1] - 1 (term_first
 *              ascends from 0, at most 16 terms a window).  Term m: `batch` (which noise batch), `index` (the noise window in that
 *              batch; -1: the term adds nothing, and batch is not looked at), `offset` (the window sample at which the noise
 *              enters), `loop` (0 or 1), `snr_db` (finite within -200 .. 200, or +inf: nothing added).
 *   cover      P = noise_valid of the term's noise window.  The term covers the window samples off <= t < end, end = Vs with
 *              loop, else min(Vs, off + P); the cover is empty if off >= Vs or P == 0.  Nc = end - off.  At t the term reads noise
 *              sample i mod P, i = t - off (without loop i < P anyway): a looped noise starts over at its live end, not at T.
 *   Es         exactly clx_add_windows' Es over t < Vs of the data as it arrives; every gain of the window is taken from this ONE
 *              Es -- a later term does not see an earlier one in the signal.
 *   En_m       the sum over the rows r ascending, from +0.0, of the row sums of (double)n[r][i mod P]^2 for i = 0 .. Nc - 1, each
 *              row sum in clx_norm_windows' ORDER indexed by i with n = Nc: chunk i / 4096, strand i % 64, the xor fold, the
 *              chunks' partials ascending from +0.0.  A term with offset 0 and no loop sums what clx_add_windows sums, in its order.
 *   g_m        q_m = pow(10.0, -(double)snr_db / 10.0) by the host's libm, 0 for +inf (clx_add_windows' q);
 *              g_m = (float)sqrt((Es * (double)Nc * q_m) / (En_m * (double)Vs)), with clx_add_windows' operations and roundings.
 *              g_m = +0.0 where index < 0, the cover is empty, Es == 0, En_m == 0 or q_m == 0.  Nothing is clamped (see there).
 *   cell       a cell with t < Vs becomes the chain x = fmaf(g_m, n_m[r][(t - off_m) mod P_m], x) over the window's terms in
 *              ascending m, taking those whose cover holds t and whose g_m != 0; one rounding a step.  A cell in no such term's
 *              cover keeps its word, and so does the padding; a window none of whose terms has g_m != 0 is not rewritten; no data
 *              cell with t >= Vs is read, no noise cell at or behind its P.  CT and TC of the same data give the same words.
 *   gains      d_gains (may be NULL) is [M] float32 and receives g_m of every term of a call that launches.
 *
 * Not Kaldi's rule: wav-reverberate divides by the power of the whole noise file and of the whole signal.  Here both are means over
 * the cells that actually meet -- clx_add_windows' rule, kept: 10 log10((Es / Vs) / (g_m^2 En_m / Nc)) = snr_db, and the samples of
 * a looped noise are counted as often as they sound.  Where a noise covers the whole window once the two rules agree.
 *
 * opts is NULL or all zero.  Every array but d_data, the noise batches and d_gains is a host array, staged as clx_add_windows
 * stages its own (one pinned table a call, a table that has to grow replaced before anything is queued, one event behind the
 * upload and one behind the last launch), so the call is asynchronous on `stream` (NULL: the context's) and the arrays may be
 * reused at once.  The partial sums wait in a table of (n_windows + M) * rows * ceil(T / 4096) doubles, the gains in one of M
 * floats.  No floating-point atomics.  CLX_API_ERROR, each with a clx_last_error text of its own, for opts that are not zero, an
 * unknown layout, rows outside 1..8, more than 8 batches, a null valid or term_first, a term_first that does not ascend from 0,
 * more than 16 terms in a window, a valid[k] > T, a null terms with M > 0, a loop other than 0 or 1, a snr_db that is NaN, one that
 * is -inf or beyond 200 in magnitude, an index below -1 or outside its batch, a batch outside 0 .. n_batches - 1, and -- where some
 * index >= 0 -- a null d_data, d_noise, noise_valid or named batch and a noise_valid[j] > T.  n_windows == 0, T == 0, M == 0 or
 * every index == -1 succeeds, launches nothing and leaves d_gains alone.  Not here: Kaldi's whole-file power rule, peak or
 * loudness rules, fades at the loop points, reverberated noises, noise batches of another T, rows or layout. */
typedef struct { uint32_t reserved; } clx_addn_opts;
typedef struct { int32_t batch; int32_t index; uint32_t offset; uint32_t loop; float snr_db; } clx_addn_term;
int  clx_addn_windows(clx_ctx* ctx, void* d_data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                      const void* const* d_noise, const size_t* n_noise, uint32_t n_batches, const uint32_t* noise_valid,
                      const uint32_t* term_first, const clx_addn_term* terms, uint32_t layout, const clx_addn_opts* opts,
                      void* d_gains, void* stream);
/* A dense float32 batch of windows convolved with room impulse responses, out of place on the device: reverberation, the step
 * between the crop and clx_add_windows (noise is added to the reverberant speech).  d_data is [n_windows][rows][T] (CLX_WINDOW_CT)
 * or [n_windows][T][rows] (CLX_WINDOW_TC), rows in 1..8, and is never written; d_out has the same shape and layout, must not
 * overlap d_data, and receives every cell.  d_ir is [n_ir][K] float32, mono responses, row j live for its first ir_len[j] <= K
 * taps, and is never written.  ir_index[k] = j names the response of window k, -1 none; several k may name one j.  For window k
 * with V = valid[k], x[r][t] its cells, h[] row j of d_ir and L = ir_len[j]:
 *
 *   window     the window is the crop: the signal starts at its sample 0, and what the stream held before it is not part of it.
 *   y[r][t]    for t < V: acc = +0.0f; for k = 0, 1, .., min(t, L - 1) in ascending order acc = fmaf(h[k], x[r][t - k], acc), each
 *              step one rounding; y[r][t] = acc.  Every row is convolved with the same response.
 *   before     a tap that reaches before the crop (k > t) is SKIPPED: it is not an fmaf(h[k], +0.0f, acc).  So an infinite or NaN
 *              tap h[k] leaves the outputs t < k alone (it reaches y[r][t] for t >= k, as IEEE gives: inf * 0 = NaN), and an
 *              accumulator of -0.0 stays -0.0.  A cell y[r][t] is a function of x[r][0 .. t] and h[0 .. min(t, L - 1)] alone.
 *   not read   no tap h[k] with k >= L, and no tap with k >= V; no data cell with t >= V: whatever lies there -- NaNs, another
 *              caller's words -- reaches nothing.
 *   other      a cell with t >= V becomes +0.0f, in every window.  A window with ir_index[k] < 0 or L == 0 receives its own
 *              words for t < V (a copy: -0.0 and NaN payloads survive).
 *   layouts    CT and TC of the same data give the same words: a cell's chain does not know the layout.
 *
 * opts->keep_power = 1 (lhotse's normalize_output) rescales a window so that the reverberant signal has the dry signal's power:
 *
 *   Ex, Ey     the sums over the rows r ascending, from +0.0, of the row sums of (double)x[r][t]^2 and of (double)y[r][t]^2 over
 *              t < V (the squares are exact in double), each row sum in clx_norm_windows' ORDER with n = V, exactly as
 *              clx_add_windows defines Es: chunks of 4096, 64 strands, the xor fold, the chunks' partials ascending from +0.0.
 *   g          (float)sqrt(Ex / Ey): one double division, one correctly rounded double square root, one rounding to float32.
 *              g = 1 where the window has no response (ir_index[k] < 0, L == 0), V == 0, Ex == 0 or Ey == 0, and with
 *              keep_power = 0.
 *   cell       fl32(y[r][t] * g) for t < V, one float32 multiplication rounded once; a window with g == 1 is not rewritten.
 *   range      nothing is clamped.  A ratio beyond float32 gives g = +inf or +0.0 and the cells are what IEEE gives (+-inf, NaN
 *              for a zero cell; zeros).  A cell or tap that is inf or NaN makes Ex or Ey inf or NaN; g is then what the double
 *              arithmetic gives (inf / inf = NaN, finite / inf = 0) and the window's cells follow; other windows do not.
 *   gains      d_gains (may be NULL) is [n_windows] float32 and receives g of every window, 1 where nothing was scaled.
 *
 * opts is NULL (keep_power 0) or has keep_power 0 or 1 and reserved 0.  K is 1..65536 (4 s at 16 kHz): a condition of the
 * interface, the cost of the direct form grows with the taps.  valid, ir_len and ir_index are host arrays, staged as
 * clx_add_windows stages its arrays -- one pinned table a call, tables that have to grow replaced before anything is queued, one
 * event behind the upload and one behind the last launch -- so the call is asynchronous on `stream` (NULL: the context's),
 * returns without waiting for the device and the arrays may be reused at once.  The partial sums of keep_power wait between the
 * launches in a table of n_windows * 2 * rows * ceil(T / 4096) doubles that the context keeps.  No floating-point atomics.
 * CLX_API_ERROR, each with a clx_last_error text of its own, for opts with a keep_power above 1 or reserved bits, an unknown
 * layout, rows outside 1..8, K outside 1..65536, a null d_data, d_out, valid or ir_index, a null d_ir or ir_len with n_ir > 0, an
 * ir_len[j] > K, a valid[k] > T, an ir_index[k] outside -1 .. n_ir - 1 and a d_out that overlaps d_data.  n_windows == 0 or
 * T == 0 succeeds and launches nothing.  Not here: an FFT or overlap-save form (that is clx_reverb_windows_fft below, a second method
 * with a definition of its own), multi-channel responses, the tail of what the stream held before the crop. */
typedef struct { uint32_t keep_power, reserved; } clx_reverb_opts;
int  clx_reverb_windows(clx_ctx* ctx, const void* d_data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                        const void* d_ir, size_t n_ir, uint32_t K, const uint32_t* ir_len, const int32_t* ir_index,
                        uint32_t layout, const clx_reverb_opts* opts, void* d_out, void* d_gains, void* stream);
/* The same convolution by uniformly partitioned overlap-save: a second method beside clx_reverb_windows for long responses, whose
 * work does not grow with the taps the way the direct form's does.  The arguments, their shapes and the refusals are
 * clx_reverb_windows' (each text under this call's name); opts is NULL (keep_power 0) or has keep_power 0 or 1 and reserved[] all 0.
 * The call is out of place, asynchronous on `stream`, stages its host arrays as clx_reverb_windows does (a table of 40 bytes a
 * window and 12 a transformed partition) and never writes d_data or d_ir.  Its cells are NOT the direct form's words: they are the
 * words of the schedule below, within the bound of DESIGN.md 4.19 of the exact convolution.  With H = 1024, N = 2 H = 2048, for
 * window k with V = valid[k], L = ir_len[j], Lv = min(L, V), x[r][t] its cells (+0.0f for t < 0 and for t >= V) and h[] its taps
 * (+0.0f for k >= Lv):
 *
 *   twiddles   tw[q] = (fl32(cos(2 pi q / N)), fl32(-sin(2 pi q / N))), q = 0 .. N / 2 - 1: the host's double cos and sin of the
 *              double 2 pi q / N, each rounded once to float32.  One table, uploaded once; no device sine or cosine.
 *   transform  F(w), of N real words w[n]: a[rev(n)] = (w[n], +0.0f), rev the reversal of the 11 bits of n.  Then the stages
 *              s = 1 .. 11 in this order, radix 2, decimation in time; stage s has half = 2^(s - 1), and its butterflies
 *              i = 0 .. N / 2 - 1 (independent of each other) have k = i mod half, lo = 2 (i - k) + k, hi = lo + half,
 *              w = tw[k * (N / 2) / half], u = a[lo], v = a[hi] and
 *                t.re = fmaf(w.re, v.re, -fl(w.im * v.im))        t.im = fmaf(w.re, v.im, fl(w.im * v.re))
 *                a[lo] = (fl(u.re + t.re), fl(u.im + t.im))       a[hi] = (fl(u.re - t.re), fl(u.im - t.im))
 *              : two rounded multiplications, two fmaf and four rounded additions a butterfly.  Bins 0 .. N / 2 of a[] are kept.
 *              The inverse stages G(a) are the same with w.im negated (exact).
 *   segments   X[s] = F(x[r][(s - 1) H + n], n = 0 .. N - 1) for s = 0 .. ceil(V / H) - 1.
 *   partitions Hp[p] = F(h[p H + n] for n < H, +0.0f for n >= H) for p = 0 .. P - 1, P = ceil(Lv / H).
 *   block b    (the outputs t = b H .. b H + H - 1, b H < V) per kept bin, p ascending from the p = 0 product:
 *                p = 0:  Y.re = fmaf(X.re, Hp.re, -fl(X.im * Hp.im))                Y.im = fmaf(X.re, Hp.im, fl(X.im * Hp.re))
 *                p >= 1: Y.re = fmaf(-X.im, Hp.im, fmaf(X.re, Hp.re, Y.re))         Y.im = fmaf(X.im, Hp.re, fmaf(X.re, Hp.im, Y.im))
 *              with X = X[b - p], Hp = Hp[p], over p = 0 .. min(b, P - 1).  Then a[rev(n)] = Y[n] for n <= N / 2 and the
 *              conjugate (Y[N - n].re, -Y[N - n].im) for n > N / 2, the inverse stages, and
 *              y[r][b H + n] = fl(a[H + n].re * 2^-11) for n < H, b H + n < V: the scaling by 1 / N, exact but for underflow.
 *   locality   the words of y[r][t] are a function of x[r][0 .. V), h[0 .. Lv), V and L alone: not of the layout (CT and TC give
 *              the same words), the row count, the other rows, the other windows or the batch.  No two rows or windows share a
 *              transform.  A partition's spectrum is computed once for all windows that read the same taps of it.
 *   not read   no data cell with t >= V, no tap with k >= Lv: what lies there reaches nothing.  A partition wholly behind every
 *              naming window's Lv and a segment wholly behind V are not transformed.
 *   other      a cell with t >= V becomes +0.0f; a window with ir_index[k] < 0 or L == 0 receives its own words for t < V.
 *   non-finite the contract covers finite live cells and taps.  UNLIKE the direct form, which skips a tap before the crop and so
 *              keeps a NaN or infinite tap h[k] from the outputs t < k, every output of a block depends on every tap and every
 *              sample the block's transforms read: a window with a non-finite live cell or tap has unspecified cells for t < V
 *              (and an unspecified gain).  Every other window's words are untouched.
 *   keep_power exactly clx_reverb_windows': Ex, Ey by clx_add's sum kernels over (d_data, d_out), the same g, the same g = 1
 *              cases, the same cell = fl32(y * g), the same d_gains.
 *
 * Workspace: the spectra wait between the two launches in a table the context keeps and grows, of
 * (n_windows * rows * ceil(T / H) + Q) * 8320 bytes, Q the partitions transformed: per response the whole partitions some window
 * reads (max over its windows of floor(Lv / H)) and one ragged partition for every distinct (response, Lv) with Lv mod H != 0.
 * An allocation that fails is CLX_API_ERROR with "hipMalloc reverb spectra" in clx_last_error, before anything is queued.  The
 * partial sums of keep_power are as in clx_reverb_windows.  No floating-point atomics.  K keeps the 1..65536 limit.  Not here:
 * multi-channel responses, tails from audio before the crop, spectra cached across calls, non-uniform partitions. */
typedef struct { uint32_t keep_power, reserved[3]; } clx_reverb_fft_opts;
int  clx_reverb_windows_fft(clx_ctx* ctx, const void* d_data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                            const void* d_ir, size_t n_ir, uint32_t K, const uint32_t* ir_len, const int32_t* ir_index,
                            uint32_t layout, const clx_reverb_fft_opts* opts, void* d_out, void* d_gains, void* stream);
/* SpecAugment of a dense float32 feature batch, out of place on the device: a time warp about one frame, frequency masks and time
 * masks, the last step of the usual speech training recipe.  d_in is [n_windows][rows][T] (CLX_WINDOW_CT) or [n_windows][T][rows]
 * (CLX_WINDOW_TC), rows in 1..256, and is never written; d_out has the same shape and layout and receives every cell; d_out ==
 * d_in is refused.  Window k has V = valid[k] <= T live frames.  With x[r][t] the cells of d_in and y[r][t] those of d_out:
 *
 *   padding    a cell at t >= V is the input's word, whatever it is: copied, never interpreted, never warped, never masked, and
 *              never part of the mean.
 *   warp       warp (may be NULL: none) is [n_windows][2], the pair (c, w) of window k.  (0, 0) is no warp; otherwise
 *              1 <= c <= V - 1 and 1 <= w <= V - 1.  Output frames [0, w) are input frames [0, c) resized, output frames [w, V)
 *              are input frames [c, V) resized, each segment by torch.nn.functional.interpolate(mode="bicubic",
 *              align_corners=False) along time with the coordinate taken exactly.  For local output frame j of a segment with I
 *              input and O output frames that starts at input frame b:
 *                num = (2 j + 1) I - O, den = 2 O (64-bit integers); ix = floor(num / den), which is -1 where num < 0;
 *                tx = (float)((double)(num - ix den) / (double)den): one double division, one rounding to float32.
 *                The weights, every operation one float32 rounding, none fused, with near(u) = fl(fl(fl(fl(fl(1.25 u) - 2.25) u) u) + 1)
 *                and far(u) = fl(fl(fl(fl(fl(fl(-0.75 u) + 3.75) u) - 6) u) + 3) (the cubic convolution with A = -0.75):
 *                w_0 = far(fl(tx + 1)), w_1 = near(tx), w_2 = near(fl(1 - tx)), w_3 = far(fl(2 - tx)).
 *                The source frames: s_k = b + clamp(ix - 1 + k, 0, I - 1), k = 0 .. 3: inside the segment, never the other segment,
 *                the padding or another window.
 *                y[r][t] = acc after acc = +0.0f; acc = fmaf(w_k, x[r][s_k], acc) for k = 0, 1, 2, 3: four fused steps.
 *              Where I == O (c == w) the segment's cells are the input's words, copied and not computed, as torch does; a NaN
 *              next to such a cell stays where it is.
 *   masks      fmasks (may be NULL) is [n_windows][F][2]: (first_row, width); tmasks (may be NULL) is [n_windows][M][2]:
 *              (first_frame, width), counted in output (warped) frames.  F = opts->n_freq_masks and M = opts->n_time_masks are at
 *              most 32.  Time masks are clipped to [0, V), frequency masks to [0, rows) and to the frames t < V.  Width 0 masks
 *              nothing; masks may overlap.  A masked cell is the fill, whatever the warp would have given: its taps are not read.
 *   fill       opts->fill_mean == 0: the constant opts->fill (finite).  opts->fill_mean == 1: the window's mean over the live
 *              cells of the INPUT (before the warp): S_r the sum of (double)x[r][t] over t < V in clx_norm_windows' ORDER with
 *              n = V, S the sum of S_r in ascending r from +0.0, fill = (float)(S / (double)(V * rows)): one double division, one
 *              rounding; +0.0 for V == 0.  d_fill (may be NULL) is [n_windows] float32 and receives every window's fill.
 *   layouts    CT and TC of the same data give the same fill and the same cells, bit for bit.
 *
 * valid, warp, fmasks and tmasks are host arrays of 32-bit unsigned words, staged as clx_add_windows stages its arrays -- one
 * pinned table a call, tables that have to grow replaced before anything is queued, one event behind the upload and one behind
 * the last launch -- so the call is asynchronous on `stream` (NULL: the context's), returns without waiting for the device and
 * the arrays may be reused at once.  With fill_mean the row sums wait in a table of n_windows * rows * 2 * ceil(T / 4096) doubles
 * that the context keeps (clx_norm's sum kernels write it).  No floating-point atomics.  CLX_API_ERROR, each with a
 * clx_last_error text of its own, for opts == NULL, reserved bits, a fill_mean above 1, a constant fill that is not finite, F or M
 * above 32, an unknown layout, rows outside 1..256, T above 2^31 - 1 (the frames of a window are counted in 32 bits with one to
 * spare for ix = -1, and (2 j + 1) I stays below 2^63), a null d_in, d_out or valid, d_out == d_in, a valid[k] > T and a warp pair
 * outside the ranges above.  n_windows == 0 or T == 0 succeeds and launches nothing.  Not here: warps in frequency, several warp
 * points per window, other interpolation modes, the drawing of the random plan (that is the caller's: claxon_amd.SpecAugment). */
typedef struct { uint32_t n_freq_masks, n_time_masks, fill_mean; float fill; uint32_t reserved; } clx_specaug_opts;
int  clx_specaug_windows(clx_ctx* ctx, const void* d_in, void* d_out, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                         uint32_t layout, const uint32_t* warp, const uint32_t* fmasks, const uint32_t* tmasks,
                         const clx_specaug_opts* opts, void* d_fill, void* stream);
/* Frame splicing of a dense float32 feature batch on the device, out of place: blocks of small time-domain FIRs over every window's
 * valid frames, the edge frame repeated, with an output stride.  Kaldi's add-deltas, splice-feats and subsample-feats and FunASR's
 * low-frame-rate stacking are plans of it (claxon_amd.Splice builds them).  d_in is [n_windows][rows][T] (CLX_WINDOW_CT) or
 * [n_windows][T][rows] (CLX_WINDOW_TC), rows in 1..256, and is never written.  Window k has V = valid[k] <= T live frames.
 *
 *   plan       K = opts->n_blocks blocks (1..32), a stride s = opts->stride (1..64); block j is blocks[j]: an offset o_j
 *              (|o_j| <= 64), a half-width m_j (0..16) and either copy = 1 (then m_j = 0) or copy = 0 and the 2 m_j + 1 float32
 *              coefficients c_j[-m_j .. m_j] at coefs[coef .. coef + 2 m_j].  K * rows is at most 8192.
 *   output     d_out is [n_windows][K * rows][T_out] (CT) or [n_windows][T_out][K * rows] (TC), T_out = ceil(T / s); the call
 *              writes every float of it.  Window k has V_out = ceil(V / s) live output frames.
 *   live       for u < V_out, with t = u s + o_j and clamp(i) = min(max(i, 0), V - 1), row j * rows + r of frame u is
 *                copy block   the 32-bit word of x[r][clamp(t)], moved and never interpreted: NaN payloads and -0.0 survive;
 *                FIR block    acc after acc = +0.0f; acc = fmaf(c_j[d], x[r][clamp(t + d)], acc) for d = -m_j .. m_j ascending:
 *                             2 m_j + 1 fused steps, one rounding each; no tap is skipped, a zero coefficient included.
 *   padding    a frame u >= V_out is the word of opts->pad in every row; a window with V = 0 is all padding.
 *   reads      no cell of d_in outside the frames [0, V) of its window is read, whatever it holds.
 *   layouts    CT and TC of the same data give the same words.
 *
 * valid, blocks and coefs are host arrays, staged as clx_specaug_windows stages its arrays (one pinned table a call, tables that
 * have to grow replaced before anything is queued, one event behind the upload and one behind the launch), so the call is
 * asynchronous on `stream` (NULL: the context's), returns without waiting for the device and the arrays may be reused at once.
 * CLX_API_ERROR, each with a clx_last_error text of its own, for opts == NULL, reserved bits, n_blocks outside 1..32, a stride
 * outside 1..64, an unknown layout, rows outside 1..256 (so K * rows cannot pass 8192), T above 2^31 - 1, blocks == NULL, an offset, a
 * half-width or a copy mark out of range, a copy block with a half-width, a FIR block with coefs == NULL, a null d_in, d_out or
 * valid, d_out == d_in and a valid[k] > T.  n_windows == 0 or T == 0 succeeds and launches nothing.  Not here: per-window plans,
 * running in place, deltas in frequency.
 *
 * clx_splice_deltas fills the plan of Kaldi's DeltaFeatures (host only, no context): block 0 a copy, block i = 1 .. order the
 * i-fold convolution of [-window .. window] / (2 sum_{d = 1 .. window} d^2) with itself at offset 0, m_i = i * window, the clamp
 * applied once to the combined filter.  The numerators and the denominators (2 sum d^2)^i are whole numbers; a coefficient is
 * (float)((double)num / (double)den).  blocks receives order + 1 entries, coefs their coefficients (84 floats at most), *n_coefs
 * their count.  CLX_API_ERROR for a null argument, order above 4, and with order >= 1 a window of 0 or order * window above 16. */
typedef struct { int32_t offset; uint32_t m, copy, coef; } clx_splice_block;
typedef struct { uint32_t n_blocks, stride; float pad; uint32_t reserved; } clx_splice_opts;
int  clx_splice_windows(clx_ctx* ctx, const void* d_in, void* d_out, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                        uint32_t layout, const clx_splice_block* blocks, const float* coefs, const clx_splice_opts* opts, void* stream);
int  clx_splice_deltas(uint32_t order, uint32_t window, clx_splice_block* blocks, float* coefs, uint32_t* n_coefs);
/* Global CMVN of a dense float32 feature batch on the device, in place: a fixed shift and scale per row, from a stats file
 * (WeNet's global_cmvn, FunASR's am.mvn behind the low-frame-rate stacking, Kaldi's apply-cmvn with global statistics).  d_data is
 * [n_windows][rows][T] (CLX_WINDOW_CT) or [n_windows][T][rows] (CLX_WINDOW_TC), rows in 1..8192 (the most clx_splice_windows can
 * emit).  Window k has V = valid[k] <= T live frames.
 *
 *   plan       one launch (clx_k_cmvn_global), tiles of 1024 16-byte vectors of a window, 16-byte accesses where a vector lies
 *              whole inside the window (and, on the load side, inside its live cells); no LDS.
 *   live       for t < V, y = fl32(fl32(x + shift[r]) * scale[r]): two float32 operations, each rounded to nearest, never one
 *              fused multiply-add.  That is word for word what (x + shift) * scale gives in numpy or torch float32, hence FunASR's
 *              (x + means) * vars and WeNet's (x - mean) * istd with shift = -mean.  ESPnet's GlobalMVN divides, x / std, which is
 *              another rounding and is not bit-equal to a multiplication by 1 / std.
 *   padding    every cell with t >= V becomes the word of opts->pad; a window with V = 0 is all padding.
 *   reads      no cell with t >= V is read, whatever it holds.
 *   layouts    CT and TC of the same data give the same words.
 *
 * valid, shift and scale (rows float32 each) are host arrays, staged as clx_splice_windows stages its arrays (one pinned table a
 * call -- V per window, then shift, then scale --, tables that have to grow replaced before anything is queued, one event behind
 * the upload and one behind the launch), so the call is asynchronous on `stream` (NULL: the context's), returns without waiting
 * for the device and the arrays may be reused at once.  CLX_API_ERROR, each with a clx_last_error text of its own, for
 * opts == NULL, reserved bits, a pad that is not finite, an unknown layout, rows outside 1..8192, T above 2^31 - 1, shift == NULL,
 * scale == NULL, a shift or a scale that is not finite, a null d_data or valid, a valid[k] > T and more than 2^31 - 1 tiles.
 * n_windows == 0 or T == 0 succeeds and launches nothing.
 *
 * Sliding-window CMVN, out of place (Kaldi's apply-cmvn-sliding, the normaliser of the x-vector recipes): every live cell minus
 * the mean of its row over a window of frames around (center) or up to (not center) its own, optionally divided by the standard
 * deviation over the same frames.  d_in and d_out have one shape, as above; d_in is never written.
 *
 *   options    window N (1..1024; Kaldi's default 600), min_window M (1..N, only read when center == 0; Kaldi's 100), center and
 *              norm_vars (0 or 1), pad.
 *   window     for live frame t of a window with V live frames the statistics window [a, b) is Kaldi's SlidingWindowCmnInternal as
 *              this project reads it (neither Kaldi nor torchaudio was run against it):
 *                center:      a = t - N / 2 (whole-number division);  b = a + N
 *                not center:  a = t - N;                              b = t + 1
 *                if a < 0:             b -= a;  a = 0
 *                if !center and b > t: b = max(t + 1, M)
 *                if b > V:             a -= b - V;  b = V;  if a < 0: a = 0
 *                n = b - a
 *              so 0 <= a <= t < b <= V, and an uncentred window holds up to N + 1 frames.
 *   ORDER      a row's sums S (of (double)x[u]) and Q (of (double)x[u] * (double)x[u], exact in double) over [a, b) are added up
 *              in an order that is a function of (a, b, V) alone, never of the layout, the tile or the grid.  The time axis is cut
 *              into groups of 32 frames from frame 0: G[k] is the double sum of (double)x[u] over u in [32 k, min(32 k + 32, V))
 *              ascending from +0.0, H[k] the same over the squares.  With ka = ceil(a / 32) and kb = floor(b / 32): if ka <= kb, S
 *              starts at +0.0 and adds x[a .. 32 ka) one by one ascending, then G[ka .. kb) ascending, then x[32 kb .. b)
 *              ascending; otherwise S adds x[a .. b) ascending.  Q likewise with squares and H.  Every addition is a double
 *              addition rounded once: at most 62 cell additions and 32 group additions a sum, instead of 1025.
 *   live       m = S / (double)n; y = (double)x[t] - m; with norm_vars and n > 1 (n == 1: y stays; Kaldi sets the variance to 1):
 *              v = Q / (double)n - m * m (a division, a product and a difference, each rounded once, none fused),
 *              v = v < 1e-10 ? 1e-10 : v, y = y / sqrt(v) (a correctly rounded double square root and division).  The cell is
 *              (float)y, one rounding.  Cells that are not finite give what IEEE gives inside the windows that reach them, and
 *              nothing elsewhere.
 *   padding    a frame t >= V is the word of opts->pad in every row; a window with V = 0 is all padding.
 *   reads      no cell of d_in outside the frames [0, V) of its window is read, whatever it holds.
 *   layouts    CT and TC of the same data give the same words.
 *   plan       one launch (clx_k_cmvn_sliding): a block is a tile of 256 output frames of one window; it stages the tile's source
 *              span [32 floor(a(first frame) / 32), b(last live frame)), at most 1311 frames, of 8 rows at a time as floats in
 *              LDS with the span's whole groups' G and H as doubles beside them (48 608 bytes: three workgroups a CU); a tile whose
 *              frames are all padding writes the pad and stages nothing.
 *
 * valid is staged as above (the table is V per window).  CLX_API_ERROR, each with a text of its own, for opts == NULL, reserved
 * bits, a pad that is not finite, an unknown layout, rows outside 1..8192, T above 2^31 - 1, window outside 1..1024, center or
 * norm_vars above 1, with center == 0 a min_window outside 1..window, a null d_in, d_out or valid, d_out == d_in, a valid[k] > T
 * and more than 2^31 - 1 tiles.  n_windows == 0 or T == 0 succeeds and launches nothing.  Not here: windows above 1024 frames.
 * (Accumulating the statistics of a corpus is clx_cmvn_stats_windows, Kaldi's VAD is clx_vad_windows, both below.)
 *
 * clx_cmvn_from_stats (host only, no context) turns Kaldi's CMVN accumulator into shift and scale: stats is [2][rows + 1] doubles,
 * row 0 the sums and the count, row 1 the sums of squares (its last entry unused).  mean = sum / count,
 * var = max(sumsq / count - mean * mean, 1e-20) (ApplyCmvn's floor), shift = -mean, scale = norm_vars ? 1 / sqrt(var) : 1, all in
 * double, each result rounded once to float32.  Kaldi itself applies x * scale + offset with offset = -mean * scale, which rounds
 * differently from (x + shift) * scale: the two agree to float32 rounding, not word for word.  CLX_API_ERROR for a null argument,
 * rows outside 1..8192, norm_vars above 1, a count that is not above 0 and statistics that give a shift or scale that is not finite. */
typedef struct { float pad; uint32_t reserved; } clx_cmvn_global_opts;
typedef struct { uint32_t window, min_window, center, norm_vars; float pad; uint32_t reserved; } clx_cmvn_sliding_opts;
int  clx_cmvn_global_windows(clx_ctx* ctx, void* d_data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                             uint32_t layout, const float* shift, const float* scale, const clx_cmvn_global_opts* opts, void* stream);
int  clx_cmvn_sliding_windows(clx_ctx* ctx, const void* d_in, void* d_out, size_t n_windows, uint32_t rows, uint32_t T,
                              const uint32_t* valid, uint32_t layout, const clx_cmvn_sliding_opts* opts, void* stream);
int  clx_cmvn_from_stats(const double* stats, uint32_t rows, uint32_t norm_vars, float* shift, float* scale);
/* Kaldi's CMVN accumulator on the device (compute-cmvn-stats, per corpus or per speaker), and the normalisation of every window by
 * the accumulator of its group (apply-cmvn --utt2spk).  d_data is a dense float32 feature batch, [n_windows][rows][T]
 * (CLX_WINDOW_CT) or [n_windows][T][rows] (CLX_WINDOW_TC), rows in 1..8192, window k with V = valid[k] <= T live frames:
 * clx_cmvn_global_windows' shape and limits.  group is n_windows int32 on the host: group[k] in 0..n_groups - 1 is the group
 * (speaker) of window k, -1 says the window takes no part, group == NULL says every window is group 0.  n_groups is 1..65536.
 * d_stats is the accumulator, device memory the caller owns, 8-byte aligned: [n_groups][2][rows + 1] doubles in Kaldi's layout --
 * row 0 the sums of the group's live cells per feature row, with the number of frames in column `rows`; row 1 the sums of their
 * squares, with column `rows` unused (0 behind a reset, otherwise untouched).  One group's [2][rows + 1] on the host is what
 * clx_cmvn_from_stats and a Kaldi stats file hold.
 *
 * The accumulation, clx_cmvn_stats_windows: d_data is only read.
 *
 *   options    accumulate (0: the accumulator is zeroed first, all n_groups groups of it; 1: the call adds to what it holds).
 *   ORDER      per window k, feature row r and chunk c of 4096 frames the call forms S_c, the double sum of (double)x[t], and
 *              Q_c, the double sum of (double)x[t] * (double)x[t] (exact in double: raw squares, as Kaldi's accumulator holds
 *              them, not deviations), over the chunk's live frames exactly as clx_norm_windows forms its S_c: strand i of 64 adds
 *              the frames t = i mod 64 ascending from +0.0, the strands are folded by xor 32, 16, 8, 4, 2, 1 (strand i takes
 *              strand i ^ d), every addition a double addition rounded once.  W[k][r] is the S_c of the window's live chunks
 *              added ascending from +0.0 (a window with V = 0: +0.0), likewise for Q.  Then, per group g and word of it,
 *              acc = accumulate ? the word : +0.0, and acc += W[k] for the windows k with group[k] == g in ascending k; the count
 *              column adds (double)valid[k] the same way.  The order is a function of (valid, group) alone, never of the
 *              layout or the grid, and nothing is added atomically: the same calls leave the same words.
 *   absent     a group without a window in this call keeps its words (accumulate) or is zeros (reset).  A group whose windows
 *              all have V = 0 adds +0.0 to its words.
 *   reads      no cell with t >= V is read, whatever it holds, and no cell of a window with group -1.  Cells that are not finite
 *              give what IEEE gives in their group, row and sum, and nothing elsewhere.
 *   layouts    CT and TC of the same data give the same words.
 *   plan       a memset of the accumulator (reset only), then two launches: clx_k_cmvn_stats_sum (CT, and TC with one row: a wave
 *              is one chunk of one row, no LDS) or clx_k_cmvn_stats_sum_tc (TC: clx_norm's tile of 64 frames x 16 rows through
 *              4 352 bytes of LDS) makes one pass over the data and leaves S_c and Q_c in a per-call table of doubles
 *              [n_windows][rows][2][chunks]; clx_k_cmvn_stats_fold, one lane a (group with a window, column, S | Q), folds them
 *              into the accumulator along the host's list of each group's windows (a stable counting sort, CSR, part of the
 *              call's staged table).
 *
 * Two calls that accumulate into one d_stats read and write the same words: the caller has to order them, by queueing them on
 * one stream or by an event between their streams.  (The per-call tables are the context's and are handed from call to call as
 * every window call's are; d_stats is the caller's and is not.)
 *
 * The normalisation, clx_cmvn_grouped_windows, in place: d_shift_scale is device memory the caller owns, [n_groups][2][rows]
 * floats (a group's shifts, then its scales), written by the call and only meaningful to it: nothing is allocated per call.
 *
 *   options    norm_vars (0 or 1), pad.
 *   solve      per group and row, clx_cmvn_from_stats' arithmetic on the device, word for word: in double, nothing fused,
 *              mean = sum / count, var = max(sumsq / count - mean * mean, 1e-20), shift = (float)(-mean),
 *              scale = norm_vars ? (float)(1 / sqrt(var)) : 1 (a correctly rounded division and square root, each result rounded
 *              once to float32).  A group whose count is not above 0 gets shift +0.0 and scale 1.0f (its cells come out as x + 0);
 *              statistics that are not finite give what IEEE gives, in that group only -- where clx_cmvn_from_stats refuses.
 *   live       for t < V and g = group[k] >= 0, y = fl32(fl32(x + shift[g][r]) * scale[g][r]), clx_cmvn_global_windows' two
 *              float32 operations: with one group, the words of clx_cmvn_global_windows given clx_cmvn_from_stats' vectors.  A
 *              window with group -1 keeps its live cells.
 *   padding    every cell with t >= V becomes the word of opts->pad, in a window of group -1 too.
 *   reads      no cell with t >= V is read.  d_stats is only read.
 *   layouts    CT and TC of the same data give the same words.
 *   plan       two launches: clx_k_cmvn_stats_solve, one lane a (group, row), over all n_groups groups; clx_k_cmvn_grouped,
 *              clx_k_cmvn_global's tiling (1024 16-byte vectors a block, 16-byte accesses where a vector lies whole inside the
 *              window and its live cells), shift and scale read from d_shift_scale.  No LDS.
 *
 * valid and group are staged before either call returns (one pinned table a call, as clx_cmvn_global_windows stages its arrays), so
 * the calls are asynchronous on `stream` (NULL: the context's), return without waiting for the device, and the arrays may be reused
 * at once.  n_windows == 0 or T == 0 succeeds and launches nothing -- except that clx_cmvn_stats_windows with accumulate == 0 still
 * zeroes the accumulator (that is how an accumulator is reset on a stream).  CLX_API_ERROR, each with a clx_last_error text of its
 * own, for opts == NULL, reserved bits, accumulate or norm_vars above 1, a pad that is not finite, an unknown layout, rows outside
 * 1..8192, T above 2^31 - 1, n_groups outside 1..65536, a null d_stats, a d_stats that is not 8-byte aligned, a null or misaligned
 * d_shift_scale, a null d_data or valid, a valid[k] > T, a group[k] outside -1..n_groups - 1 and more than 2^31 - 1 blocks in a
 * launch. */
typedef struct { uint32_t accumulate; uint32_t reserved; } clx_cmvn_stats_opts;
typedef struct { uint32_t norm_vars; float pad; uint32_t reserved; } clx_cmvn_grouped_opts;
int  clx_cmvn_stats_windows(clx_ctx* ctx, const void* d_data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                            uint32_t layout, const int32_t* group, uint32_t n_groups, void* d_stats, const clx_cmvn_stats_opts* opts,
                            void* stream);
int  clx_cmvn_grouped_windows(clx_ctx* ctx, void* d_data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                              uint32_t layout, const int32_t* group, uint32_t n_groups, const void* d_stats, void* d_shift_scale,
                              const clx_cmvn_grouped_opts* opts, void* stream);
/* Kaldi's energy VAD over one row of a dense float32 feature batch on the device (compute-vad), and the selection of the frames a
 * byte mask names (select-voiced-frames, or any other mask: a neural VAD's).  d_data is [n_windows][rows][n_frames] (CLX_WINDOW_CT)
 * or [n_windows][n_frames][rows] (CLX_WINDOW_TC), rows 1..8192; valid[k] <= n_frames is window k's live frames V.
 *
 * The decision, clx_vad_windows: d_mask is [n_windows][n_frames] bytes, d_thresholds (may be NULL) [n_windows] floats.
 *
 *   options    float32 energy_threshold E (Kaldi's default 5.0) and energy_mean_scale s (0.5), frames_context c (0..128; 0) and
 *              float32 proportion_threshold p (0 < p < 1; 0.6); row r < rows, the energy row (0: C0 or the log energy of a Kaldi
 *              MFCC); reserved words, 0.  conf/vad.conf of the VoxCeleb and SRE16 recipes: 5.5, 0.5, 2, 0.12.
 *   energy     e[t] is the cell at (row r, frame t) of the window.
 *   SUM        S is the double sum of (double)e[0 .. V) in clx_norm_windows' order: chunks of 4096 frames; inside a chunk strand
 *              i of 64 adds the cells t = i mod 64 ascending from +0.0; the strands fold by xor 32, 16, 8, 4, 2, 1; the chunks
 *              that hold a live frame add up ascending from +0.0.  Every addition is a double addition rounded once.  The same
 *              function of the cells in CT and TC.
 *   threshold  s == 0 (Kaldi's `if (mean_scale != 0)`) or V == 0: thr = E, and with s == 0 nothing is summed and no sum kernel is
 *              launched.  Otherwise thr = (float)(E + s * (S / V)): E, s and V as doubles, a division, a product and a sum, each
 *              rounded once to double, none fused, then one rounding to float32.
 *   above      above[u] = e[u] > thr, a float32 compare: false for a NaN on either side, false for a cell equal to thr.
 *   decision   for t < V: lo = max(t - c, 0), hi = min(t + c, V - 1), den = hi - lo + 1, num = the number of above[u] over
 *              lo <= u <= hi; the byte is ((float)num >= fl32((float)den * p)) ? 1 : 0, one float32 product rounded once.  For
 *              t >= V the byte is 0.
 *   reads      no cell at t >= V and no cell of another row is read, whatever it holds.
 *   outputs    every byte of d_mask is written once; d_thresholds[k] = thr.  d_data is not written.
 * This is Kaldi's ComputeVadEnergy as this project reads it.  Kaldi sums the energies and forms the threshold in float32, so a cell
 * within an ulp or so of the threshold may fall the other way there; no Kaldi binary was run against this.
 *   plan       clx_k_vad_sum (a wave a chunk of a window's energy row; skipped when s == 0), then clx_k_vad_decide: a block is a
 *              tile of 256 frames; it folds the partial sums into thr, takes the `above` flags of the tile and its context (512
 *              frames at most) with ballots, leaves an inclusive prefix count in LDS (2 080 bytes) and forms num as the difference
 *              of two entries: no lane loops over the context.
 * CLX_API_ERROR, each with a clx_last_error text of its own, for opts == NULL, reserved words, an E or s that is not finite, a p
 * outside (0, 1) or not finite, c above 128, an unknown layout, rows outside 1..8192, n_frames above 2^31 - 1, row >= rows, a null
 * d_data, valid or d_mask, a valid[k] > n_frames and more than 2^31 - 1 tiles.  n_windows == 0 or n_frames == 0 succeeds and
 * launches nothing.
 *
 * The selection, clx_select_windows, out of place: frame t < V of window k is selected when d_mask[k][t] != 0; bytes at t >= V are
 * never read.  count is the number of selected frames.  Output frame j < count holds the words of source frame t_j, the j-th
 * selected frame in ascending order: a copy of 32-bit words over all rows, so NaN payloads survive.  Output frames count <= j <
 * n_frames hold the word of opts->pad in every row (any float32 value).  d_dst has d_src's shape and must not overlap it; every
 * cell of d_dst is written exactly once, d_src is not written and no cell of it at t >= V is read.  CT and TC give the same words.
 * count == 0 is a window that is all pad, not an error (Kaldi skips such an utterance).  d_counts (device uint32 [n_windows], may
 * be NULL) receives the counts.
 *   plan       clx_k_select_rank (a block a tile of 256 source frames: ballots, the tile's popcount), clx_k_select_scan (a wave a
 *              window: the exclusive scan of the tile counts, and count), clx_k_select_move (a block a source tile: ranks from the
 *              ballots, the tile's selected frames listed in LDS, 1 040 bytes, then lanes along the output's contiguous axis; the
 *              block also writes the pad of its own 256 output frames).
 * With counts (HOST uint32 [n_windows], may be NULL) the call copies the counts into it and RETURNS ONCE THEY HAVE ARRIVED, through
 * the pinned staging of its scratch set and a wait on the event behind its own launches: the one window entry point that waits for
 * the device.  Without counts it is asynchronous like the others.
 * CLX_API_ERROR, each with a text of its own, for opts == NULL, reserved words, an unknown layout, rows outside 1..8192, n_frames
 * above 2^31 - 1, a null d_src, d_dst, valid or d_mask, a valid[k] > n_frames, more than 2^31 - 1 tiles and a d_dst that overlaps
 * d_src.  n_windows == 0 or n_frames == 0 succeeds and launches nothing (counts is then zeros, d_counts is not written).
 * Both calls stage valid[] as the calls above do and share one scratch set. */
typedef struct { float energy_threshold, energy_mean_scale; uint32_t frames_context; float proportion_threshold; uint32_t row; uint32_t reserved[3]; } clx_vad_opts;
typedef struct { float pad; uint32_t reserved[3]; } clx_select_opts;
int  clx_vad_windows(clx_ctx* ctx, const void* d_data, size_t n_windows, uint32_t rows, uint32_t n_frames, const uint32_t* valid,
                     uint32_t layout, const clx_vad_opts* opts, void* d_mask, void* d_thresholds, void* stream);
int  clx_select_windows(clx_ctx* ctx, const void* d_src, void* d_dst, size_t n_windows, uint32_t rows, uint32_t n_frames,
                        const uint32_t* valid, const void* d_mask, uint32_t layout, const clx_select_opts* opts, void* d_counts,
                        uint32_t* counts, void* stream);
/* Number of predictor slots (subframes incl. alignment padding) in the plan. */
uint64_t clx_batch_slots(const clx_batch* b);
/* Per-kernel HIP-event timing: kernels are numbered in launch order (clx_batch_kernel_name gives the name; NULL past the last
 * one).  enable = 1: every clx_batch_run / clx_batch_submit is a plain run with an event in front of each kernel (the LAST run's
 * durations are kept); enable = 2: pipelined submissions go out as usual and the events bracket the kernels of each MERGED launch
 * of the lane kernels (the LAST launch's durations are kept: submit, clx_batch_flush, synchronise, read); 0: off. */
int  clx_batch_set_profiling(clx_batch* b, int enable);
int  clx_batch_kernel_ms(clx_batch* b, int kernel, float* ms);
const char* clx_batch_kernel_name(const clx_batch* b, int kernel);
void clx_batch_destroy(clx_batch* b);

/* ------------------------------------------------------------------------
 * Stream API (host C++ classes claxon::FlacReader / FrameReader / Block live
 * in claxon_amd/csrc/host/claxon.hpp; these are their C handles so that any
 * FFI can reach them).  Replaces FlacReader::{new,open,streaminfo,blocks}
 * (lib.rs:217-458) and FrameReader::read_next_or_eof (frame.rs:667) for a
 * stream held in memory; frames are indexed on the host and decoded on the
 * device in batches.
 * ---------------------------------------------------------------------- */
typedef struct clx_streaminfo {          /* metadata.rs:24-54 */
    uint16_t min_block_size, max_block_size;
    uint32_t min_frame_size, max_frame_size;   /* 0 = unknown (None) */
    uint32_t sample_rate, channels, bits_per_sample;
    uint64_t samples;                          /* 0 = unknown (None) */
    uint8_t  md5sum[16];
} clx_streaminfo;

typedef struct clx_block_info {          /* frame.rs:402-411 (Block) */
    uint64_t time;
    uint32_t block_size;
    uint32_t channels;
} clx_block_info;

typedef struct clx_reader clx_reader;

/* Parse the `fLaC` marker + metadata blocks of an in-memory stream
 * (lib.rs:186-205, 230-307; metadata.rs:214-400).  *audio_offset = first frame byte. */
int clx_read_stream_header(const uint8_t* data, size_t len, clx_streaminfo* info,
                           size_t* audio_offset, uint32_t* msg);

/* FLAC tags (VORBIS_COMMENT block; FlacReader::vendor / tags / get_tag, lib.rs:321-360, metadata.rs:73-212). */
typedef struct clx_tags clx_tags;
enum {
    CLX_OPT_METADATA_ONLY        = 1u << 0,   /* FlacReaderOptions::metadata_only (lib.rs:131): stop once the wanted metadata is in */
    CLX_OPT_NO_VORBIS_COMMENT    = 1u << 1    /* FlacReaderOptions::read_vorbis_comment = false (lib.rs:141) */
};
/* FlacReader::new_ext (lib.rs:230-307) on an in-memory stream: clx_read_stream_header plus the tags.  *tags (may be
 * NULL on return: the stream has no Vorbis comment block, or it was not asked for) is owned by the caller. */
int clx_read_stream_header_ext(const uint8_t* data, size_t len, uint32_t options, clx_streaminfo* info,
                               size_t* audio_offset, clx_tags** tags, uint32_t* msg);
const char* clx_tags_vendor(const clx_tags* t, size_t* len);              /* the vendor string (UTF-8, not NUL-safe: use *len) */
size_t      clx_tags_count(const clx_tags* t);
/* i-th "NAME=value" pair in stream order; pointers stay valid until clx_tags_free */
int         clx_tags_get(const clx_tags* t, size_t i, const char** name, size_t* name_len, const char** value, size_t* value_len);
/* value of the `occurrence`-th tag whose name equals `name` ASCII-case-insensitively (metadata::GetTag, metadata.rs:197-211);
 * NULL when there is none */
const char* clx_tags_lookup(const clx_tags* t, const char* name, size_t occurrence, size_t* value_len);
void        clx_tags_free(clx_tags* t);
/* tags of an open reader (NULL if the stream has none); owned by the reader */
const clx_tags* clx_reader_tags(const clx_reader* r);

/* One metadata block, as `metadata::read_metadata_block` (metadata.rs:261-319) returns it: for streams embedded in a
 * container (examples/decode_ogg.rs:32-41, 85-103: Ogg packets hold metadata blocks with their header;
 * examples/decode_mp4.rs: the "FLAC specific box" holds type and raw data).  `kind` is the variant of the reference's
 * `MetadataBlock` enum (metadata.rs:104-131): seek tables, cue sheets and pictures are read as Padding (the reference's
 * TODOs at metadata.rs:287, 296, 301), unknown types as Reserved. */
enum { CLX_BLOCK_STREAMINFO = 0, CLX_BLOCK_PADDING = 1, CLX_BLOCK_APPLICATION = 2, CLX_BLOCK_VORBIS_COMMENT = 4, CLX_BLOCK_RESERVED = 126 };
typedef struct clx_metadata_block {
    uint32_t kind;                       /* CLX_BLOCK_* */
    uint32_t length;                     /* Padding { length } (metadata.rs:108-111); the block's length for every kind */
    clx_streaminfo streaminfo;           /* StreamInfo(..) */
    uint32_t application_id;             /* Application { id, data } (metadata.rs:113-118) */
    const uint8_t* application_data;     /* points into the caller's buffer */
    size_t application_len;
    clx_tags* tags;                      /* VorbisComment(..); owned by the caller: clx_tags_free */
} clx_metadata_block;
/* read_metadata_block (metadata.rs:261): `data[0..len)` stands right behind the block header, whose fields the caller
 * passes.  *consumed = bytes read on success.  Errors and messages as the reference (too short a buffer: CLX_IO_ERROR). */
int clx_read_metadata_block(const uint8_t* data, size_t len, uint8_t block_type, uint32_t length,
                            clx_metadata_block* out, size_t* consumed, uint32_t* msg);
/* read_metadata_block_with_header (metadata.rs:244): header (last-block flag + type, 24-bit length; metadata.rs:214-231)
 * and body.  *is_last receives the header's flag (MetadataBlockReader stops after it, metadata.rs:573-578). */
int clx_read_metadata_block_with_header(const uint8_t* data, size_t len, clx_metadata_block* out, int* is_last,
                                        size_t* consumed, uint32_t* msg);
/* Container packets -> frame descriptors.  What the reference's container examples do per packet -- FrameReader::new over
 * the packet's bytes, then read_next_or_eof (examples/decode_ogg.rs:105-114, decode_mp4.rs:143-152) -- for n packets at
 * once: packet i = arena[offs[i] .. offs[i] + lens[i]) holds one frame; its header is parsed (clx_parse_frame_header) into
 * descs[i] / headers[i] (either may be NULL) with max_bytes = lens[i].  results[i] (may be NULL) receives the header's
 * status and message; packets shorter than two bytes give CLX_END_OF_STREAM (frame.rs:140-143; the examples skip empty
 * packets).  Returns CLX_OK when every packet has a valid header, else the first failing packet's status. */
int clx_describe_packets(const uint8_t* arena, size_t arena_len, const uint64_t* offs, const uint32_t* lens, size_t n,
                         int check_crc, clx_frame_desc* descs, clx_frame_header* headers, clx_frame_result* results);

int  clx_reader_open(clx_ctx* ctx, const char* path, clx_reader** out, uint32_t* msg);       /* lib.rs:455 */
int  clx_reader_new(clx_ctx* ctx, const uint8_t* data, size_t len, clx_reader** out, uint32_t* msg); /* lib.rs:217 */
int  clx_reader_streaminfo(const clx_reader* r, clx_streaminfo* out);                        /* lib.rs:312 */
/* read_next_or_eof: decodes (in device batches, lazily) and hands out the next
 * block.  `buffer` (capacity `cap` i32) receives channels*block_size planar
 * samples.  CLX_END_OF_STREAM at the end; errors as the reference. */
int  clx_reader_next_block(clx_reader* r, int32_t* buffer, size_t cap,
                           clx_block_info* info, uint32_t* msg);                             /* frame.rs:667 */
void clx_reader_close(clx_reader* r);

/* Host-side frame indexer for a contiguous stream: locates frame starts by
 * sync code + CRC-8-valid header, confirmed by the previous frame's CRC-16
 * (frame.rs:131-316 grammar; the reference has no resync, frame.rs:601-602).
 * Writes up to `cap` descriptors/headers; returns the number found in *n_found.
 * Stops at the first position where the chain cannot be continued and reports
 * that byte offset in *stop_off. */
int clx_index_frames(const uint8_t* data, size_t len, size_t start_off,
                     clx_frame_desc* descs, clx_frame_header* headers, size_t cap,
                     size_t* n_found, size_t* stop_off);

/* The same indexer with the byte work on the GPU (sync-code scan + CRC-8 of every candidate header, CRC-16 of every
 * byte between candidates); identical outputs.  `data` is a host pointer, or with CLX_ARENA_ON_DEVICE a 16-byte
 * aligned device pointer whose allocation is padded like a decode arena (>= round16(len) + 32 bytes). */
int clx_index_frames_device(clx_ctx* ctx, const uint8_t* data, size_t len, size_t start_off,
                            clx_frame_desc* descs, clx_frame_header* headers, size_t cap,
                            size_t* n_found, size_t* stop_off, uint32_t flags);

/* The device indexer for a whole shard: `n_streams` streams that lie in one arena, indexed in one pass (a fixed number of
 * kernel launches, allocations and host-device synchronisations per call, whatever n_streams is).  Stream k is
 * arena[offs[k] .. offs[k] + lens[k]); its indexing begins at offs[k] + starts[k] (what clx_read_stream_header reported
 * as the audio offset, 0 for a bare frame sequence; starts == NULL: all zero).  offs[k] is a multiple of 16 and the
 * streams ascend without overlap.
 * Contract: for every k the frames, headers and stop offset are exactly what
 *   clx_index_frames(arena + offs[k], lens[k], starts[k], ...)
 * returns for that stream alone, with byte_off and stop_offs[k] rebased onto the arena (offs[k] added); max_bytes still
 * ends at the stream's own end.  Nothing outside [offs[k] + starts[k], offs[k] + lens[k]) influences stream k's answer,
 * and no stream's content makes the call fail (candidates are held as one bit per byte position: nothing overflows).
 * Frames of stream k are descs[first_frame[k] .. first_frame[k + 1]) (first_frame has n_streams + 1 entries);
 * *n_found = first_frame[n_streams].  If the frames do not fit `cap` the call returns CLX_API_ERROR with *n_found set
 * to the number needed (first_frame and stop_offs are complete, descs / headers untouched): call again with that cap.
 * CLX_API_ERROR with a clx_last_error that names the stream for a misaligned, overlapping or out-of-arena stream and for
 * starts[k] > lens[k]; also for NULL outputs (headers may be NULL) and an arena of 4 GiB or more.
 * `arena` is a host pointer (uploaded once), or with CLX_ARENA_ON_DEVICE a device pointer under the rule of
 * clx_index_frames_device.
 * Memory: the call's device scratch (2 bytes per 16 arena bytes, 34 bytes per candidate header, and for a host arena
 * its device copy) belongs to the context and is kept until clx_destroy; a call that needs more than any call before
 * frees and reallocates it (which waits for the device), later calls of that size allocate nothing. */
int clx_index_streams_device(clx_ctx* ctx, const uint8_t* arena, size_t arena_len,
                             const uint64_t* offs, const uint64_t* lens, const uint64_t* starts, size_t n_streams,
                             clx_frame_desc* descs, clx_frame_header* headers, size_t cap,
                             uint64_t* first_frame, uint64_t* stop_offs, size_t* n_found, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* CLAXON_HIP_H */
