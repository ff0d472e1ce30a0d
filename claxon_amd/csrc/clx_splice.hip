// clx_splice.hip -- frame splicing of a dense float32 feature batch, out of place: K blocks of small time-domain FIRs (or word
// copies) over every window's valid frames, the edge frame repeated, with an output stride: Kaldi's add-deltas, splice-feats and
// subsample-feats and FunASR's low-frame-rate stacking are plans of it: clx_splice_windows.  claxon_hip.h has the definition; this
// is how it is computed.  It stands alone: one launch, no sums, nothing taken from the other kernels.
//
// The per-call table (clx_splice_fill_table, uploaded once) is 32-bit words: V[n], then the K blocks as (offset, m, copy, first
// coefficient), then the FIR blocks' coefficients packed one block behind the other (at most 32 x 33 floats).
//
// clx_k_splice: block = tile kTile = 256 output frames of one window.  A tile wholly at or behind V_out = ceil(V / s) writes the
// pad and reads nothing.  Otherwise the block copies the blocks and coefficients into LDS and works through the tile in sub-tiles
// of Fs output frames by Rc rows (the plan's: clx_splice_check): it stages the sub-tile's source span -- frames
// [max(ua s - H, 0), min((ua + live - 1) s + H, V - 1)], H = max |o_j| + m_j, so never a frame outside [0, V) -- of those rows in
// LDS, one global load a cell, and serves all K blocks from there: a cell is wanted up to K (2m + 1) times, and with s > 1 the CT
// reads of a block would be strided.  (Fs, Rc) are chosen so that ((Fs - 1) s + 1 + 2H) Rc <= kStageWords = 8 192:
//   CT ([n_windows][rows][T]): Fs = 256 and as many rows as fit (s = 1, H = 4: 31 rows; s = 6, H = 3: 5 rows); only a span of one
//      row that does not fit (s >= 32) shortens Fs.  Staged as [row][frame]; the sweep's lanes run along the frames, so a wave
//      stores 64 consecutive floats of one output row and reads LDS at a stride of s words (s = 6: 2-way conflicts, s = 64: 32-way;
//      a stride reads s input words from memory per word stored, which costs more than the conflicts do).
//   TC ([n_windows][T][rows]): all rows and as many frames as fit (13 rows: Fs = 256; 80 rows, s = 6, H = 3: Fs = 16, whose halo
//      is 6 of 102 staged frames).  Staged as [frame][row], one contiguous run of memory; the sweep's lanes run along the
//      K * rows cells of an output frame and on into the next, contiguous in memory too.  Only (2H + 1) rows > 8 192 (rows = 256
//      with H >= 16) splits the rows, one output frame at a time, with stores in runs of Rc floats.
// The sweep is one loop for both: a lane's cell is a three-digit counter (row, block, frame in CT; frame, block, row in TC) stepped
// by 256 without a division.  Loads and stores are 32-bit: a row starts wherever T and the caller's pointer put it, so nothing
// wider is aligned.  A cell is a 32-bit word throughout: a copy never passes through a float register's arithmetic.
// LDS: 8 192 staged words, 32 x 4 block words, 32 x 33 coefficients: 37 504 bytes, four blocks a CU.  Registers: no more than 40
// vector registers (33 as built), no scratch, no spills (tests/test_code_object_splice.py reads them from the code object).
//
// clx_splice_check, clx_splice_fill_table and clx_splice_deltas_build are the host side (plain C++, shared with the wave simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include "../../include/claxon_hip.h"

// the launch shape clx_splice_check gives (n_tiles == 0: nothing to launch)
struct clx_splice_plan {
    uint32_t n_tiles = 0;        // tiles of a window (n_windows * n_tiles blocks)
    uint32_t tc = 0;             // 1: the TC staging and sweep
    uint32_t T_out = 0;          // ceil(T / stride)
    uint32_t H = 0;              // max |o_j| + m_j: how far a tap lies from its output frame's own input frame
    uint32_t Fs = 0, Rc = 0;     // a sub-tile: output frames and rows staged at once
    uint32_t n_coefs = 0;        // coefficients of the FIR blocks, packed
    uint64_t table_words = 0;    // 32-bit words of the per-call table
};

namespace clx_splice {

constexpr uint32_t kThreads = 256u, kTile = 256u, kMaxRows = 256u, kMaxOutRows = 8192u, kMaxBlocks = 32u, kMaxStride = 64u, kMaxOffset = 64u,
                   kMaxHalf = 16u, kMaxCoefs = kMaxBlocks * (2u * kMaxHalf + 1u), kMaxT = 0x7fffffffu, kMaxOrder = 4u;
constexpr uint32_t kStageWords = 8192u;
constexpr uint32_t kLdsBytes = kStageWords * 4u + kMaxBlocks * 4u * 4u + kMaxCoefs * 4u;   // 37 504
static_assert(kTile == kThreads, "a CT sub-tile of a whole tile has one lane a frame");
static_assert((2u * (kMaxOffset + kMaxHalf) + 1u) * 1u <= kStageWords, "one row of one output frame's span always fits");

#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ float fma_rn(float a, float b, float c) { return __fmaf_rn(a, b, c); }
#else
inline float fma_rn(float a, float b, float c) { return fmaf(a, b, c); }
#endif

__device__ __forceinline__ float as_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
__device__ __forceinline__ uint32_t as_u32(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// source frames a sub-tile of F output frames spans at most
__host__ __device__ __forceinline__ uint64_t span_of(uint64_t F, uint32_t s, uint32_t H) { return (F - 1u) * s + 1u + 2u * H; }

}  // namespace clx_splice

// Block b: tile b % n_tiles of window b / n_tiles.  tab is the per-call table; pad the word of every frame from V_out on.
extern "C" __global__ __launch_bounds__(256) void clx_k_splice(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                               const uint32_t* __restrict__ tab, uint32_t n_windows, uint32_t rows, uint32_t T,
                                                               uint32_t T_out, uint32_t K, uint32_t s, uint32_t H, uint32_t n_coefs, uint32_t pad,
                                                               uint32_t tc, uint32_t n_tiles, uint32_t Fs, uint32_t Rc) {
    using namespace clx_splice;
    __shared__ uint32_t s_x[kStageWords];
    __shared__ uint32_t s_blk[kMaxBlocks * 4u];
    __shared__ float s_coef[kMaxCoefs];
    const uint32_t tid = threadIdx.x, k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const uint32_t V = tab[k], V_out = (V + s - 1u) / s, KR = K * rows;
    const uint32_t u0 = tl * kTile, u1 = T_out - u0 < kTile ? T_out : u0 + kTile, nf = u1 - u0;
    const uint32_t* const x = in + (uint64_t)k * rows * T;
    uint32_t* const y = out + (uint64_t)k * KR * T_out;
    if (u0 >= V_out) {                                         // (the whole block) only the pad
        if (tc) {
            const uint64_t e0 = (uint64_t)u0 * KR;
            const uint32_t n = nf * KR;
            for (uint32_t e = tid; e < n; e += kThreads) y[e0 + e] = pad;
        } else if (tid < nf) {
            for (uint32_t c = 0; c < KR; ++c) y[(uint64_t)c * T_out + u0 + tid] = pad;
        }
        return;
    }
    {
        const uint32_t* const bt = tab + n_windows;
        const uint32_t* const ct = bt + 4u * K;
        for (uint32_t i = tid; i < 4u * K; i += kThreads) s_blk[i] = bt[i];
        for (uint32_t i = tid; i < n_coefs; i += kThreads) s_coef[i] = as_f32(ct[i]);
    }
    for (uint32_t f0 = 0; f0 < nf; f0 += Fs) {                 // (every bound of these loops is the whole block's)
        const uint32_t fsn = nf - f0 < Fs ? nf - f0 : Fs, ua = u0 + f0;
        const uint32_t live = ua >= V_out ? 0u : (V_out - ua < fsn ? V_out - ua : fsn);
        uint32_t lo = 0u, n_span = 0u;
        if (live) {                                            // (ua s <= V - 1: ua < ceil(V / s))
            const int64_t a = (int64_t)ua * s - (int64_t)H, b = (int64_t)(ua + live - 1u) * s + (int64_t)H;
            lo = a < 0 ? 0u : (uint32_t)a;
            n_span = (b > (int64_t)V - 1 ? V - 1u : (uint32_t)b) - lo + 1u;
        }
        for (uint32_t r0 = 0; r0 < rows; r0 += Rc) {
            const uint32_t rc = rows - r0 < Rc ? rows - r0 : Rc;
            if (live) {
                if (!tc) {
                    for (uint32_t rl = 0; rl < rc; ++rl) {
                        const uint32_t* const row = x + (uint64_t)(r0 + rl) * T + lo;
                        for (uint32_t i = tid; i < n_span; i += kThreads) s_x[rl * n_span + i] = row[i];
                    }
                } else if (rc == rows) {
                    const uint32_t* const base = x + (uint64_t)lo * rows;
                    const uint32_t n = n_span * rows;
                    for (uint32_t e = tid; e < n; e += kThreads) s_x[e] = base[e];
                } else {
                    const uint32_t n = n_span * rc;
                    for (uint32_t e = tid; e < n; e += kThreads) {
                        const uint32_t i = e / rc, rl = e - i * rc;
                        s_x[e] = x[(uint64_t)(lo + i) * rows + r0 + rl];
                    }
                }
            }
            __syncthreads();
            // the sweep: cell (a, b, c) with c the fastest digit: (row, block, frame) in CT, (frame, block, row) in TC
            const uint32_t C = tc ? rc : fsn, n = rc * K * fsn;
            uint32_t c = tid % C, q = tid / C, b = q % K, a = q / K;
            const uint32_t sc = kThreads % C, sq = kThreads / C, sb = sq % K, sa = sq / K;
            for (uint32_t e = tid; e < n; e += kThreads) {
                const uint32_t rl = tc ? c : a, fl = tc ? a : c;
                uint32_t v = pad;
                if (fl < live) {
                    const int32_t off = (int32_t)s_blk[4u * b];
                    const uint32_t m = s_blk[4u * b + 1u], copy = s_blk[4u * b + 2u], ci = s_blk[4u * b + 3u];
                    const int64_t t = (int64_t)(ua + fl) * s + off, last = (int64_t)V - 1;
                    if (copy) {
                        const uint32_t i = (uint32_t)(t < 0 ? 0 : (t > last ? last : t)) - lo;
                        v = s_x[tc ? i * rc + rl : rl * n_span + i];
                    } else {
                        float acc = 0.f;
                        for (uint32_t d = 0; d <= 2u * m; ++d) {
                            const int64_t td = t - (int64_t)m + d;
                            const uint32_t i = (uint32_t)(td < 0 ? 0 : (td > last ? last : td)) - lo;
                            acc = fma_rn(s_coef[ci + d], as_f32(s_x[tc ? i * rc + rl : rl * n_span + i]), acc);
                        }
                        v = as_u32(acc);
                    }
                }
                if (tc) y[(uint64_t)(ua + fl) * KR + b * rows + r0 + rl] = v;
                else y[(uint64_t)(b * rows + r0 + rl) * T_out + ua + fl] = v;
                c += sc; if (c >= C) { c -= C; ++b; }
                b += sb; if (b >= K) { b -= K; ++a; }
                a += sa;
            }
            __syncthreads();
        }
    }
}

// The host side of clx_splice_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the
// launch shape (p->n_tiles == 0: nothing to launch).
inline const char* clx_splice_check(const void* d_in, const void* d_out, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                                    uint32_t layout, const clx_splice_block* blocks, const float* coefs, const clx_splice_opts* o,
                                    clx_splice_plan* p) {
    using namespace clx_splice;
    *p = clx_splice_plan();
    if (!o) return "clx_splice_windows: null options";
    if (o->reserved != 0u) return "clx_splice_windows: reserved must be 0";
    if (o->n_blocks < 1u || o->n_blocks > kMaxBlocks) return "clx_splice_windows: n_blocks must be 1..32";
    if (o->stride < 1u || o->stride > kMaxStride) return "clx_splice_windows: stride must be 1..64";
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return "clx_splice_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT";
    if (rows < 1u || rows > kMaxRows) return "clx_splice_windows: rows must be 1..256";
    static_assert(kMaxBlocks * kMaxRows <= kMaxOutRows, "K * rows <= 8192 follows from the two ranges");
    if (T > kMaxT) return "clx_splice_windows: T must be below 2^31";
    if (!blocks) return "clx_splice_windows: null blocks";
    const uint32_t K = o->n_blocks, s = o->stride;
    uint32_t H = 0u, nc = 0u;
    for (uint32_t j = 0; j < K; ++j) {
        const clx_splice_block& b = blocks[j];
        if (b.offset < -(int32_t)kMaxOffset || b.offset > (int32_t)kMaxOffset) return "clx_splice_windows: a block's offset must be -64..64";
        if (b.m > kMaxHalf) return "clx_splice_windows: a block's half-width must be 0..16";
        if (b.copy > 1u) return "clx_splice_windows: a block's copy mark must be 0 or 1";
        if (b.copy && b.m != 0u) return "clx_splice_windows: a copy block has half-width 0";
        if (!b.copy && !coefs) return "clx_splice_windows: null coefficients for a FIR block";
        const uint32_t h = (uint32_t)(b.offset < 0 ? -b.offset : b.offset) + b.m;
        if (h > H) H = h;
        if (!b.copy) nc += 2u * b.m + 1u;
    }
    if (n_windows == 0 || T == 0) return nullptr;
    if (!d_in || !d_out || !valid) return "clx_splice_windows: null argument";
    if (d_in == d_out) return "clx_splice_windows: d_out must not be d_in";
    for (size_t k = 0; k < n_windows; ++k)
        if (valid[k] > T) return "clx_splice_windows: valid[k] is larger than T";
    const uint32_t T_out = (uint32_t)(((uint64_t)T + s - 1u) / s);
    const uint64_t tiles = ((uint64_t)T_out + kTile - 1u) / kTile;
    if (n_windows > 0x7fffffffull || tiles * (uint64_t)n_windows > 0x7fffffffull) return "clx_splice_windows: too many windows in one call";
    uint32_t Fs, Rc;
    if (layout == CLX_WINDOW_CT) {
        if (span_of(kTile, s, H) <= kStageWords) {
            Fs = kTile;
            Rc = (uint32_t)(kStageWords / span_of(kTile, s, H));
        } else {
            Fs = (kStageWords - 1u - 2u * H) / s + 1u;
            Rc = 1u;
        }
        if (Rc > rows) Rc = rows;
    } else if (span_of(1u, s, H) * rows <= kStageWords) {
        Rc = rows;
        Fs = (kStageWords / rows - 1u - 2u * H) / s + 1u;
        if (Fs > kTile) Fs = kTile;
    } else {
        Rc = (uint32_t)(kStageWords / span_of(1u, s, H));
        Fs = 1u;
    }
    p->n_tiles = (uint32_t)tiles; p->tc = layout == CLX_WINDOW_TC ? 1u : 0u; p->T_out = T_out; p->H = H; p->Fs = Fs; p->Rc = Rc; p->n_coefs = nc;
    p->table_words = (uint64_t)n_windows + 4u * K + nc;
    return nullptr;
}

// The per-call table of checked arguments into `tab`: V, the blocks with their coefficients' places in the table, the coefficients.
inline void clx_splice_fill_table(uint32_t* tab, size_t n_windows, const uint32_t* valid, const clx_splice_block* blocks, const float* coefs,
                                  uint32_t K) {
    for (size_t k = 0; k < n_windows; ++k) tab[k] = valid[k];
    uint32_t* const bt = tab + n_windows;
    uint32_t* const ct = bt + 4u * K;
    uint32_t at = 0u;
    for (uint32_t j = 0; j < K; ++j) {
        const clx_splice_block& b = blocks[j];
        const uint32_t n = b.copy ? 0u : 2u * b.m + 1u;
        bt[4u * j] = (uint32_t)b.offset; bt[4u * j + 1u] = b.m; bt[4u * j + 2u] = b.copy; bt[4u * j + 3u] = b.copy ? 0u : at;
        if (n) memcpy(ct + at, coefs + b.coef, n * sizeof(float));
        at += n;
    }
}

// Kaldi's DeltaFeatures as a plan: block 0 a copy, block i = 1 .. order the i-fold convolution of [-w .. w] / (2 sum_{1..w} d^2)
// with itself, 2 i w + 1 taps at coefs[blocks[i].coef ..].  The numerators are whole numbers and so are the denominators
// (2 sum d^2)^i: a coefficient is (float)((double)num / (double)den), one double division of two exact operands and one rounding
// to float32.  blocks holds order + 1 entries, coefs order (order w + w + 1) floats at most (84).  nullptr: fine.
inline const char* clx_splice_deltas_build(uint32_t order, uint32_t window, clx_splice_block* blocks, float* coefs, uint32_t* n_coefs) {
    using namespace clx_splice;
    if (!blocks || !n_coefs || (order && !coefs)) return "clx_splice_deltas: null argument";
    if (order > kMaxOrder) return "clx_splice_deltas: order must be 0..4";
    if (order && (window < 1u || order * window > kMaxHalf)) return "clx_splice_deltas: window must be at least 1 and order * window at most 16";
    blocks[0].offset = 0; blocks[0].m = 0u; blocks[0].copy = 1u; blocks[0].coef = 0u;
    int64_t num[2u * kMaxHalf + 1u] = { 1 }, next[2u * kMaxHalf + 1u];
    int64_t den = 1, norm = 0;
    for (uint32_t d = 1; d <= window; ++d) norm += 2 * (int64_t)d * d;
    uint32_t at = 0u;
    for (uint32_t i = 1; i <= order; ++i) {
        const uint32_t taps = 2u * i * window + 1u, prev = taps - 2u * window;
        for (uint32_t a = 0; a < taps; ++a) next[a] = 0;
        for (uint32_t a = 0; a < prev; ++a)
            for (uint32_t b = 0; b <= 2u * window; ++b) next[a + b] += num[a] * ((int64_t)b - (int64_t)window);
        den *= norm;
        for (uint32_t a = 0; a < taps; ++a) { num[a] = next[a]; coefs[at + a] = (float)((double)num[a] / (double)den); }
        blocks[i].offset = 0; blocks[i].m = i * window; blocks[i].copy = 0u; blocks[i].coef = at;
        at += taps;
    }
    *n_coefs = at;
    return nullptr;
}
