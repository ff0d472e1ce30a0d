// clx_reverb.hip -- a dense float32 batch of windows convolved with room impulse responses, out of place: clx_reverb_windows.
// claxon_hip.h has the definition; this is how it is computed.  It stands behind clx_add.hip in clx_api.hip: the
// power sums of keep_power are clx_add's sum kernels as they are, run over (d_data, d_out) with a table in clx_add's form.
//
// Up to five launches on one stream, each reading what the one before left:
//   fir     clx_k_reverb                        the direct form: y[t] = the ascending-k fmaf chain of h[k] x[t - k]; padding becomes
//                                               +0.0, a window without a response is copied
//   sum     clx_k_add_sum / clx_k_add_sum_tc    (keep_power) per (window, x or y, row, chunk) the sum of the squared live cells
//   gain    clx_k_reverb_gain                   (keep_power or d_gains) one lane per window: Ex, Ey, g = (float)sqrt(Ex / Ey)
//   scale   clx_k_reverb_scale                  (keep_power) y = y * g over the live cells of the windows with g != 1
// The per-call table (clx_reverb_fill, uploaded once): clx_add's q, Vs, Vn, j (q unused, Vs = valid, Vn = valid where the window's
// power is kept and 0 elsewhere, j = k: the "noise" of window k is window k of d_out), then len (the response's live taps, 0: none)
// and idx (its row of d_ir) as 32-bit words, then (device only) g.
//
// The FIR.  A block is one tile of kTile = 2048 consecutive outputs of one row of one window; lane l of its 256 holds the kRun = 8
// outputs t0 + 8 l .. t0 + 8 l + 7 in registers.  The response goes by in chunks of kChunk = 256 taps, ascending.  For chunk c0 the
// block stages once, in LDS, the taps h[c0 .. c0 + 255] (H) and the source span x[t0 - c0 - 256 .. t0 - c0 + 2047] (S, 2304 words;
// samples before the crop and at or behind valid[k] are not loaded and count as +0.0, taps at or behind the live count are not
// loaded): with TC the stride-`rows` loads happen here, once per word, and the inner loop is the same for both layouts.  Inside a
// chunk the taps go in groups of eight: a lane reads the eight taps (two 16-byte loads of one address a wave: a broadcast) and the
// eight source words its window gains (two 16-byte loads), and then runs 64 fused multiply-adds out of a 16-word register window --
// tap j of the group on output i takes word 8 + i - j --, whose upper half is the group's and whose lower half becomes the next
// group's (the two halves swap roles, nothing is moved).  A lane's two loads are 32 bytes apart from its neighbour's: S is kept
// with bit 0 of a 16-byte slot's number flipped where bit 4 is set, so that the sixteen lanes the hardware serves together always
// hit sixteen different slots of the 64 banks.  A group whose taps are all live and reach no output's t < k runs unconditionally
// (the fast form); the groups of the first 2048 / 256 = 8 chunks that reach before the crop, and a last ragged group, test every
// (tap, output) pair and skip -- not multiply by zero -- where k > t or k is no live tap.  Chunks ascend and taps inside them ascend,
// so every output's chain is the definition's.  The outputs leave through S: lane l then stores t0 + l, t0 + l + 256, .., 256
// contiguous bytes a wave for CT.  LDS: 2304 + 256 words = 10 240 bytes.
//
// clx_reverb_check and clx_reverb_fill are the host side (plain C++, shared with the wave simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include "../../include/claxon_hip.h"

// the launch shape clx_reverb_check gives (n_tiles == 0: nothing to launch)
struct clx_reverb_plan {
    uint32_t n_tiles = 0;        // tiles of a row in the FIR (n_windows * rows * n_tiles blocks)
    uint32_t tc = 0;             // 1: the windows are [T][rows] with rows > 1
    uint32_t power = 0;          // 1: the sum and scale passes run (keep_power, and some window has a response and a live sample)
    uint32_t n_chunks = 0;       // clx_add's sum pass: chunks of the time axis,
    uint64_t units = 0;          // ... its waves
    uint32_t sum_blocks = 0;     // ... and its blocks
    uint32_t gain_blocks = 0;    // blocks of the gain step
    uint32_t lines = 0;          // the scale pass: lines of a window (CT: its rows; TC: one),
    uint64_t line_len = 0;       // ... their cells,
    uint32_t mult = 0;           // ... the live cells of a line per live time step,
    uint32_t scale_tiles = 0;    // ... and the tiles of a line (n_windows * lines * scale_tiles blocks)
    uint64_t partials = 0;       // doubles of the per-call table of sums: [n_windows][2][rows][n_chunks]
};

namespace clx_reverb {

using clx_norm::f4;
constexpr uint32_t kThreads = 256u, kRun = 8u, kTile = kThreads * kRun, kChunk = 256u, kGroup = 8u;
constexpr uint32_t kSpan = kTile + kChunk;                       // words of S
constexpr uint32_t kLdsBytes = (kSpan + kChunk) * 4u;            // 10 240
constexpr uint32_t kMaxRows = 8u, kMaxTaps = 65536u, kScaleCells = 4096u;
constexpr uint32_t kTableBytes = 28u, kTableBytesDevice = 32u;   // a window's share of the per-call table: host staging / device
static_assert(kChunk == kThreads, "a lane stages one tap of a chunk");
static_assert(kChunk % (2u * kGroup) == 0u && kSpan % 8u == 0u, "groups come in pairs, and the slot swizzle stays inside S");

#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
#else
inline float mul_rn(float a, float b) { return a * b; }
#endif
using clx_add::fma_rn;

// the per-call table of n windows: clx_add's, then the responses
struct table { clx_add::table a; const uint32_t* len; const int32_t* idx; };
__host__ __device__ __forceinline__ table table_of(const void* tab, size_t n) {
    table t;
    t.a = clx_add::table_of(tab, n);
    t.len = (const uint32_t*)(t.a.j + n);
    t.idx = (const int32_t*)(t.len + n);
    return t;
}

// where word m of the source span lies in S: the 16-byte slot m / 4 with bit 0 flipped where bit 4 is set
__device__ __forceinline__ uint32_t swz(uint32_t m) {
    const uint32_t s = m >> 2;
    return ((s ^ ((s >> 4) & 1u)) << 2) | (m & 3u);
}

// Eight taps, kk .. kk + 7 of the chunk at c0, on a lane's eight outputs t .. t + 7.  cur: the words x[t + q - c0 - kk], q = 0..7;
// nw receives x[t + q - c0 - kk - 8] (word m0 + q of S), the next group's cur.  kFast: every tap is live (kk + 8 <= n) and
// reaches no output's t < k; else each pair is tested.
template <bool kFast>
__device__ __forceinline__ void group(float (&acc)[kRun], float (&nw)[kGroup], const float (&cur)[kGroup], const float* S, const float* H,
                                      uint32_t m0, uint32_t kk, uint32_t n, uint64_t t, uint64_t k0) {
    const f4 a = *reinterpret_cast<const f4*>(S + swz(m0)), b = *reinterpret_cast<const f4*>(S + swz(m0 + 4u));
    const f4 ha = *reinterpret_cast<const f4*>(H + kk), hb = *reinterpret_cast<const f4*>(H + kk + 4u);
    float h[kGroup];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) { nw[q] = a[q]; nw[q + 4u] = b[q]; h[q] = ha[q]; h[q + 4u] = hb[q]; }
#pragma unroll
    for (uint32_t j = 0; j < kGroup; ++j) {
        if (!kFast && kk + j >= n) break;                      // (the whole block)
#pragma unroll
        for (uint32_t i = 0; i < kRun; ++i) {
            const float w = i >= j ? cur[i - j] : nw[kGroup + i - j];
            if (kFast || t + i >= k0 + j) acc[i] = fma_rn(h[j], w, acc[i]);
        }
    }
}

}  // namespace clx_reverb

// Block b: tile b % n_tiles of row (b / n_tiles) % rows of window b / (n_tiles * rows); x and out are [n_windows][rows][T] (tc == 0)
// or [n_windows][T][rows] (tc == 1), ir is [..][K].
extern "C" __global__ __launch_bounds__(256) void clx_k_reverb(const float* __restrict__ x, const float* __restrict__ ir, const void* __restrict__ tab,
                                                               float* __restrict__ out, uint32_t n_windows, uint32_t rows, uint32_t T, uint32_t K,
                                                               uint32_t tc, uint32_t n_tiles) {
    using namespace clx_reverb;
    __shared__ __attribute__((aligned(16))) float S[kSpan];
    __shared__ __attribute__((aligned(16))) float H[kChunk];
    const uint32_t tid = threadIdx.x;
    const uint32_t tl = blockIdx.x % n_tiles, kr = blockIdx.x / n_tiles, k = kr / rows, r = kr - k * rows;
    const table tb = table_of(tab, n_windows);
    const uint32_t v = tb.a.vs[k], len = tb.len[k];
    const uint64_t stride = tc ? rows : 1u;
    const uint64_t base = tc ? (uint64_t)k * rows * T + r : ((uint64_t)k * rows + r) * T;
    const float* const xr = x + base;
    float* const yr = out + base;
    const uint64_t t0 = (uint64_t)tl * kTile;
    if (len == 0u || t0 >= v) {                                // (the whole block) no response: a copy; behind the live part: zeros
#pragma unroll
        for (uint32_t i = 0; i < kRun; ++i) {
            const uint64_t t = t0 + tid + i * kThreads;
            if (t < T) yr[t * stride] = t < v ? xr[t * stride] : 0.f;
        }
        return;
    }
    const float* const h = ir + (uint64_t)(uint32_t)tb.idx[k] * K;
    const uint64_t live_end = t0 + kTile < v ? t0 + kTile : v;                    // the tile's live outputs are t0 <= t < live_end
    const uint32_t nk = len < live_end ? len : (uint32_t)live_end;                // ... and reach the taps k < nk
    const uint64_t t = t0 + (uint64_t)tid * kRun;                                 // the lane's first output
    float acc[kRun] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    for (uint32_t c0 = 0; c0 < nk; c0 += kChunk) {
        const int64_t b = (int64_t)t0 - (int64_t)c0 - (int64_t)kChunk;            // the sample in word 0 of S
#pragma unroll
        for (uint32_t i = 0; i < kSpan / kThreads; ++i) {
            const uint32_t m = tid + i * kThreads;
            const int64_t s = b + m;
            S[swz(m)] = s >= 0 && (uint64_t)s < v ? xr[(uint64_t)s * stride] : 0.f;
        }
        H[tid] = c0 + tid < nk ? h[c0 + tid] : 0.f;
        __syncthreads();
        const uint32_t n = nk - c0 < kChunk ? nk - c0 : kChunk;                   // the chunk's live taps
        float w0[kGroup], w1[kGroup];
        {
            const f4 a = *reinterpret_cast<const f4*>(S + swz(kChunk + tid * kRun)), c = *reinterpret_cast<const f4*>(S + swz(kChunk + tid * kRun + 4u));
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) { w1[q] = a[q]; w1[q + 4u] = c[q]; }
        }
        for (uint32_t kk = 0; kk < n; kk += 2u * kGroup) {
            const uint32_t m0 = kChunk + tid * kRun - kk - kGroup;
            const uint64_t k0 = (uint64_t)c0 + kk;
            if (kk + kGroup <= n && t0 >= k0 + kGroup - 1u) group<true>(acc, w0, w1, S, H, m0, kk, n, t, k0);
            else group<false>(acc, w0, w1, S, H, m0, kk, n, t, k0);
            if (kk + kGroup >= n) break;                       // (the whole block)
            if (kk + 2u * kGroup <= n && t0 >= k0 + 2u * kGroup - 1u) group<true>(acc, w1, w0, S, H, m0 - kGroup, kk + kGroup, n, t, k0 + kGroup);
            else group<false>(acc, w1, w0, S, H, m0 - kGroup, kk + kGroup, n, t, k0 + kGroup);
        }
        __syncthreads();                                       // (the chunk has been read)
    }
    *reinterpret_cast<f4*>(S + tid * kRun) = f4{ acc[0], acc[1], acc[2], acc[3] };
    *reinterpret_cast<f4*>(S + tid * kRun + 4u) = f4{ acc[4], acc[5], acc[6], acc[7] };
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < kRun; ++i) {
        const uint64_t to = t0 + tid + i * kThreads;
        if (to < T) yr[to * stride] = to < v ? S[tid + i * kThreads] : 0.f;
    }
}

// Lane k of the grid: window k's gain, into gain (the context's) and gains (the caller's, may be null).  part may be null where
// every Vn is 0.
extern "C" __global__ __launch_bounds__(256) void clx_k_reverb_gain(const void* __restrict__ tab, const double* __restrict__ part, float* gain,
                                                                    float* gains, uint32_t n_windows, uint32_t rows, uint32_t n_chunks) {
    using namespace clx_norm;
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n_windows) return;
    const clx_reverb::table t = clx_reverb::table_of(tab, n_windows);
    const uint32_t vn = t.a.vn[k];
    float g = 1.f;
    if (vn != 0u) {
        const double* const P = part + k * 2u * rows * n_chunks;
        const uint32_t live = live_chunks(vn);
        double ex = 0.0, ey = 0.0;
        for (uint32_t r = 0; r < rows; ++r) {
            ex = dadd_rn(ex, fold_chunks(P + (uint64_t)r * n_chunks, live));
            ey = dadd_rn(ey, fold_chunks(P + (uint64_t)(rows + r) * n_chunks, live));
        }
        if (ex != 0.0 && ey != 0.0) g = to_f32(clx_add::dsqrt_rn(ddiv_rn(ex, ey)));
    }
    gain[k] = g;
    if (gains) gains[k] = g;
}

// The scale pass, in place on out.  Block b: tile b % n_tiles of line (b / n_tiles) % lines of window b / (n_tiles * lines); a line
// is line_len contiguous cells of which the first Vn * mult are live.
extern "C" __global__ __launch_bounds__(256) void clx_k_reverb_scale(float* out, const void* __restrict__ tab, const float* __restrict__ gain,
                                                                     uint32_t n_windows, uint32_t lines, uint64_t line_len, uint32_t mult,
                                                                     uint32_t n_tiles) {
    using namespace clx_reverb;
    const uint32_t tl = blockIdx.x % n_tiles, kl = blockIdx.x / n_tiles, k = kl / lines;
    const float g = gain[k];
    if (g == 1.f) return;                                      // (the whole block: the window is not rewritten)
    const uint64_t live = (uint64_t)table_of(tab, n_windows).a.vn[k] * mult, e0 = (uint64_t)tl * kScaleCells;
    if (e0 >= live) return;                                    // (the whole block)
    float* const p = out + (uint64_t)kl * line_len;
#pragma unroll
    for (uint32_t i = 0; i < kScaleCells / kThreads; ++i) {
        const uint64_t e = e0 + threadIdx.x + i * kThreads;
        if (e < live) p[e] = mul_rn(p[e], g);
    }
}

// The host side of clx_reverb_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the launch
// shape (p->n_tiles == 0: nothing to launch).
inline const char* clx_reverb_check(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const void* ir, size_t n_ir,
                                    uint32_t K, const uint32_t* ir_len, const int32_t* ir_index, uint32_t layout, const clx_reverb_opts* o,
                                    const void* out, clx_reverb_plan* p) {
    using namespace clx_reverb;
    *p = clx_reverb_plan();
    if (o && (o->keep_power > 1u || o->reserved != 0u)) return "clx_reverb_windows: opts->keep_power must be 0 or 1 and opts->reserved 0";
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return "clx_reverb_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT";
    if (rows < 1u || rows > kMaxRows) return "clx_reverb_windows: rows must be 1..8";
    if (K < 1u || K > kMaxTaps) return "clx_reverb_windows: K must be 1..65536";
    if (n_windows == 0 || T == 0) return nullptr;
    if (!data || !out || !valid || !ir_index) return "clx_reverb_windows: null argument";
    if (n_ir && (!ir || !ir_len)) return "clx_reverb_windows: null argument";
    for (size_t j = 0; j < n_ir; ++j)
        if (ir_len[j] > K) return "clx_reverb_windows: ir_len[j] is larger than K";
    bool work = false;
    for (size_t k = 0; k < n_windows; ++k) {
        if (valid[k] > T) return "clx_reverb_windows: valid[k] is larger than T";
        if (ir_index[k] < -1 || (ir_index[k] >= 0 && (uint64_t)ir_index[k] >= n_ir)) return "clx_reverb_windows: ir_index[k] must be -1 .. n_ir - 1";
        work = work || (ir_index[k] >= 0 && ir_len[ir_index[k]] != 0u && valid[k] != 0u);
    }
    const uint64_t cells = (uint64_t)rows * T, tiles = ((uint64_t)T + kTile - 1u) / kTile;
    if (n_windows > 0x7fffffffull || n_ir > 0x7fffffffull || (uint64_t)n_windows * rows * tiles > 0x7fffffffull)
        return "clx_reverb_windows: too many windows in one call";
    const uint64_t bytes = (uint64_t)n_windows * cells * 4u;
    const uintptr_t a = (uintptr_t)data, b = (uintptr_t)out;
    if (a < b + bytes && b < a + bytes) return "clx_reverb_windows: d_out overlaps d_data";
    const uint32_t tc = layout == CLX_WINDOW_TC && rows > 1u ? 1u : 0u;
    p->n_tiles = (uint32_t)tiles; p->tc = tc;
    p->gain_blocks = (uint32_t)((n_windows + kThreads - 1u) / kThreads);
    if (o && o->keep_power && work) {                          // clx_add_check's shape of the sums, and the scale pass
        const uint64_t nc = ((uint64_t)T + clx_add::kChunk - 1u) / clx_add::kChunk;
        const uint64_t partials = (uint64_t)n_windows * 2u * rows * nc, units = tc ? (uint64_t)n_windows * 2u * nc : partials;
        const uint64_t line_len = tc ? cells : T, lines = tc ? 1u : rows, st = (line_len + kScaleCells - 1u) / kScaleCells;
        if (partials > 0x7fffffffull || (uint64_t)n_windows * lines * st > 0x7fffffffull) return "clx_reverb_windows: too many windows in one call";
        p->power = 1u; p->n_chunks = (uint32_t)nc; p->units = units; p->sum_blocks = (uint32_t)((units + 3u) / 4u); p->partials = partials;
        p->lines = (uint32_t)lines; p->line_len = line_len; p->mult = tc ? rows : 1u; p->scale_tiles = (uint32_t)st;
    }
    return nullptr;
}

// The per-call table of checked arguments, kTableBytes a window, into `tab` (8-byte aligned): q, Vs, Vn, j, len, idx.
inline void clx_reverb_fill(void* tab, size_t n_windows, const uint32_t* valid, const uint32_t* ir_len, const int32_t* ir_index, uint32_t keep_power) {
    double* const q = (double*)tab;
    uint32_t* const vs = (uint32_t*)(q + n_windows);
    uint32_t* const vn = vs + n_windows;
    int32_t* const jj = (int32_t*)(vn + n_windows);
    uint32_t* const len = (uint32_t*)(jj + n_windows);
    int32_t* const idx = (int32_t*)(len + n_windows);
    for (size_t k = 0; k < n_windows; ++k) {
        const int32_t j = ir_index[k];
        q[k] = 0.0;
        vs[k] = valid[k];
        jj[k] = (int32_t)k;
        len[k] = j < 0 ? 0u : ir_len[j];
        idx[k] = j < 0 ? 0 : j;
        vn[k] = keep_power && len[k] != 0u ? valid[k] : 0u;
    }
}
