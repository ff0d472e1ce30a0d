// clx_specaug.hip -- SpecAugment of a dense float32 feature batch, out of place: a time warp about one frame, frequency masks and
// time masks filled with a constant or the window's mean: clx_specaug_windows.  claxon_hip.h has the definition; this is how it is
// computed.  It stands behind clx_norm.hip in clx_api.hip and takes the mean's sums from there.
//
// Launches on one stream, each reading what the one before left in tables the context keeps:
//   sum      clx_k_norm_sum / clx_k_norm_sum_tc   (fill = mean only) clx_norm's S partials of every row: the ORDER is clx_norm's
//   fill     clx_k_specaug_fill                   (fill = mean only) one lane per window: the rows' sums ascending, the division
//   apply    clx_k_specaug                        one read and one write of the batch
// The per-call table (clx_specaug_fill_table, uploaded once) is 32-bit words: V[n], then (c, w)[n], then the frequency masks
// [n][F] as clipped row ranges (lo, hi), then the time masks [n][M] as clipped frame ranges (lo, hi); behind them (device only)
// the n fills of a call whose fill is the mean.
//
// clx_k_specaug: block = tile kTile = 256 frames of one window, so its warp and masks are block-uniform.  A tile wholly in padding,
// or in a stretch that is neither warped nor touched by a mask, is a word copy (a block-uniform branch).  Otherwise lane i first
// works out frame t0 + i once: the time-masked bit, and for a warped window the four source frames and the four weights (the only
// 64-bit integer and double arithmetic of the kernel), into LDS: 4 x 256 source frames, 4 x 256 weights, 256 flags, and the
// 256-bit row mask: 9 248 bytes.  Then the sweep along the contiguous axis:
//   CT ([n_windows][rows][T]; also TC with rows == 1, the same memory): lane i keeps frame t0 + i's entry in registers and loops
//      over the rows; a wave's loads and stores of one row are 256 contiguous bytes (the four taps' loads lie within a few frames
//      of them).
//   TC ([n_windows][T][rows], rows > 1): the tile is nf * rows contiguous cells; lane i takes cells i, i + 256, .. and steps its
//      (frame, row) pair without a division; a cell's entry comes from LDS (lanes of one frame read one address), its four taps are
//      the same row of four other frames: contiguous across the lanes.
// A cell is 32-bit words throughout: a copy never passes through a float register's arithmetic, so NaN payloads survive.
//
// clx_specaug_check and clx_specaug_fill_table are the host side (plain C++, shared with the wave simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include "../../include/claxon_hip.h"

// the launch shape clx_specaug_check gives (n_tiles == 0: nothing to launch)
struct clx_specaug_plan {
    uint32_t n_tiles = 0;        // tiles of a window (n_windows * n_tiles blocks)
    uint32_t tc = 0;             // 1: the TC sweep and the TC sum kernel (layout TC with rows > 1)
    uint32_t mean = 0;           // 1: the fill is the window's mean: the sum pass and the fill step run
    uint32_t n_chunks = 0;       // chunks of the time axis (clx_norm's)
    uint32_t n_groups = 0;       // TC: row groups of a window (clx_norm's)
    uint32_t sum_blocks = 0;     // blocks of the sum pass
    uint32_t fill_blocks = 0;    // blocks of the fill step
    uint64_t partials = 0;       // doubles of the table of partial sums: clx_norm's [n_windows][rows][2][n_chunks]
    uint64_t table_words = 0;    // 32-bit words of the per-call table (host staging); the device's has n_windows more
};

namespace clx_specaug {

using clx_norm::kThreads;
constexpr uint32_t kTile = 256u, kMaxRows = 256u, kMaxMasks = 32u, kMaxT = 0x7fffffffu;
constexpr uint32_t kLdsBytes = 4u * kTile * 4u + 4u * kTile * 4u + kTile * 4u + (kMaxRows / 32u) * 4u;   // 9 248
static_assert(kTile == kThreads, "lane i of a block works out frame i of its tile");

// float32 operations that are each rounded once and never contracted, and the fused multiply-add.  The device compiler's
// __fmul_rn, __fadd_rn and __fsub_rn are the plain operators, which it contracts into one fused operation where a product feeds a
// sum: the weights are products that feed sums, so these three switch contraction off for the operation they hold (the wave
// simulator's host build is compiled without contraction).
#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float fma_rn(float a, float b, float c) { return __fmaf_rn(a, b, c); }
#else
inline float mul_rn(float a, float b) { return a * b; }
inline float add_rn(float a, float b) { return a + b; }
inline float sub_rn(float a, float b) { return a - b; }
inline float fma_rn(float a, float b, float c) { return fmaf(a, b, c); }
#endif

__device__ __forceinline__ float as_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
__device__ __forceinline__ uint32_t as_u32(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// the cubic convolution with A = -0.75, every operation one float32 rounding, none fused:
//   cub_near(x) = ((1.25 x - 2.25) x) x + 1        for |x| <= 1
//   cub_far(x)  = ((-0.75 x + 3.75) x - 6) x + 3   for 1 < |x| < 2
__device__ __forceinline__ float cub_near(float x) { return add_rn(mul_rn(mul_rn(sub_rn(mul_rn(1.25f, x), 2.25f), x), x), 1.f); }
__device__ __forceinline__ float cub_far(float x) { return add_rn(mul_rn(sub_rn(mul_rn(add_rn(mul_rn(-0.75f, x), 3.75f), x), 6.f), x), 3.f); }

// the per-call table of n windows with F frequency and M time masks
struct table { const uint32_t* valid; const uint32_t* warp; const uint32_t* fm; const uint32_t* tm; const float* fill; };
__host__ __device__ __forceinline__ table table_of(const uint32_t* tab, size_t n, uint32_t F, uint32_t M) {
    table t;
    t.valid = tab;
    t.warp = tab + n;
    t.fm = t.warp + 2u * n;
    t.tm = t.fm + 2u * n * F;
    t.fill = (const float*)(t.tm + 2u * n * M);
    return t;
}

}  // namespace clx_specaug

// Lane k of the grid: window k's mean over its live cells, into the table's fills.  part is clx_norm's [n_windows][rows][2][n_chunks].
extern "C" __global__ __launch_bounds__(256) void clx_k_specaug_fill(const uint32_t* __restrict__ valid, const double* __restrict__ part, float* fill,
                                                                     uint32_t n_windows, uint32_t rows, uint32_t n_chunks) {
    using namespace clx_norm;
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n_windows) return;
    const uint32_t n = valid[k];
    float f = 0.f;
    if (n != 0u) {
        const double* const P = part + k * rows * 2u * n_chunks;
        const uint32_t live = live_chunks(n);
        double s = 0.0;
        for (uint32_t r = 0; r < rows; ++r) s = dadd_rn(s, fold_chunks(P + (uint64_t)r * 2u * n_chunks, live));
        f = to_f32(ddiv_rn(s, (double)((uint64_t)n * rows)));
    }
    fill[k] = f;
}

// Block b: tile b % n_tiles of window b / n_tiles.  tab is the per-call table; mean != 0: the fills are the table's, else fill_c.
// d_fill (may be null) receives every window's fill.
extern "C" __global__ __launch_bounds__(256) void clx_k_specaug(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                const uint32_t* __restrict__ tab, float* d_fill, uint32_t n_windows, uint32_t rows,
                                                                uint32_t T, uint32_t F, uint32_t M, uint32_t mean, float fill_c, uint32_t tc,
                                                                uint32_t n_tiles) {
    using namespace clx_specaug;
    __shared__ uint32_t s_src[4u * kTile];
    __shared__ float s_w[4u * kTile];
    __shared__ uint32_t s_flag[kTile];                         // bit 0: the frame is time-masked; bit 1: it is live (t < V)
    __shared__ uint32_t s_rows[kMaxRows / 32u];                // bit r: row r is frequency-masked
    const uint32_t tid = threadIdx.x, k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const table tb = table_of(tab, n_windows, F, M);
    const uint32_t V = tb.valid[k], c = tb.warp[2u * k], w = tb.warp[2u * k + 1u];
    const uint32_t t0 = tl * kTile, t1 = T - t0 < kTile ? T : t0 + kTile, nf = t1 - t0;
    const uint32_t fill = as_u32(mean ? tb.fill[k] : fill_c);
    if (tl == 0u && tid == 0u && d_fill) d_fill[k] = as_f32(fill);
    const uint32_t* const fm = tb.fm + (uint64_t)k * 2u * F;
    const uint32_t* const tm = tb.tm + (uint64_t)k * 2u * M;
    const bool warped = c != w;                                // (c == w, (0, 0) included: both segments are copies)
    bool any_f = false, any_t = false;                         // block-uniform: a mask reaches a live cell of the tile
    for (uint32_t i = 0; i < F; ++i) any_f = any_f || fm[2u * i] < fm[2u * i + 1u];
    for (uint32_t i = 0; i < M; ++i) any_t = any_t || (tm[2u * i] < tm[2u * i + 1u] && tm[2u * i] < t1 && tm[2u * i + 1u] > t0);
    const uint64_t cells = (uint64_t)rows * T;
    const uint32_t* const x = in + (uint64_t)k * cells;
    uint32_t* const y = out + (uint64_t)k * cells;
    if (t0 >= V || !(warped || any_f || any_t)) {              // (the whole block) a word copy
        if (tc) {
            const uint64_t e0 = (uint64_t)t0 * rows;
            const uint32_t n = nf * rows;
            for (uint32_t e = tid; e < n; e += kThreads) y[e0 + e] = x[e0 + e];
        } else if (tid < nf) {
            for (uint32_t r = 0; r < rows; ++r) y[(uint64_t)r * T + t0 + tid] = x[(uint64_t)r * T + t0 + tid];
        }
        return;
    }
    if (tid < kMaxRows / 32u) {
        uint32_t bits = 0u;
        for (uint32_t i = 0; i < F; ++i) {
            const uint32_t lo = fm[2u * i], hi = fm[2u * i + 1u], a = lo > 32u * tid ? lo : 32u * tid, b = hi < 32u * tid + 32u ? hi : 32u * tid + 32u;
            if (a < b) bits |= (b - a == 32u ? 0xffffffffu : ((1u << (b - a)) - 1u) << (a - 32u * tid));
        }
        s_rows[tid] = bits;
    }
    {
        const uint32_t t = t0 + tid;
        uint32_t flag = 0u;
        if (t < V) {
            flag = 2u;
            for (uint32_t i = 0; i < M; ++i)
                if (t >= tm[2u * i] && t < tm[2u * i + 1u]) flag = 3u;
            if (warped && flag == 2u) {
                const uint32_t base = t < w ? 0u : c, I = t < w ? c : V - c, O = t < w ? w : V - w, j = t < w ? t : t - w;
                const int64_t num = (int64_t)(2u * (uint64_t)j + 1u) * I - (int64_t)O;
                const uint64_t den = 2u * (uint64_t)O;
                const int32_t ix = num < 0 ? -1 : (int32_t)((uint64_t)num / den);
                const uint64_t rem = (uint64_t)(num - (int64_t)ix * (int64_t)den);
                const float tx = clx_norm::to_f32(clx_norm::ddiv_rn((double)rem, (double)den));
                s_w[tid] = cub_far(add_rn(tx, 1.f));
                s_w[kTile + tid] = cub_near(tx);
                s_w[2u * kTile + tid] = cub_near(sub_rn(1.f, tx));
                s_w[3u * kTile + tid] = cub_far(sub_rn(2.f, tx));
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int32_t s = ix - 1 + q;
                    s_src[(uint32_t)q * kTile + tid] = base + (s < 0 ? 0u : ((uint32_t)s > I - 1u ? I - 1u : (uint32_t)s));
                }
            }
        }
        s_flag[tid] = flag;
    }
    __syncthreads();
    if (!tc) {
        if (tid >= nf) return;
        const uint32_t t = t0 + tid, flag = s_flag[tid];
        const bool live = (flag & 2u) != 0u, tmask = (flag & 1u) != 0u, chain = warped && flag == 2u;
        uint32_t s0 = t, s1 = t, s2 = t, s3 = t;
        float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
        if (chain) {
            s0 = s_src[tid]; s1 = s_src[kTile + tid]; s2 = s_src[2u * kTile + tid]; s3 = s_src[3u * kTile + tid];
            w0 = s_w[tid]; w1 = s_w[kTile + tid]; w2 = s_w[2u * kTile + tid]; w3 = s_w[3u * kTile + tid];
        }
#pragma unroll 2
        for (uint32_t r = 0; r < rows; ++r) {
            const uint32_t* const row = x + (uint64_t)r * T;
            const bool rmask = (s_rows[r >> 5] >> (r & 31u)) & 1u;   // (the whole block)
            uint32_t v;
            if (live && (tmask || (any_f && rmask))) v = fill;
            else if (chain) {
                float acc = fma_rn(w0, as_f32(row[s0]), 0.f);
                acc = fma_rn(w1, as_f32(row[s1]), acc);
                acc = fma_rn(w2, as_f32(row[s2]), acc);
                acc = fma_rn(w3, as_f32(row[s3]), acc);
                v = as_u32(acc);
            } else v = row[t];
            y[(uint64_t)r * T + t] = v;
        }
        return;
    }
    const uint32_t n = nf * rows, qs = kThreads / rows, rs = kThreads - qs * rows;   // (rows <= 256 = kThreads)
    uint32_t f = tid / rows, r = tid - f * rows;
    const uint64_t e0 = (uint64_t)t0 * rows;
    for (uint32_t e = tid; e < n; e += kThreads) {
        const uint32_t flag = s_flag[f];
        uint32_t v;
        if ((flag & 2u) && ((flag & 1u) || (any_f && ((s_rows[r >> 5] >> (r & 31u)) & 1u)))) v = fill;
        else if (warped && flag == 2u) {
            float acc = fma_rn(s_w[f], as_f32(x[(uint64_t)s_src[f] * rows + r]), 0.f);
            acc = fma_rn(s_w[kTile + f], as_f32(x[(uint64_t)s_src[kTile + f] * rows + r]), acc);
            acc = fma_rn(s_w[2u * kTile + f], as_f32(x[(uint64_t)s_src[2u * kTile + f] * rows + r]), acc);
            acc = fma_rn(s_w[3u * kTile + f], as_f32(x[(uint64_t)s_src[3u * kTile + f] * rows + r]), acc);
            v = as_u32(acc);
        } else v = x[e0 + e];
        y[e0 + e] = v;
        f += qs; r += rs;
        if (r >= rows) { r -= rows; ++f; }
    }
}

// The host side of clx_specaug_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the
// launch shape (p->n_tiles == 0: nothing to launch).  warp is [n_windows][2] (c, w), fmasks [n_windows][F][2] (first row, width),
// tmasks [n_windows][M][2] (first frame, width); each may be null (no warp / no such masks).
inline const char* clx_specaug_check(const void* d_in, const void* d_out, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                                     uint32_t layout, const uint32_t* warp, const uint32_t* fmasks, const uint32_t* tmasks,
                                     const clx_specaug_opts* o, clx_specaug_plan* p) {
    using namespace clx_specaug;
    *p = clx_specaug_plan();
    if (!o) return "clx_specaug_windows: null options";
    if (o->reserved != 0u) return "clx_specaug_windows: reserved must be 0";
    if (o->fill_mean > 1u) return "clx_specaug_windows: fill_mean must be 0 or 1";
    if (!o->fill_mean && !std::isfinite(o->fill)) return "clx_specaug_windows: fill must be finite";
    if (o->n_freq_masks > kMaxMasks) return "clx_specaug_windows: more than 32 frequency masks";
    if (o->n_time_masks > kMaxMasks) return "clx_specaug_windows: more than 32 time masks";
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return "clx_specaug_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT";
    if (rows < 1u || rows > kMaxRows) return "clx_specaug_windows: rows must be 1..256";
    if (T > kMaxT) return "clx_specaug_windows: T must be below 2^31";
    if (n_windows == 0 || T == 0) return nullptr;
    if (!d_in || !d_out || !valid) return "clx_specaug_windows: null argument";
    if (d_in == d_out) return "clx_specaug_windows: d_out must not be d_in";
    const uint32_t F = fmasks ? o->n_freq_masks : 0u, M = tmasks ? o->n_time_masks : 0u;
    for (size_t k = 0; k < n_windows; ++k) {
        const uint32_t V = valid[k];
        if (V > T) return "clx_specaug_windows: valid[k] is larger than T";
        if (warp) {
            const uint32_t c = warp[2u * k], w = warp[2u * k + 1u];
            if (!(c == 0u && w == 0u) && (c < 1u || w < 1u || c >= V || w >= V))
                return "clx_specaug_windows: warp[k] must be (0, 0) or have c and w within 1 .. valid[k] - 1";
        }
    }
    const uint64_t tiles = ((uint64_t)T + kTile - 1u) / kTile;
    const uint64_t nc = ((uint64_t)T + clx_norm::kChunk - 1u) / clx_norm::kChunk;
    const uint32_t tc = layout == CLX_WINDOW_TC && rows > 1u ? 1u : 0u;
    const uint64_t groups = (rows + clx_norm::kTcRows - 1u) / clx_norm::kTcRows;
    const uint64_t units = (uint64_t)n_windows * rows * nc;
    const uint64_t sum_blocks = tc ? (uint64_t)n_windows * nc * groups : (units + 3u) / 4u;
    if (n_windows > 0x7fffffffull || tiles * (uint64_t)n_windows > 0x7fffffffull || (o->fill_mean && (units > 0x7fffffffull || sum_blocks > 0x7fffffffull)))
        return "clx_specaug_windows: too many windows in one call";
    p->n_tiles = (uint32_t)tiles; p->tc = tc; p->mean = o->fill_mean; p->n_chunks = (uint32_t)nc; p->n_groups = (uint32_t)groups;
    p->sum_blocks = (uint32_t)sum_blocks; p->fill_blocks = (uint32_t)((n_windows + kThreads - 1u) / kThreads);
    p->partials = o->fill_mean ? units * 2u : 0u;
    p->table_words = (uint64_t)n_windows * (3u + 2u * F + 2u * M);
    return nullptr;
}

// The per-call table of checked arguments into `tab`: V, (c, w), then every mask as a clipped range (lo, hi): rows within
// [0, rows), frames within [0, V); an empty mask is (0, 0).  F and M are the counts the table is laid out for (0 for a null array).
inline void clx_specaug_fill_table(uint32_t* tab, size_t n_windows, uint32_t rows, const uint32_t* valid, const uint32_t* warp,
                                   const uint32_t* fmasks, uint32_t F, const uint32_t* tmasks, uint32_t M) {
    uint32_t* const wp = tab + n_windows;
    uint32_t* const fm = wp + 2u * n_windows;
    uint32_t* const tm = fm + 2u * n_windows * F;
    for (size_t k = 0; k < n_windows; ++k) {
        tab[k] = valid[k];
        wp[2u * k] = warp ? warp[2u * k] : 0u;
        wp[2u * k + 1u] = warp ? warp[2u * k + 1u] : 0u;
        for (uint32_t i = 0; i < F; ++i) {
            const uint64_t lo = fmasks[(k * F + i) * 2u], hi = lo + fmasks[(k * F + i) * 2u + 1u];
            const bool some = lo < rows && hi > lo;
            fm[(k * F + i) * 2u] = some ? (uint32_t)lo : 0u;
            fm[(k * F + i) * 2u + 1u] = some ? (uint32_t)(hi < rows ? hi : rows) : 0u;
        }
        for (uint32_t i = 0; i < M; ++i) {
            const uint64_t lo = tmasks[(k * M + i) * 2u], hi = lo + tmasks[(k * M + i) * 2u + 1u];
            const bool some = lo < valid[k] && hi > lo;
            tm[(k * M + i) * 2u] = some ? (uint32_t)lo : 0u;
            tm[(k * M + i) * 2u + 1u] = some ? (uint32_t)(hi < valid[k] ? hi : valid[k]) : 0u;
        }
    }
}
