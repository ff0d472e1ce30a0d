// clx_cmvn.hip -- the two forms of cepstral mean and variance normalisation whose statistics are not the window's own: a fixed
// per-row shift and scale (global CMVN: WeNet's global_cmvn, FunASR's am.mvn, Kaldi's apply-cmvn with global stats),
// clx_cmvn_global_windows, and statistics over a sliding window of frames (Kaldi's apply-cmvn-sliding),
// clx_cmvn_sliding_windows.  claxon_hip.h has the definition; this is how it is computed.  One launch a call.
// No product fuses with a sum anywhere in this file: every operation below goes through a helper that is rounded once and is
// compiled with contraction off.
//
// The per-call table (clx_cmvn_fill_table, uploaded once) is 32-bit words: V[n], then for the global call shift[rows] and
// scale[rows].
//
// clx_k_cmvn_global: in place, streaming; clx_k_norm_apply's tiling.  Block = tile of kVecs = 1024 16-byte vectors of the window's
// 16-byte grid: a vector that lies whole inside the window is one 16-byte store, and one 16-byte load when all four of its cells
// are live; the ragged head and tail of a window and the vectors that hold padding go cell by cell on the load side, so no cell
// with t >= V is read.  A lane finds (row, t) of its vector's first cell with one division and steps from there.  A live cell is
// mul_rn(add_rn(x, shift[r]), scale[r]); shift and scale come from the table (8192 rows at most: 64 KiB, cache resident), so the
// kernel uses 0 bytes of LDS.  CT and TC differ in the index arithmetic alone.
//
// clx_k_cmvn_sliding: out of place.  Block = tile of kTile = 256 output frames [t0, t1) of one window.  A tile with t0 >= V writes
// the pad and stages nothing.  Otherwise, with `last` the tile's last live frame, the tile's source span is the frames
// [lo, hi) = [32 floor(a(t0) / 32), b(last)) -- a() and b() of clx_cmvn::stat_window never decrease with t, and b - a <= N + 1, so
// the span is at most 31 + 255 + 1025 = 1311 frames (claxon_hip.h allows kSpan = 1344: 42 groups of 32) and
// lies inside [0, V).  The rows go in chunks of kRc = 8:
//   stage   the chunk's rows of the span into LDS as floats, one global load a cell.  Frame i of the span stands at word
//           pos(i) = i + i / 32 (one spare word behind every group of 32 frames, so that lanes which walk different groups at the
//           same step hit different banks); CT keeps [row][pos] with rows kRowStride = 1351 apart (odd), TC keeps [pos][row].
//   groups  one lane a (group, row): G = the double sum of the group's 32 cells ascending from +0.0, H the same over the squares
//           (exact in double).  Only the groups that lie whole inside [lo, hi) are summed: no statistics window uses another one.
//   sweep   one lane a cell, lanes along the contiguous axis of the output (frames in CT, rows in TC): S and Q in the ORDER of
//           claxon_hip.h -- the cells in front of the first whole group one by one, the whole groups, the cells behind them --
//           then the cell.  About 62 cell additions and 32 group additions at most, against 1025.
// The ORDER is a function of (a, b, V) alone: groups are cut from frame 0 of the window, not from the tile or the span.
// LDS: 8 x 1351 floats + 2 x 8 x 42 doubles = 48 608 bytes: three workgroups a CU.  No scratch, no spills, wave64, blocks of 256
// (tests/test_code_object_cmvn.py reads them from the code object).
//
// clx_cmvn_check_global, clx_cmvn_check_sliding, clx_cmvn_fill_table and clx_cmvn_from_stats_build are the host side (plain C++,
// shared with the wave simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include "../../include/claxon_hip.h"

// the launch shape clx_cmvn_check_global / clx_cmvn_check_sliding give (n_tiles == 0: nothing to launch)
struct clx_cmvn_plan {
    uint32_t n_tiles = 0;        // tiles of a window (n_windows * n_tiles blocks)
    uint32_t tc = 0;             // 1: [n_windows][T][rows]
    uint32_t Rc = 0;             // sliding: rows staged at once
    uint32_t span = 0;           // sliding: the most frames a tile of this call stages
    uint64_t table_words = 0;    // 32-bit words of the per-call table
};

namespace clx_cmvn {

constexpr uint32_t kThreads = 256u, kTile = 256u, kVecs = 1024u, kMaxRows = 8192u, kMaxT = 0x7fffffffu, kMaxWindow = 1024u, kGroup = 32u;
constexpr uint32_t kSpan = kTile + kMaxWindow + 2u * kGroup;                    // 1344 frames
constexpr uint32_t kGroups = kSpan / kGroup;                                    // 42
constexpr uint32_t kMaxSpan = (kGroup - 1u) + (kTile - 1u) + (kMaxWindow + 1u); // 1311: what a tile can span
constexpr uint32_t kRowStride = ((kMaxSpan - 1u) + (kMaxSpan - 1u) / kGroup + 1u) | 1u;   // 1351: the last frame's word, plus one, made odd
constexpr uint32_t kRc = 8u;
constexpr uint32_t kSlidingLdsBytes = ((kRc * kRowStride * 4u + 7u) & ~7u) + 2u * kRc * kGroups * 8u;   // 48 608 (the doubles stand on a multiple of 8)
constexpr uint32_t kGlobalLdsBytes = 0u;
static_assert(kMaxSpan <= kSpan, "a tile's span fits what the definition allows");
static_assert(kRowStride == 1351u && kSlidingLdsBytes == 48608u, "the header states these");
static_assert(3u * kSlidingLdsBytes <= 160u * 1024u, "three workgroups a CU");
static_assert(kTile == kThreads, "a CT sweep of a whole tile has one lane a frame");

#if defined(__clang__)
typedef float f4 __attribute__((ext_vector_type(4)));
#else
typedef float f4 __attribute__((vector_size(16)));
#endif

// float32 and float64 operations that are each rounded once and never contracted: the device compiler contracts a * b + c into
// one fused operation where it sees a product feed a sum, so every helper switches contraction off for the operation it holds
// (the wave simulator's host build is compiled without contraction).  The square root and the divisions are the correctly rounded
// ones (the library is built without fast-math).
#if defined(__HIP__) || defined(__HIPCC__)
#define CLX_CMVN_OP(type, name, expr) \
    __device__ __forceinline__ type name(type a, type b) { _Pragma("clang fp contract(off)") return expr; }
__device__ __forceinline__ double dsqrt_rn(double a) { return __dsqrt_rn(a); }
__device__ __forceinline__ float to_f32(double a) { return __double2float_rn(a); }
#else
#define CLX_CMVN_OP(type, name, expr) \
    inline type name(type a, type b) { return expr; }
inline double dsqrt_rn(double a) { return sqrt(a); }
inline float to_f32(double a) { return (float)a; }
#endif
CLX_CMVN_OP(float, add_rn, a + b)
CLX_CMVN_OP(float, mul_rn, a * b)
CLX_CMVN_OP(double, dadd_rn, a + b)
CLX_CMVN_OP(double, dsub_rn, a - b)
CLX_CMVN_OP(double, dmul_rn, a * b)
CLX_CMVN_OP(double, ddiv_rn, a / b)
#undef CLX_CMVN_OP

__device__ __forceinline__ float as_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// The statistics window [a, b) of live frame t < V (claxon_hip.h: Kaldi's SlidingWindowCmnInternal as this project reads it).
// N = window, M = min_window (only read when center == 0).  0 <= a < b <= V, b - a <= N + 1, and neither a nor b decreases with t.
__host__ __device__ __forceinline__ void stat_window(uint32_t t, uint32_t V, uint32_t N, uint32_t M, uint32_t center, uint32_t* pa, uint32_t* pb) {
    int64_t a, b;
    if (center) { a = (int64_t)t - (int64_t)(N / 2u); b = a + (int64_t)N; }
    else { a = (int64_t)t - (int64_t)N; b = (int64_t)t + 1; }
    if (a < 0) { b -= a; a = 0; }
    if (!center && b > (int64_t)t) b = (int64_t)t + 1 > (int64_t)M ? (int64_t)t + 1 : (int64_t)M;
    if (b > (int64_t)V) { a -= b - (int64_t)V; b = (int64_t)V; if (a < 0) a = 0; }
    *pa = (uint32_t)a; *pb = (uint32_t)b;
}

// the word of frame i of a staged span: one spare word behind every group
__device__ __forceinline__ uint32_t pos(uint32_t i) { return i + i / kGroup; }

}  // namespace clx_cmvn

// Block b: tile b % n_tiles of window b / n_tiles, in place; the window's rows * T cells lie [rows][T] (tc == 0) or [T][rows]
// (tc == 1).  tab: V[n_windows], shift[rows], scale[rows].  pad is the word of every cell with t >= V.
extern "C" __global__ __launch_bounds__(256) void clx_k_cmvn_global(float* x, const uint32_t* __restrict__ tab, uint32_t n_windows, uint32_t rows,
                                                                    uint32_t T, float pad, uint32_t tc, uint32_t n_tiles) {
    using namespace clx_cmvn;
    const uint32_t tid = threadIdx.x, k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const uint64_t cells = (uint64_t)rows * T;
    float* const w = x + (uint64_t)k * cells;
    const uint32_t head = (uint32_t)(((uintptr_t)w >> 2) & 3u);
    const uint64_t vectors = (cells + head + 3u) >> 2;
    const uint64_t v_lo = (uint64_t)tl * kVecs;
    if (v_lo >= vectors) return;                               // (the whole block: n_tiles is sized for the largest head)
    const uint64_t v_hi = v_lo + kVecs < vectors ? v_lo + kVecs : vectors;
    const uint32_t n = tab[k];
    const uint32_t* const shift = tab + n_windows;
    const uint32_t* const scale = shift + rows;
    const uint32_t inner = tc ? rows : T;                      // the cells of the faster axis
    for (uint32_t i = 0; i < kVecs / kThreads; ++i) {
        const uint64_t v = v_lo + i * kThreads + tid;
        if (v >= v_hi) break;
        const int64_t e0 = (int64_t)(v * 4u) - (int64_t)head;
        float* const p = w + e0;                               // 16-byte aligned
        const uint64_t e = e0 < 0 ? 0u : (uint64_t)e0;         // the vector's first cell of the window: cell b of line a
        uint32_t a, b;
        if (cells <= 0xffffffffull) { a = (uint32_t)e / inner; b = (uint32_t)e - a * inner; }
        else { a = (uint32_t)(e / inner); b = (uint32_t)(e - (uint64_t)a * inner); }
        const bool whole = e0 >= 0 && (uint64_t)e0 + 4u <= cells;
        uint32_t r[4], live = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = 0u;
            if (e0 + j < 0 || (uint64_t)(e0 + j) >= cells) continue;
            r[j] = tc ? b : a;
            if ((tc ? a : b) < n) live |= 1u << j;
            if (++b == inner) { b = 0u; ++a; }
        }
        f4 q = { pad, pad, pad, pad };
        if (live == 15u && whole) q = *reinterpret_cast<const f4*>(p);
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live >> j & 1u) q[j] = p[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (live >> j & 1u) q[j] = mul_rn(add_rn(q[j], as_f32(shift[r[j]])), as_f32(scale[r[j]]));
        if (whole) *reinterpret_cast<f4*>(p) = q;
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j >= 0 && (uint64_t)(e0 + j) < cells) p[j] = q[j];
        }
    }
}

// Block b: tile b % n_tiles of window b / n_tiles.  tab: V[n_windows].  pad is the word of every frame from V on.
extern "C" __global__ __launch_bounds__(256) void clx_k_cmvn_sliding(const float* __restrict__ in, float* __restrict__ out,
                                                                     const uint32_t* __restrict__ tab, uint32_t rows, uint32_t T, uint32_t N, uint32_t M,
                                                                     uint32_t center, uint32_t norm_vars, float pad, uint32_t tc, uint32_t n_tiles) {
    using namespace clx_cmvn;
    __shared__ float s_x[kRc * kRowStride];
    __shared__ double s_g[kRc * kGroups];
    __shared__ double s_h[kRc * kGroups];
    const uint32_t tid = threadIdx.x, k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const uint32_t V = tab[k];
    const uint32_t t0 = tl * kTile, t1 = T - t0 < kTile ? T : t0 + kTile, nf = t1 - t0;
    const float* const x = in + (uint64_t)k * rows * T;
    float* const y = out + (uint64_t)k * rows * T;
    if (t0 >= V) {                                             // (the whole block) only the pad
        if (tc) {
            const uint64_t e0 = (uint64_t)t0 * rows, n = (uint64_t)nf * rows;
            for (uint64_t e = tid; e < n; e += kThreads) y[e0 + e] = pad;
        } else if (tid < nf) {
            for (uint32_t r = 0; r < rows; ++r) y[(uint64_t)r * T + t0 + tid] = pad;
        }
        return;
    }
    const uint32_t live = V - t0 < nf ? V - t0 : nf;
    uint32_t lo, hi, unused;
    stat_window(t0, V, N, M, center, &lo, &unused);
    stat_window(t0 + live - 1u, V, N, M, center, &unused, &hi);
    lo = lo / kGroup * kGroup;
    const uint32_t n_span = hi - lo, ng = n_span / kGroup, g_lo = lo / kGroup;     // (n_span <= kMaxSpan; ng whole groups, each inside [0, V))
    for (uint32_t r0 = 0; r0 < rows; r0 += kRc) {              // (every bound of these loops is the whole block's)
        const uint32_t rc = rows - r0 < kRc ? rows - r0 : kRc;
        if (!tc) {
            for (uint32_t rl = 0; rl < rc; ++rl) {
                const float* const row = x + (uint64_t)(r0 + rl) * T + lo;
                for (uint32_t i = tid; i < n_span; i += kThreads) s_x[rl * kRowStride + pos(i)] = row[i];
            }
        } else {
            const uint32_t n = n_span * rc;
            for (uint32_t e = tid; e < n; e += kThreads) {
                const uint32_t i = e / rc, rl = e - i * rc;
                s_x[pos(i) * rc + rl] = x[(uint64_t)(lo + i) * rows + r0 + rl];
            }
        }
        __syncthreads();
        for (uint32_t e = tid; e < ng * rc; e += kThreads) {   // the groups: lanes along the groups (CT) or the rows (TC)
            const uint32_t g = tc ? e / rc : e % ng, rl = tc ? e % rc : e / ng;
            double G = 0.0, H = 0.0;
            for (uint32_t j = 0; j < kGroup; ++j) {
                const uint32_t w = pos(g * kGroup + j);
                const double v = (double)s_x[tc ? w * rc + rl : rl * kRowStride + w];
                G = dadd_rn(G, v);
                H = dadd_rn(H, dmul_rn(v, v));
            }
            s_g[tc ? g * rc + rl : rl * kGroups + g] = G;
            s_h[tc ? g * rc + rl : rl * kGroups + g] = H;
        }
        __syncthreads();
        for (uint32_t e = tid; e < nf * rc; e += kThreads) {   // the sweep: lanes along the frames (CT) or the rows (TC)
            const uint32_t fl = tc ? e / rc : e % nf, rl = tc ? e % rc : e / nf, t = t0 + fl;
            float cell = pad;
            if (fl < live) {
                uint32_t a, b;
                stat_window(t, V, N, M, center, &a, &b);
                const uint32_t ka = (a + kGroup - 1u) / kGroup, kb = b / kGroup;
                const uint32_t e1 = ka <= kb ? ka * kGroup : b;          // the cells [a, e1) one by one, then the groups, then [e2, b)
                const uint32_t e2 = ka <= kb ? kb * kGroup : b;
                double S = 0.0, Q = 0.0;
                for (uint32_t u = a; u < e1; ++u) {
                    const uint32_t w = pos(u - lo);
                    const double v = (double)s_x[tc ? w * rc + rl : rl * kRowStride + w];
                    S = dadd_rn(S, v);
                    if (norm_vars) Q = dadd_rn(Q, dmul_rn(v, v));
                }
                if (ka < kb) {
                    for (uint32_t g = ka - g_lo; g < kb - g_lo; ++g) {
                        S = dadd_rn(S, s_g[tc ? g * rc + rl : rl * kGroups + g]);
                        if (norm_vars) Q = dadd_rn(Q, s_h[tc ? g * rc + rl : rl * kGroups + g]);
                    }
                }
                for (uint32_t u = e2; u < b; ++u) {
                    const uint32_t w = pos(u - lo);
                    const double v = (double)s_x[tc ? w * rc + rl : rl * kRowStride + w];
                    S = dadd_rn(S, v);
                    if (norm_vars) Q = dadd_rn(Q, dmul_rn(v, v));
                }
                const uint32_t n = b - a, wt = pos(t - lo);
                const double m = ddiv_rn(S, (double)n);
                double yv = dsub_rn((double)s_x[tc ? wt * rc + rl : rl * kRowStride + wt], m);
                if (norm_vars && n > 1u) {
                    double v = dsub_rn(ddiv_rn(Q, (double)n), dmul_rn(m, m));
                    v = v < 1e-10 ? 1e-10 : v;
                    yv = ddiv_rn(yv, dsqrt_rn(v));
                }
                cell = to_f32(yv);
            }
            if (tc) y[(uint64_t)t * rows + r0 + rl] = cell;
            else y[(uint64_t)(r0 + rl) * T + t] = cell;
        }
        __syncthreads();                                       // (the stage has been read)
    }
}

// What both calls refuse alike; `who` is 0 for the global call and 1 for the sliding one.
#define CLX_CMVN_WHO(text) (who ? "clx_cmvn_sliding_windows: " text : "clx_cmvn_global_windows: " text)
inline const char* clx_cmvn_check_common(int who, uint32_t reserved, float pad, uint32_t layout, uint32_t rows, uint32_t T) {
    using namespace clx_cmvn;
    if (reserved != 0u) return CLX_CMVN_WHO("reserved must be 0");
    if (!std::isfinite(pad)) return CLX_CMVN_WHO("pad must be finite");
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return CLX_CMVN_WHO("layout must be CLX_WINDOW_TC or CLX_WINDOW_CT");
    if (rows < 1u || rows > kMaxRows) return CLX_CMVN_WHO("rows must be 1..8192");
    if (T > kMaxT) return CLX_CMVN_WHO("T must be below 2^31");
    return nullptr;
}

// The host side of clx_cmvn_global_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the
// launch shape (p->n_tiles == 0: nothing to launch).
inline const char* clx_cmvn_check_global(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                         const float* shift, const float* scale, const clx_cmvn_global_opts* o, clx_cmvn_plan* p) {
    using namespace clx_cmvn;
    *p = clx_cmvn_plan();
    if (!o) return "clx_cmvn_global_windows: null options";
    if (const char* why = clx_cmvn_check_common(0, o->reserved, o->pad, layout, rows, T)) return why;
    if (!shift) return "clx_cmvn_global_windows: null shift";
    if (!scale) return "clx_cmvn_global_windows: null scale";
    for (uint32_t r = 0; r < rows; ++r) {
        if (!std::isfinite(shift[r])) return "clx_cmvn_global_windows: shift must be finite";
        if (!std::isfinite(scale[r])) return "clx_cmvn_global_windows: scale must be finite";
    }
    if (n_windows == 0 || T == 0) return nullptr;
    if (!data || !valid) return "clx_cmvn_global_windows: null argument";
    for (size_t k = 0; k < n_windows; ++k)
        if (valid[k] > T) return "clx_cmvn_global_windows: valid[k] is larger than T";
    const uint64_t cells = (uint64_t)rows * T, tiles = (((cells + 6u) >> 2) + kVecs - 1u) / kVecs;   // (at most (cells + 6) / 4 vectors)
    if (n_windows > 0x7fffffffull || tiles * (uint64_t)n_windows > 0x7fffffffull) return "clx_cmvn_global_windows: too many tiles in one call";
    p->n_tiles = (uint32_t)tiles; p->tc = layout == CLX_WINDOW_TC ? 1u : 0u;
    p->table_words = (uint64_t)n_windows + 2u * (uint64_t)rows;
    return nullptr;
}

// The host side of clx_cmvn_sliding_windows, likewise.
inline const char* clx_cmvn_check_sliding(const void* d_in, const void* d_out, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                                          uint32_t layout, const clx_cmvn_sliding_opts* o, clx_cmvn_plan* p) {
    using namespace clx_cmvn;
    *p = clx_cmvn_plan();
    if (!o) return "clx_cmvn_sliding_windows: null options";
    if (const char* why = clx_cmvn_check_common(1, o->reserved, o->pad, layout, rows, T)) return why;
    if (o->window < 1u || o->window > kMaxWindow) return "clx_cmvn_sliding_windows: window must be 1..1024";
    if (o->center > 1u) return "clx_cmvn_sliding_windows: center must be 0 or 1";
    if (o->norm_vars > 1u) return "clx_cmvn_sliding_windows: norm_vars must be 0 or 1";
    if (!o->center && (o->min_window < 1u || o->min_window > o->window)) return "clx_cmvn_sliding_windows: min_window must be 1..window";
    if (n_windows == 0 || T == 0) return nullptr;
    if (!d_in || !d_out || !valid) return "clx_cmvn_sliding_windows: null argument";
    if (d_in == d_out) return "clx_cmvn_sliding_windows: d_out must not be d_in";
    for (size_t k = 0; k < n_windows; ++k)
        if (valid[k] > T) return "clx_cmvn_sliding_windows: valid[k] is larger than T";
    const uint64_t tiles = ((uint64_t)T + kTile - 1u) / kTile;
    if (n_windows > 0x7fffffffull || tiles * (uint64_t)n_windows > 0x7fffffffull) return "clx_cmvn_sliding_windows: too many tiles in one call";
    const uint64_t span = (uint64_t)(kGroup - 1u) + (kTile - 1u) + (o->window + 1u);
    p->n_tiles = (uint32_t)tiles; p->tc = layout == CLX_WINDOW_TC ? 1u : 0u; p->Rc = rows < kRc ? rows : kRc;
    p->span = (uint32_t)(span < T ? span : T);
    p->table_words = (uint64_t)n_windows;
    return nullptr;
}
#undef CLX_CMVN_WHO

// The per-call table of checked arguments into `tab`: V, then (global: shift != nullptr) the rows' shifts and scales.
inline void clx_cmvn_fill_table(uint32_t* tab, size_t n_windows, const uint32_t* valid, uint32_t rows, const float* shift, const float* scale) {
    for (size_t k = 0; k < n_windows; ++k) tab[k] = valid[k];
    if (!shift) return;
    memcpy(tab + n_windows, shift, (size_t)rows * sizeof(float));
    memcpy(tab + n_windows + rows, scale, (size_t)rows * sizeof(float));
}

// Kaldi's CMVN accumulator, [2][rows + 1] doubles (row 0: the sums and the count, row 1: the sums of squares), as shift and scale:
// mean = sum / count, var = max(sumsq / count - mean * mean, 1e-20) (ApplyCmvn's floor), shift = (float)(-mean), scale =
// (float)(1 / sqrt(var)) or 1, everything in double, each result rounded once to float32.  nullptr: fine.
inline const char* clx_cmvn_from_stats_build(const double* stats, uint32_t rows, uint32_t norm_vars, float* shift, float* scale) {
    if (!stats || !shift || !scale) return "clx_cmvn_from_stats: null argument";
    if (rows < 1u || rows > clx_cmvn::kMaxRows) return "clx_cmvn_from_stats: rows must be 1..8192";
    if (norm_vars > 1u) return "clx_cmvn_from_stats: norm_vars must be 0 or 1";
    const double count = stats[rows];
    if (!(count > 0.0) || !std::isfinite(count)) return "clx_cmvn_from_stats: the count must be above 0";
    for (uint32_t r = 0; r < rows; ++r) {
        const double mean = stats[r] / count;
        double var = stats[(size_t)rows + 1u + r] / count - mean * mean;
        if (!(var >= 1e-20)) var = 1e-20;
        const float sh = (float)-mean, sc = norm_vars ? (float)(1.0 / sqrt(var)) : 1.f;
        if (!std::isfinite(sh) || !std::isfinite(sc)) return "clx_cmvn_from_stats: a row's statistics are not finite";
        shift[r] = sh; scale[r] = sc;
    }
    return nullptr;
}
