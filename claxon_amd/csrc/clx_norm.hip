// clx_norm.hip -- per-window, per-row mean and variance normalisation of a dense float32 batch, in place: clx_norm_windows.
// claxon_hip.h has the definition; this is how it is computed.
//
// Three launches on one stream, each reading what the one before left in a per-call table of double partial sums:
//   sum     clx_k_norm_sum / clx_k_norm_sum_tc     S_c, the sum of a row's cells in chunk c (kChunk = 4096 cells of the time axis)
//   square  clx_k_norm_sq / clx_k_norm_sq_tc       Q_c, the sum of the squared deviations from the mean (skipped when var == 0)
//   apply   clx_k_norm_apply                       subtract, divide, pad -- a streaming pass like clx_k_mel_range
// The order of a sum is a function of (t, n) alone: inside a chunk, strand i of kStrands = 64 adds the cells t = i mod 64 in
// ascending order from +0.0, the strands are folded by xor 32, 16, 8, 4, 2, 1 (strand i takes strand i ^ d at each step, so every
// strand ends with the same value), and whoever needs the row's sum adds the partials of the live chunks in ascending order from
// +0.0.  Strand = lane, and the fold is six shuffles of a double.  Nothing is added atomically.
//
// CT ([n_windows][rows][T]; also TC with rows == 1, which is the same memory): a wave is one chunk of one row, lane i loads t = i,
// i + 64, ..: 256 contiguous bytes a load.  Four waves a block, no LDS, no barrier.
// TC ([n_windows][T][rows], rows > 1): a block is one chunk of a group of kTcRows = 16 rows of one window.  It walks the chunk in
// tiles of 64 time steps x 16 rows: lanes run along the rows first (16 lanes cover the 64 contiguous bytes of the group at one
// time step, a wave four time steps), the tile crosses LDS (rows kTcRow = 17 floats apart: the 64 lanes that then read one row
// of the group at 64 time steps hit 64 different banks, 17 l mod 64 being a bijection), and lane l of wave w adds time step l of
// rows 4 w .. 4 w + 3 to four accumulators: the strands are the same, so is every sum.  LDS: 4 352 bytes.
// The square pass first needs the mean: every wave adds the row's S partials itself (the loads are one address a wave).
//
// Apply: block = tile of kApplyVecs = 1024 16-byte vectors of the window's 16-byte grid (clx_k_mel_range's tiling: whole vectors
// are one load and one store, the ragged head and tail go float by float).  One lane per row the tile touches (all rows for TC)
// first folds the partials into (m, s) and leaves them in LDS (2 x 256 floats = 2 048 bytes); the block that holds a row's first
// cell also writes them to stats.  A lane finds the (row, t) of its vector's first cell with one division (32-bit when the window
// has fewer than 2^32 cells) and steps from there.
//
// clx_norm_check is the host side (plain C++, shared with the wave simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>

#include "../../include/claxon_hip.h"

// the launch shape clx_norm_check gives (n_chunks == 0: nothing to launch)
struct clx_norm_plan {
    uint32_t n_chunks = 0;       // chunks of the time axis
    uint32_t tc = 0;             // 1: the TC kernels (layout TC with rows > 1)
    uint32_t n_groups = 0;       // TC: row groups of a window
    uint32_t sum_blocks = 0;     // blocks of a sum pass
    uint32_t n_tiles = 0;        // tiles of a window in the apply pass (n_windows * n_tiles blocks)
    uint64_t partials = 0;       // doubles of the per-call table: [n_windows][rows][2][n_chunks]
};

namespace clx_norm {

constexpr uint32_t kThreads = 256u, kStrands = 64u, kChunk = 4096u, kMaxRows = 256u, kTcRows = 16u, kTcRow = 17u, kApplyVecs = 1024u;
constexpr uint32_t kTcLdsBytes = kStrands * kTcRow * 4u;        // 4 352
constexpr uint32_t kApplyLdsBytes = 2u * kMaxRows * 4u;         // 2 048
static_assert(kThreads == 4u * kStrands, "a block is four waves, a wave the strands of one chunk");
static_assert(kTcRows * kStrands == 4u * kThreads, "a TC tile is four floats a lane");
static_assert(kChunk % kStrands == 0u, "a chunk is whole rounds of the strands");

#if defined(__clang__)
typedef float f4 __attribute__((ext_vector_type(4)));
#else
typedef float f4 __attribute__((vector_size(16)));
#endif

// float32 and float64 operations that are each rounded once and never contracted (the wave simulator's host build is compiled
// without contraction)
#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float sqrt_rn(float a) { return sqrtf(a); }      // (hipcc's sqrtf is correctly rounded; its __fsqrt_rn is the native one)
__device__ __forceinline__ double dadd_rn(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dmul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double ddiv_rn(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float to_f32(double a) { return __double2float_rn(a); }
#else
inline float sub_rn(float a, float b) { return a - b; }
inline float add_rn(float a, float b) { return a + b; }
inline float div_rn(float a, float b) { return a / b; }
inline float sqrt_rn(float a) { return sqrtf(a); }
inline double dadd_rn(double a, double b) { return a + b; }
inline double dmul_rn(double a, double b) { return a * b; }
inline double ddiv_rn(double a, double b) { return a / b; }
inline float to_f32(double a) { return (float)a; }
#endif

// the chunks of a row that hold a live cell
__device__ __forceinline__ uint32_t live_chunks(uint32_t n) { return (uint32_t)(((uint64_t)n + kChunk - 1u) / kChunk); }

// the partials of `live` chunks, ascending, from +0.0
__device__ __forceinline__ double fold_chunks(const double* __restrict__ p, uint32_t live) {
    double a = 0.0;
    for (uint32_t c = 0; c < live; ++c) a = dadd_rn(a, p[c]);
    return a;
}

// m = (float)(S / n), +0.0 for an empty row
__device__ __forceinline__ float mean_of(const double* __restrict__ ps, uint32_t n) {
    return n ? to_f32(ddiv_rn(fold_chunks(ps, live_chunks(n)), (double)n)) : 0.f;
}

// s = sqrtf(v + eps), v = (float)(Q / (n - ddof)), +0.0 where n <= ddof
__device__ __forceinline__ float scale_of(const double* __restrict__ pq, uint32_t n, uint32_t ddof, float eps) {
    const float v = n > ddof ? to_f32(ddiv_rn(fold_chunks(pq, live_chunks(n)), (double)(n - ddof))) : 0.f;
    return sqrt_rn(add_rn(v, eps));
}

// the strands' fold: every lane ends with the same value
__device__ __forceinline__ double fold_strands(double a) {
    a = dadd_rn(a, __shfl_xor(a, 32));
    a = dadd_rn(a, __shfl_xor(a, 16));
    a = dadd_rn(a, __shfl_xor(a, 8));
    a = dadd_rn(a, __shfl_xor(a, 4));
    a = dadd_rn(a, __shfl_xor(a, 2));
    a = dadd_rn(a, __shfl_xor(a, 1));
    return a;
}

// one cell's term: the cell itself, or the square of its deviation from m (exact in double)
template <bool kSq>
__device__ __forceinline__ double term(float x, float m) {
    if (!kSq) return (double)x;
    const double d = (double)sub_rn(x, m);
    return dmul_rn(d, d);
}

// Wave u of the grid: chunk u % n_chunks of row u / n_chunks (rows counted through the batch: window * rows + row).  part is
// [n_windows * rows][2][n_chunks]: S partials, then Q partials.  A chunk without a live cell is neither read nor written.
template <bool kSq>
__device__ __forceinline__ void sum_ct(const float* __restrict__ x, const uint32_t* __restrict__ valid, double* part, uint32_t rows, uint32_t T,
                                       uint32_t n_chunks, uint64_t units) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t u = (uint64_t)blockIdx.x * (kThreads / kStrands) + (threadIdx.x >> 6);
    if (u >= units) return;                                    // (the whole wave)
    const uint64_t kr = u / n_chunks;
    const uint32_t c = (uint32_t)(u - kr * n_chunks), n = valid[kr / rows];
    const uint64_t t0 = (uint64_t)c * kChunk;
    if (t0 >= n) return;                                       // (the whole wave)
    double* const P = part + kr * 2u * n_chunks;
    const float m = kSq ? mean_of(P, n) : 0.f;
    const float* const row = x + kr * T;
    const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
    double acc = 0.0;
    for (uint64_t t = t0 + lane; t < end; t += kStrands) acc = dadd_rn(acc, term<kSq>(row[t], m));
    acc = fold_strands(acc);
    if (lane == 0u) P[(kSq ? n_chunks : 0u) + c] = acc;
}

// Block b: row group b % n_groups of chunk (b / n_groups) % n_chunks of window b / (n_groups * n_chunks); x is [n_windows][T][rows].
template <bool kSq>
__device__ __forceinline__ void sum_tc(const float* __restrict__ x, const uint32_t* __restrict__ valid, double* part, uint32_t rows, uint32_t T,
                                       uint32_t n_chunks, uint32_t n_groups) {
    __shared__ float s_tile[kStrands * kTcRow];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t g = blockIdx.x % n_groups, kc = blockIdx.x / n_groups, c = kc % n_chunks, k = kc / n_chunks;
    const uint32_t n = valid[k], r0 = g * kTcRows;
    const uint64_t t0 = (uint64_t)c * kChunk;
    if (t0 >= n) return;                                       // (the whole block)
    const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
    const float* const base = x + (uint64_t)k * rows * T;
    double* const P = part + ((uint64_t)k * rows + r0) * 2u * n_chunks;
    float m[4] = { 0.f, 0.f, 0.f, 0.f };
    double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
    if (kSq)
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q)
            if (r0 + 4u * w + q < rows) m[q] = mean_of(P + (uint64_t)(4u * w + q) * 2u * n_chunks, n);
    for (uint64_t ts = t0; ts < end; ts += kStrands) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t idx = tid + i * kThreads, rr = idx & (kTcRows - 1u), tt = idx / kTcRows;
            if (ts + tt < end && r0 + rr < rows) s_tile[tt * kTcRow + rr] = base[(ts + tt) * rows + r0 + rr];
        }
        __syncthreads();
        if (ts + lane < end)
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q)
                if (r0 + 4u * w + q < rows) acc[q] = dadd_rn(acc[q], term<kSq>(s_tile[lane * kTcRow + 4u * w + q], m[q]));
        __syncthreads();                                       // (the tile has been read)
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        const double a = fold_strands(acc[q]);
        if (lane == 0u && r0 + 4u * w + q < rows) P[(uint64_t)(4u * w + q) * 2u * n_chunks + (kSq ? n_chunks : 0u) + c] = a;
    }
}

}  // namespace clx_norm

extern "C" __global__ __launch_bounds__(256) void clx_k_norm_sum(const float* __restrict__ x, const uint32_t* __restrict__ valid, double* part,
                                                                 uint32_t rows, uint32_t T, uint32_t n_chunks, uint64_t units) {
    clx_norm::sum_ct<false>(x, valid, part, rows, T, n_chunks, units);
}

extern "C" __global__ __launch_bounds__(256) void clx_k_norm_sq(const float* __restrict__ x, const uint32_t* __restrict__ valid, double* part,
                                                                uint32_t rows, uint32_t T, uint32_t n_chunks, uint64_t units) {
    clx_norm::sum_ct<true>(x, valid, part, rows, T, n_chunks, units);
}

extern "C" __global__ __launch_bounds__(256) void clx_k_norm_sum_tc(const float* __restrict__ x, const uint32_t* __restrict__ valid, double* part,
                                                                    uint32_t rows, uint32_t T, uint32_t n_chunks, uint32_t n_groups) {
    clx_norm::sum_tc<false>(x, valid, part, rows, T, n_chunks, n_groups);
}

extern "C" __global__ __launch_bounds__(256) void clx_k_norm_sq_tc(const float* __restrict__ x, const uint32_t* __restrict__ valid, double* part,
                                                                   uint32_t rows, uint32_t T, uint32_t n_chunks, uint32_t n_groups) {
    clx_norm::sum_tc<true>(x, valid, part, rows, T, n_chunks, n_groups);
}

// The apply pass, in place.  Block b: tile b % n_tiles of window b / n_tiles; the window's `rows * T` cells lie [rows][T] (tc == 0)
// or [T][rows] (tc == 1).  stats (may be null) is [n_windows][rows][2].
extern "C" __global__ __launch_bounds__(256) void clx_k_norm_apply(float* x, const uint32_t* __restrict__ valid, const double* __restrict__ part,
                                                                   float* stats, clx_norm_opts o, uint32_t rows, uint32_t T, uint32_t n_chunks,
                                                                   uint32_t tc, uint32_t n_tiles) {
    using namespace clx_norm;
    __shared__ float s_m[kMaxRows];
    __shared__ float s_s[kMaxRows];
    const uint32_t tid = threadIdx.x, k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const uint64_t cells = (uint64_t)rows * T;
    float* const w = x + (uint64_t)k * cells;
    const uint32_t head = (uint32_t)(((uintptr_t)w >> 2) & 3u);
    const uint64_t vectors = (cells + head + 3u) >> 2;
    const uint64_t v_lo = (uint64_t)tl * kApplyVecs;
    if (v_lo >= vectors) return;                               // (the whole block: n_tiles is sized for the largest head)
    const uint64_t v_hi = v_lo + kApplyVecs < vectors ? v_lo + kApplyVecs : vectors;
    const uint64_t e_lo = v_lo ? v_lo * 4u - head : 0u, e_hi = v_hi * 4u - head < cells ? v_hi * 4u - head : cells;   // the tile's cells
    const uint32_t n = valid[k];
    const uint32_t r_lo = tc ? 0u : (uint32_t)(e_lo / T), r_n = tc ? rows : (uint32_t)((e_hi - 1u) / T) - r_lo + 1u;
    for (uint32_t i = tid; i < r_n; i += kThreads) {
        const uint32_t r = r_lo + i;
        const double* const P = part + ((uint64_t)k * rows + r) * 2u * n_chunks;
        const float m = mean_of(P, n), s = o.var ? scale_of(P + n_chunks, n, o.ddof, o.eps) : 1.f;
        s_m[i] = m;
        s_s[i] = s;
        if (stats && (tc ? tl == 0u : (uint64_t)r * T >= e_lo)) {   // (the tile with the row's first cell)
            stats[((uint64_t)k * rows + r) * 2u] = m;
            stats[((uint64_t)k * rows + r) * 2u + 1u] = s;
        }
    }
    __syncthreads();
    const uint32_t inner = tc ? rows : T;                      // the cells of the faster axis
    for (uint32_t i = 0; i < kApplyVecs / kThreads; ++i) {
        const uint64_t v = v_lo + i * kThreads + tid;
        if (v >= v_hi) break;
        const int64_t e0 = (int64_t)(v * 4u) - (int64_t)head;
        float* const p = w + e0;                               // 16-byte aligned
        const uint64_t e = e0 < 0 ? 0u : (uint64_t)e0;         // the vector's first cell of the window: cell b of line a
        uint32_t a, b;
        if (cells <= 0xffffffffull) { a = (uint32_t)e / inner; b = (uint32_t)e - a * inner; }
        else { a = (uint32_t)(e / inner); b = (uint32_t)(e - (uint64_t)a * inner); }
        const bool whole = e0 >= 0 && (uint64_t)e0 + 4u <= cells;
        f4 q = { 0.f, 0.f, 0.f, 0.f };
        if (whole) q = *reinterpret_cast<const f4*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (e0 + j < 0 || (uint64_t)(e0 + j) >= cells) continue;
            const uint32_t r = tc ? b : a, t = tc ? a : b;
            float y = o.pad;
            if (t < n) {
                y = whole ? q[j] : p[j];
                if (o.mean) y = sub_rn(y, s_m[r - r_lo]);
                if (o.var) y = div_rn(y, s_s[r - r_lo]);
            }
            if (whole) q[j] = y; else p[j] = y;
            if (++b == inner) { b = 0u; ++a; }
        }
        if (whole) *reinterpret_cast<f4*>(p) = q;
    }
}

// The host side of clx_norm_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the launch
// shape (p->n_chunks == 0: nothing to launch).
inline const char* clx_norm_check(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                  const clx_norm_opts* o, clx_norm_plan* p) {
    using namespace clx_norm;
    *p = clx_norm_plan();
    if (!o) return "clx_norm_windows: null options";
    if (o->mean > 1u) return "clx_norm_windows: mean must be 0 or 1";
    if (o->var > 1u) return "clx_norm_windows: var must be 0 or 1";
    if (o->ddof > 1u) return "clx_norm_windows: ddof must be 0 or 1";
    if (!o->mean && !o->var) return "clx_norm_windows: mean and var are both 0: nothing to do";
    if (!std::isfinite(o->eps) || !(o->eps >= 0.f)) return "clx_norm_windows: eps must be finite and not negative";
    if (!std::isfinite(o->pad)) return "clx_norm_windows: pad must be finite";
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return "clx_norm_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT";
    if (rows < 1u || rows > kMaxRows) return "clx_norm_windows: rows must be 1..256";
    if (n_windows == 0 || T == 0) return nullptr;
    if (!data || !valid) return "clx_norm_windows: null argument";
    for (size_t k = 0; k < n_windows; ++k)
        if (valid[k] > T) return "clx_norm_windows: valid[k] is larger than T";
    const uint64_t nc = ((uint64_t)T + kChunk - 1u) / kChunk;
    const uint32_t tc = layout == CLX_WINDOW_TC && rows > 1u ? 1u : 0u;
    const uint64_t groups = (rows + kTcRows - 1u) / kTcRows;
    const uint64_t units = (uint64_t)n_windows * rows * nc;
    const uint64_t sum_blocks = tc ? (uint64_t)n_windows * nc * groups : (units + 3u) / 4u;
    const uint64_t cells = (uint64_t)rows * T, tiles = (((cells + 6u) >> 2) + kApplyVecs - 1u) / kApplyVecs;   // (at most (cells + 6) / 4 vectors)
    if (n_windows > 0x7fffffffull || units > 0x7fffffffull || sum_blocks > 0x7fffffffull || tiles * (uint64_t)n_windows > 0x7fffffffull)
        return "clx_norm_windows: too many windows in one call";
    p->n_chunks = (uint32_t)nc; p->tc = tc; p->n_groups = (uint32_t)groups; p->sum_blocks = (uint32_t)sum_blocks; p->n_tiles = (uint32_t)tiles;
    p->partials = units * 2u;
    return nullptr;
}
