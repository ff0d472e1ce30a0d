// clx_add.hip -- a second batch of windows added to a dense float32 batch at a target signal-to-noise ratio, in place:
// clx_add_windows.  claxon_hip.h has the definition; this is how it is computed.  It stands behind clx_norm.hip in
// clx_api.hip and takes the order of its sums from there: clx_norm's chunks, strands, xor fold and ascending chunk fold.
//
// Four launches on one stream, each reading what the one before left in tables the context keeps:
//   sum     clx_k_add_sum / clx_k_add_sum_tc    per (window, signal or noise, row, chunk) the sum of the squared live cells, a double
//   gain    clx_k_add_gain                      one lane per window: the row sums in order, Es and En, the double arithmetic, g
//   apply   clx_k_add_apply                     x = fmaf(g, n, x) over the cells with t < Vn -- a streaming pass like clx_k_norm_apply
// The per-call table (clx_add_fill, uploaded once): q[n_windows] doubles, then Vs, Vn and j as 32-bit words, then (device only) g.
// Vn is 0 for a window that gets nothing (j < 0, Vs == 0, no live noise sample, q == 0): no pass reads a cell of it.
//
// CT ([n_windows][rows][T]; also TC with rows == 1, the same memory): a wave is one chunk of one row of the signal or the noise,
// lane i loads t = i, i + 64, ..: clx_norm's sum_ct with the square in place of the cell.  Four waves a block, no LDS, no barrier.
// TC ([n_windows][T][rows], rows 2..8): a wave is one chunk of one window's signal or noise with all its rows: lane i holds the
// strand i of every row (up to eight double accumulators) and loads the `rows` contiguous floats of time step t = i, i + 64, ..;
// the wave's loads of one round cover 64 * rows contiguous floats between them.  No LDS either: with at most eight rows there is
// nothing to transpose.
// Apply: clx_k_norm_apply's tiling -- a block is kApplyVecs 16-byte vectors of the window's 16-byte grid; a vector whose four
// cells are all live is one load of x, one of n (four scalar loads where the noise window sits at another offset within 16 bytes)
// and one store; every other live cell goes float by float; a cell with t >= Vn is neither loaded nor stored.  No LDS.
//
// clx_add_check and clx_add_fill are the host side (plain C++, shared with the wave simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include "../../include/claxon_hip.h"

// the launch shape clx_add_check gives (n_chunks == 0: nothing to launch)
struct clx_add_plan {
    uint32_t n_chunks = 0;       // chunks of the time axis
    uint32_t tc = 0;             // 1: the TC sum kernel (layout TC with rows > 1)
    uint64_t units = 0;          // waves of the sum pass
    uint32_t sum_blocks = 0;     // ... and its blocks
    uint32_t gain_blocks = 0;    // blocks of the gain step
    uint32_t n_tiles = 0;        // tiles of a window in the apply pass (n_windows * n_tiles blocks)
    uint64_t partials = 0;       // doubles of the per-call table: [n_windows][2][rows][n_chunks]
};

namespace clx_add {

using clx_norm::kThreads;
using clx_norm::kStrands;
using clx_norm::kChunk;
using clx_norm::kApplyVecs;
using clx_norm::f4;
constexpr uint32_t kMaxRows = 8u;
constexpr uint32_t kTableBytes = 20u, kTableBytesDevice = 24u;   // a window's share of the per-call table: host staging / device
constexpr double kMaxSnr = 200.0;

#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ float fma_rn(float a, float b, float c) { return __fmaf_rn(a, b, c); }
__device__ __forceinline__ double dsqrt_rn(double a) { return __dsqrt_rn(a); }
#else
inline float fma_rn(float a, float b, float c) { return fmaf(a, b, c); }
inline double dsqrt_rn(double a) { return sqrt(a); }
#endif

// the per-call table of n windows
struct table { const double* q; const uint32_t* vs; const uint32_t* vn; const int32_t* j; };
__host__ __device__ __forceinline__ table table_of(const void* tab, size_t n) {
    table t;
    t.q = (const double*)tab;
    t.vs = (const uint32_t*)(t.q + n);
    t.vn = t.vs + n;
    t.j = (const int32_t*)(t.vn + n);
    return t;
}

// one cell's term: its square, exact in double
__device__ __forceinline__ double sq(float x) {
    const double d = (double)x;
    return clx_norm::dmul_rn(d, d);
}

}  // namespace clx_add

// Wave u of the grid: chunk u % n_chunks of row (u / n_chunks) % rows of the signal (even) or the noise (odd) of window
// u / (2 * rows * n_chunks).  part is [n_windows][2][rows][n_chunks].  A chunk without a live cell is neither read nor written.
extern "C" __global__ __launch_bounds__(256) void clx_k_add_sum(const float* __restrict__ x, const float* __restrict__ noise, const void* __restrict__ tab,
                                                                double* part, uint32_t n_windows, uint32_t rows, uint32_t T, uint32_t n_chunks,
                                                                uint64_t units) {
    using namespace clx_add;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t u = (uint64_t)blockIdx.x * (kThreads / kStrands) + (threadIdx.x >> 6);
    if (u >= units) return;                                    // (the whole wave)
    const uint64_t kr = u / n_chunks, kw = kr / rows;
    const uint32_t c = (uint32_t)(u - kr * n_chunks), r = (uint32_t)(kr - kw * rows), k = (uint32_t)(kw >> 1), is_noise = (uint32_t)kw & 1u;
    const table t = table_of(tab, n_windows);
    const uint32_t vn = t.vn[k];
    if (vn == 0u) return;                                      // (the whole wave: the window gets nothing)
    const uint32_t n = is_noise ? vn : t.vs[k];
    const uint64_t t0 = (uint64_t)c * kChunk;
    if (t0 >= n) return;                                       // (the whole wave)
    const float* const row = is_noise ? noise + ((uint64_t)(uint32_t)t.j[k] * rows + r) * T : x + ((uint64_t)k * rows + r) * T;
    const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
    double acc = 0.0;
    for (uint64_t i = t0 + lane; i < end; i += kStrands) acc = clx_norm::dadd_rn(acc, sq(row[i]));
    acc = clx_norm::fold_strands(acc);
    if (lane == 0u) part[kr * n_chunks + c] = acc;
}

// Wave u: chunk u % n_chunks of the signal (even) or the noise (odd) of window u / (2 * n_chunks), every row; the windows are
// [T][rows].
extern "C" __global__ __launch_bounds__(256) void clx_k_add_sum_tc(const float* __restrict__ x, const float* __restrict__ noise,
                                                                   const void* __restrict__ tab, double* part, uint32_t n_windows, uint32_t rows,
                                                                   uint32_t T, uint32_t n_chunks, uint64_t units) {
    using namespace clx_add;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t u = (uint64_t)blockIdx.x * (kThreads / kStrands) + (threadIdx.x >> 6);
    if (u >= units) return;                                    // (the whole wave)
    const uint64_t kw = u / n_chunks;
    const uint32_t c = (uint32_t)(u - kw * n_chunks), k = (uint32_t)(kw >> 1), is_noise = (uint32_t)kw & 1u;
    const table t = table_of(tab, n_windows);
    const uint32_t vn = t.vn[k];
    if (vn == 0u) return;                                      // (the whole wave)
    const uint32_t n = is_noise ? vn : t.vs[k];
    const uint64_t t0 = (uint64_t)c * kChunk;
    if (t0 >= n) return;                                       // (the whole wave)
    const float* const base = is_noise ? noise + (uint64_t)(uint32_t)t.j[k] * rows * T : x + (uint64_t)k * rows * T;
    const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
    double acc[kMaxRows] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (uint64_t i = t0 + lane; i < end; i += kStrands) {
        const float* const p = base + i * rows;
#pragma unroll
        for (uint32_t r = 0; r < kMaxRows; ++r)
            if (r < rows) acc[r] = clx_norm::dadd_rn(acc[r], sq(p[r]));
    }
#pragma unroll
    for (uint32_t r = 0; r < kMaxRows; ++r) {
        if (r >= rows) break;                                  // (the whole wave)
        const double a = clx_norm::fold_strands(acc[r]);
        if (lane == 0u) part[(kw * rows + r) * n_chunks + c] = a;
    }
}

// Lane k of the grid: window k's gain, into gain (the context's) and gains (the caller's, may be null).
extern "C" __global__ __launch_bounds__(256) void clx_k_add_gain(const void* __restrict__ tab, const double* __restrict__ part, float* gain,
                                                                 float* gains, uint32_t n_windows, uint32_t rows, uint32_t n_chunks) {
    using namespace clx_add;
    using namespace clx_norm;
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n_windows) return;
    const table t = table_of(tab, n_windows);
    const uint32_t vn = t.vn[k], vs = t.vs[k];
    float g = 0.f;
    if (vn != 0u) {
        const double* const P = part + k * 2u * rows * n_chunks;
        const uint32_t ls = live_chunks(vs), ln = live_chunks(vn);
        double es = 0.0, en = 0.0;
        for (uint32_t r = 0; r < rows; ++r) {
            es = dadd_rn(es, fold_chunks(P + (uint64_t)r * n_chunks, ls));
            en = dadd_rn(en, fold_chunks(P + (uint64_t)(rows + r) * n_chunks, ln));
        }
        if (es != 0.0 && en != 0.0)
            g = to_f32(dsqrt_rn(ddiv_rn(dmul_rn(dmul_rn(es, (double)vn), t.q[k]), dmul_rn(en, (double)vs))));
    }
    gain[k] = g;
    if (gains) gains[k] = g;
}

// The apply pass, in place.  Block b: tile b % n_tiles of window b / n_tiles; the window's `rows * T` cells lie [rows][T] (tc == 0)
// or [T][rows] (tc == 1), the noise window's too.
extern "C" __global__ __launch_bounds__(256) void clx_k_add_apply(float* x, const float* __restrict__ noise, const void* __restrict__ tab,
                                                                  const float* __restrict__ gain, uint32_t n_windows, uint32_t rows, uint32_t T,
                                                                  uint32_t tc, uint32_t n_tiles) {
    using namespace clx_add;
    const uint32_t tid = threadIdx.x, k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const float g = gain[k];
    if (g == 0.f) return;                                      // (the whole block: the window is not rewritten)
    const table t = table_of(tab, n_windows);
    const uint32_t vn = t.vn[k];
    const uint64_t cells = (uint64_t)rows * T;
    float* const w = x + (uint64_t)k * cells;
    const float* const nw = noise + (uint64_t)(uint32_t)t.j[k] * cells;
    const uint32_t head = (uint32_t)(((uintptr_t)w >> 2) & 3u);
    const bool n_aligned = ((((uintptr_t)nw) ^ ((uintptr_t)w)) & 15u) == 0u;     // the noise window lies on the same 16-byte grid
    const uint64_t vectors = (cells + head + 3u) >> 2;
    const uint64_t v_lo = (uint64_t)tl * kApplyVecs;
    if (v_lo >= vectors) return;                               // (the whole block: n_tiles is sized for the largest head)
    const uint64_t v_hi = v_lo + kApplyVecs < vectors ? v_lo + kApplyVecs : vectors;
    if (tc && v_lo * 4u >= (uint64_t)vn * rows + head) return; // (the whole block: TC's live cells are the window's first vn * rows)
    const uint32_t inner = tc ? rows : T;                      // the cells of the faster axis
    for (uint32_t i = 0; i < kApplyVecs / kThreads; ++i) {
        const uint64_t v = v_lo + i * kThreads + tid;
        if (v >= v_hi) break;
        const int64_t e0 = (int64_t)(v * 4u) - (int64_t)head;
        float* const p = w + e0;                               // 16-byte aligned
        const float* const pn = nw + e0;
        const uint64_t e = e0 < 0 ? 0u : (uint64_t)e0;         // the vector's first cell of the window: cell b of line a
        uint32_t a, b;
        if (cells <= 0xffffffffull) { a = (uint32_t)e / inner; b = (uint32_t)e - a * inner; }
        else { a = (uint32_t)(e / inner); b = (uint32_t)(e - (uint64_t)a * inner); }
        uint32_t live = 0u;                                    // bit j: cell j of the vector is a cell of the window with t < vn
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (e0 + j < 0 || (uint64_t)(e0 + j) >= cells) continue;
            if ((tc ? a : b) < vn) live |= 1u << j;
            if (++b == inner) { b = 0u; ++a; }
        }
        if (live == 15u) {
            f4 q = *reinterpret_cast<const f4*>(p);
            f4 m;
            if (n_aligned) m = *reinterpret_cast<const f4*>(pn);
            else { m[0] = pn[0]; m[1] = pn[1]; m[2] = pn[2]; m[3] = pn[3]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = fma_rn(g, m[j], q[j]);
            *reinterpret_cast<f4*>(p) = q;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live >> j & 1u) p[j] = fma_rn(g, pn[j], p[j]);
        }
    }
}

// The host side of clx_add_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the launch
// shape (p->n_chunks == 0: nothing to launch).
inline const char* clx_add_check(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const void* noise,
                                 size_t n_noise, const uint32_t* noise_valid, const int32_t* noise_index, const float* snr_db, uint32_t layout,
                                 const clx_add_opts* o, clx_add_plan* p) {
    using namespace clx_add;
    *p = clx_add_plan();
    if (o && o->reserved != 0u) return "clx_add_windows: opts must be NULL or all zero";
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return "clx_add_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT";
    if (rows < 1u || rows > kMaxRows) return "clx_add_windows: rows must be 1..8";
    if (n_windows == 0 || T == 0) return nullptr;
    if (!valid || !noise_index || !snr_db) return "clx_add_windows: null argument";
    bool work = false;
    for (size_t k = 0; k < n_windows; ++k) {
        if (valid[k] > T) return "clx_add_windows: valid[k] is larger than T";
        if (noise_index[k] < -1 || (noise_index[k] >= 0 && (uint64_t)noise_index[k] >= n_noise))
            return "clx_add_windows: noise_index[k] must be -1 .. n_noise - 1";
        const float s = snr_db[k];
        if (std::isnan(s)) return "clx_add_windows: snr_db[k] is NaN";
        if (std::isinf(s) ? s < 0.f : std::fabs((double)s) > kMaxSnr) return "clx_add_windows: snr_db[k] must be within -200 .. 200, or +inf";
        work = work || noise_index[k] >= 0;
    }
    if (!work) return nullptr;
    if (!data || !noise || !noise_valid) return "clx_add_windows: null argument";
    for (size_t j = 0; j < n_noise; ++j)
        if (noise_valid[j] > T) return "clx_add_windows: noise_valid[j] is larger than T";
    const uint64_t nc = ((uint64_t)T + kChunk - 1u) / kChunk;
    const uint32_t tc = layout == CLX_WINDOW_TC && rows > 1u ? 1u : 0u;
    const uint64_t partials = (uint64_t)n_windows * 2u * rows * nc;
    const uint64_t units = tc ? (uint64_t)n_windows * 2u * nc : partials;
    const uint64_t sum_blocks = (units + 3u) / 4u;
    const uint64_t cells = (uint64_t)rows * T, tiles = (((cells + 6u) >> 2) + kApplyVecs - 1u) / kApplyVecs;   // (at most (cells + 6) / 4 vectors)
    if (n_windows > 0x7fffffffull || n_noise > 0x7fffffffull || partials > 0x7fffffffull || tiles * (uint64_t)n_windows > 0x7fffffffull)
        return "clx_add_windows: too many windows in one call";
    p->n_chunks = (uint32_t)nc; p->tc = tc; p->units = units; p->sum_blocks = (uint32_t)sum_blocks;
    p->gain_blocks = (uint32_t)((n_windows + kThreads - 1u) / kThreads); p->n_tiles = (uint32_t)tiles; p->partials = partials;
    return nullptr;
}

// The per-call table of checked arguments, kTableBytes a window, into `tab` (8-byte aligned): q, Vs, Vn, j.
inline void clx_add_fill(void* tab, size_t n_windows, const uint32_t* valid, const uint32_t* noise_valid, const int32_t* noise_index,
                         const float* snr_db) {
    double* const q = (double*)tab;
    uint32_t* const vs = (uint32_t*)(q + n_windows);
    uint32_t* const vn = vs + n_windows;
    int32_t* const jj = (int32_t*)(vn + n_windows);
    for (size_t k = 0; k < n_windows; ++k) {
        const int32_t j = noise_index[k];
        q[k] = std::isinf(snr_db[k]) ? 0.0 : pow(10.0, -(double)snr_db[k] / 10.0);
        vs[k] = valid[k];
        jj[k] = j < 0 ? 0 : j;
        vn[k] = j < 0 || q[k] == 0.0 ? 0u : (noise_valid[j] < valid[k] ? noise_valid[j] : valid[k]);
    }
}
