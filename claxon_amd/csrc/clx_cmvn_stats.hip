// clx_cmvn_stats.hip -- Kaldi's CMVN accumulator on the device (compute-cmvn-stats), clx_cmvn_stats_windows, and the normalisation of
// every window by the accumulator of its group (apply-cmvn --utt2spk), clx_cmvn_grouped_windows.  claxon_hip.h has the definitions;
// this is how they are computed.  This file stands behind clx_norm.hip and clx_cmvn.hip in a translation unit: the
// order of a chunk's sum is clx_norm's (its dadd_rn, dmul_rn, fold_strands, fold_chunks and live_chunks, chunk for chunk, strand for
// strand), the float32 pair of the apply and the double division and square root of the solve are clx_cmvn's.  Nothing is added
// atomically and no product fuses with a sum.
//
// The per-call table (clx_cmvn_stats_fill_table, uploaded once) is 32-bit words: V[n], G[n] (the window's group, NULL resolved to
// 0), then for the accumulating call the groups that have a window in this call, as the host's stable counting sort leaves them:
// gid[n] (in the order of their first window; n_present of them are used), start[n + 1] and list[n] (CSR: the windows of present
// group j are list[start[j] .. start[j + 1]), ascending).  Beside it the partials [n][rows][2][n_chunks] doubles, clx_norm's shape.
//
// The accumulation, two launches (behind a memset of the accumulator when the call resets it):
//   clx_k_cmvn_stats_sum     CT (and TC with rows == 1, the same memory): a wave is one chunk (kChunk = 4096 frames) of one row of one
//                            window; lane i adds (double)x[t] into S and (double)x[t] * (double)x[t] (exact) into Q for t = i, i + 64,
//                            .. ascending from +0.0, then the six-step xor fold of each; lane 0 stores S_c and Q_c.  One pass over
//                            the data, 256 contiguous bytes a load.  0 bytes of LDS.
//   clx_k_cmvn_stats_sum_tc  TC, rows > 1: clx_norm's tile of 64 time steps x 16 rows through LDS (rows 17 floats apart), four rows a
//                            wave, S and Q side by side: the strands are the same, so is every word.  4 352 bytes of LDS.
//                            Either skips a chunk without a live cell and a window of group -1: neither read nor written.
//   clx_k_cmvn_stats_fold    one lane a (present group, column, S | Q): acc = the accumulator's word; for the group's windows k
//                            ascending, W[k] = the window's chunk partials ascending from +0.0, acc += W[k]; the count column adds
//                            (double)V[k] instead; column `rows` of the Q row is no lane's.  Lanes run along the columns: the
//                            accumulator is read and written in whole lines.  A group without a window has no lane: it keeps its
//                            words, or the zeros of the reset's memset.  0 bytes of LDS.
// The normalisation, two launches:
//   clx_k_cmvn_stats_solve   one lane a (group, row): clx_cmvn_from_stats' arithmetic, word for word, into shift_scale
//                            [n_groups][2][rows] floats; a group whose count is not above 0 gets (+0.0, 1.0f).  0 bytes of LDS.
//   clx_k_cmvn_grouped       clx_k_cmvn_global's tiling (1024 16-byte vectors a block, whole live vectors one load and one store,
//                            ragged edges cell by cell), shift and scale read from shift_scale[G[k]]; a window of group -1 keeps
//                            its live cells and gets its padding.  0 bytes of LDS.
// No scratch, no spills, wave64, blocks of 256 (tests/test_code_object_cmvn_stats.py reads them from the code object).
// clx_cmvn_stats_check, clx_cmvn_grouped_check and clx_cmvn_stats_fill_table are the host side (plain C++, shared with the wave
// simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/claxon_hip.h"

// the launch shape clx_cmvn_stats_check / clx_cmvn_grouped_check give (launch == 0: nothing to launch)
struct clx_cmvn_stats_plan {
    uint32_t launch = 0;         // 1: the call has windows and frames
    uint32_t n_chunks = 0;       // accumulation: chunks of the time axis
    uint32_t tc = 0;             // accumulation: 1 for the TC sum (layout TC with rows > 1); normalisation: 1 for [n_windows][T][rows]
    uint32_t n_rgroups = 0;      // TC sum: row groups of a window
    uint32_t sum_blocks = 0;     // blocks of the sum pass
    uint32_t n_tiles = 0;        // normalisation: tiles of a window (n_windows * n_tiles blocks)
    uint32_t solve_blocks = 0;   // normalisation: blocks of the solve
    uint64_t partials = 0;       // accumulation: doubles of the partial sums, [n_windows][rows][2][n_chunks]
    uint64_t table_words = 0;    // 32-bit words of the per-call table
    uint64_t stats_bytes = 0;    // bytes of the accumulator, [n_groups][2][rows + 1] doubles
};

namespace clx_cmvn_stats {

constexpr uint32_t kThreads = 256u, kMaxRows = 8192u, kMaxGroups = 65536u, kMaxT = 0x7fffffffu, kVecs = clx_cmvn::kVecs;
constexpr uint32_t kChunk = clx_norm::kChunk, kStrands = clx_norm::kStrands, kTcRows = clx_norm::kTcRows, kTcRow = clx_norm::kTcRow;
constexpr uint32_t kSumLdsBytes = 0u, kFoldLdsBytes = 0u, kSolveLdsBytes = 0u, kApplyLdsBytes = 0u;
constexpr uint32_t kSumTcLdsBytes = kStrands * kTcRow * 4u;                // 4 352
static_assert(kSumTcLdsBytes == 4352u, "the header states this");
static_assert(kThreads == 4u * kStrands && kTcRows * kStrands == 4u * kThreads, "clx_norm's tile: four waves, four floats a lane");

// the words of the per-call table: V, G, gid, start (n + 1), list
__host__ __device__ __forceinline__ uint64_t table_words(uint64_t n, bool csr) { return csr ? 5u * n + 1u : 2u * n; }

}  // namespace clx_cmvn_stats

// Wave u of the grid: chunk u % n_chunks of row u / n_chunks (rows counted through the batch: window * rows + row).  tab: V[n], G[n].
// part is [n_windows * rows][2][n_chunks]: S partials, then Q partials.
extern "C" __global__ __launch_bounds__(256) void clx_k_cmvn_stats_sum(const float* __restrict__ x, const uint32_t* __restrict__ tab, double* part,
                                                                       uint32_t n_windows, uint32_t rows, uint32_t T, uint32_t n_chunks,
                                                                       uint64_t units) {
    using namespace clx_norm;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t u = (uint64_t)blockIdx.x * (clx_cmvn_stats::kThreads / kStrands) + (threadIdx.x >> 6);
    if (u >= units) return;                                    // (the whole wave)
    const uint64_t kr = u / n_chunks;
    const uint32_t c = (uint32_t)(u - kr * n_chunks), k = (uint32_t)(kr / rows), n = tab[k];
    const uint64_t t0 = (uint64_t)c * kChunk;
    if (t0 >= n || (int32_t)tab[n_windows + k] < 0) return;    // (the whole wave)
    const float* const row = x + kr * T;
    const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
    double S = 0.0, Q = 0.0;
#pragma unroll 4
    for (uint64_t t = t0 + lane; t < end; t += kStrands) {
        const double v = (double)row[t];
        S = dadd_rn(S, v);
        Q = dadd_rn(Q, dmul_rn(v, v));
    }
    S = fold_strands(S);
    Q = fold_strands(Q);
    if (lane == 0u) {
        double* const P = part + kr * 2u * n_chunks;
        P[c] = S;
        P[n_chunks + c] = Q;
    }
}

// Block b: row group b % n_rgroups of chunk (b / n_rgroups) % n_chunks of window b / (n_rgroups * n_chunks); x is [n_windows][T][rows].
extern "C" __global__ __launch_bounds__(256) void clx_k_cmvn_stats_sum_tc(const float* __restrict__ x, const uint32_t* __restrict__ tab, double* part,
                                                                          uint32_t n_windows, uint32_t rows, uint32_t T, uint32_t n_chunks,
                                                                          uint32_t n_rgroups) {
    using namespace clx_norm;
    __shared__ float s_tile[kStrands * kTcRow];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t g = blockIdx.x % n_rgroups, kc = blockIdx.x / n_rgroups, c = kc % n_chunks, k = kc / n_chunks;
    const uint32_t n = tab[k], r0 = g * kTcRows;
    const uint64_t t0 = (uint64_t)c * kChunk;
    if (t0 >= n || (int32_t)tab[n_windows + k] < 0) return;    // (the whole block)
    const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
    const float* const base = x + (uint64_t)k * rows * T;
    double* const P = part + ((uint64_t)k * rows + r0) * 2u * n_chunks;
    double S[4] = { 0.0, 0.0, 0.0, 0.0 }, Q[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (uint64_t ts = t0; ts < end; ts += kStrands) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t idx = tid + i * clx_cmvn_stats::kThreads, rr = idx & (kTcRows - 1u), tt = idx / kTcRows;
            if (ts + tt < end && r0 + rr < rows) s_tile[tt * kTcRow + rr] = base[(ts + tt) * rows + r0 + rr];
        }
        __syncthreads();
        if (ts + lane < end)
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q)
                if (r0 + 4u * w + q < rows) {
                    const double v = (double)s_tile[lane * kTcRow + 4u * w + q];
                    S[q] = dadd_rn(S[q], v);
                    Q[q] = dadd_rn(Q[q], dmul_rn(v, v));
                }
        __syncthreads();                                       // (the tile has been read)
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        const double a = fold_strands(S[q]), b = fold_strands(Q[q]);
        if (lane == 0u && r0 + 4u * w + q < rows) {
            P[(uint64_t)(4u * w + q) * 2u * n_chunks + c] = a;
            P[(uint64_t)(4u * w + q) * 2u * n_chunks + n_chunks + c] = b;
        }
    }
}

// Lane i of the grid: column i % (rows + 1) of row (i / (rows + 1)) % 2 (0: the sums and the count, 1: the sums of squares) of present
// group i / (2 (rows + 1)).  tab: V[n], G[n], gid[n], start[n + 1], list[n].  stats is [n_groups][2][rows + 1].
extern "C" __global__ __launch_bounds__(256) void clx_k_cmvn_stats_fold(const double* __restrict__ part, const uint32_t* __restrict__ tab, double* stats,
                                                                        uint32_t n_windows, uint32_t rows, uint32_t n_chunks, uint64_t lanes) {
    using namespace clx_norm;
    const uint64_t i = (uint64_t)blockIdx.x * clx_cmvn_stats::kThreads + threadIdx.x;
    if (i >= lanes) return;
    const uint32_t cols = rows + 1u;
    const uint32_t j = (uint32_t)(i / (2u * cols)), rem = (uint32_t)(i - (uint64_t)j * 2u * cols), h = rem / cols, col = rem - h * cols;
    if (h == 1u && col == rows) return;                        // (the unused word of the Q row)
    const uint32_t* const gid = tab + 2u * (uint64_t)n_windows;
    const uint32_t* const start = gid + n_windows;
    const uint32_t* const list = start + n_windows + 1u;
    double* const word = stats + ((uint64_t)gid[j] * 2u + h) * cols + col;
    double acc = *word;
    for (uint32_t e = start[j]; e < start[j + 1u]; ++e) {
        const uint32_t k = list[e], n = tab[k];
        const double W = col == rows ? (double)n : fold_chunks(part + (((uint64_t)k * rows + col) * 2u + h) * n_chunks, live_chunks(n));
        acc = dadd_rn(acc, W);
    }
    *word = acc;
}

// Lane i of the grid: row i % rows of group i / rows.  stats is [n_groups][2][rows + 1] doubles, ss [n_groups][2][rows] floats: the
// group's shifts, then its scales.
extern "C" __global__ __launch_bounds__(256) void clx_k_cmvn_stats_solve(const double* __restrict__ stats, float* ss, uint32_t n_groups, uint32_t rows,
                                                                         uint32_t norm_vars) {
    using namespace clx_cmvn;
    const uint64_t i = (uint64_t)blockIdx.x * clx_cmvn_stats::kThreads + threadIdx.x;
    if (i >= (uint64_t)n_groups * rows) return;
    const uint32_t g = (uint32_t)(i / rows), r = (uint32_t)(i - (uint64_t)g * rows);
    const double* const st = stats + (uint64_t)g * 2u * (rows + 1u);
    const double count = st[rows];
    float sh = 0.f, sc = 1.f;
    if (count > 0.0) {
        const double mean = ddiv_rn(st[r], count);
        double var = dsub_rn(ddiv_rn(st[(uint64_t)rows + 1u + r], count), dmul_rn(mean, mean));
        if (!(var >= 1e-20)) var = 1e-20;
        sh = to_f32(-mean);
        if (norm_vars) sc = to_f32(ddiv_rn(1.0, dsqrt_rn(var)));
    }
    ss[(uint64_t)g * 2u * rows + r] = sh;
    ss[(uint64_t)g * 2u * rows + rows + r] = sc;
}

// Block b: tile b % n_tiles of window b / n_tiles, in place; the window's rows * T cells lie [rows][T] (tc == 0) or [T][rows]
// (tc == 1).  tab: V[n_windows], G[n_windows].  pad is the word of every cell with t >= V.
extern "C" __global__ __launch_bounds__(256) void clx_k_cmvn_grouped(float* x, const uint32_t* __restrict__ tab, const float* __restrict__ ss,
                                                                     uint32_t n_windows, uint32_t rows, uint32_t T, float pad, uint32_t tc,
                                                                     uint32_t n_tiles) {
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
    const int32_t grp = (int32_t)tab[n_windows + k];
    const float* const shift = ss + (uint64_t)(grp < 0 ? 0 : grp) * 2u * rows;     // (group -1: never read)
    const float* const scale = shift + rows;
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
        if (grp >= 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live >> j & 1u) q[j] = mul_rn(add_rn(q[j], shift[r[j]]), scale[r[j]]);
        }
        if (whole) *reinterpret_cast<f4*>(p) = q;
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j >= 0 && (uint64_t)(e0 + j) < cells) p[j] = q[j];
        }
    }
}

// What both calls refuse alike; `who` is 0 for the accumulating call and 1 for the normalising one.
#define CLX_CMVN_STATS_WHO(text) (who ? "clx_cmvn_grouped_windows: " text : "clx_cmvn_stats_windows: " text)
inline const char* clx_cmvn_stats_check_shape(int who, uint32_t layout, uint32_t rows, uint32_t T, uint32_t n_groups, const void* d_stats) {
    using namespace clx_cmvn_stats;
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return CLX_CMVN_STATS_WHO("layout must be CLX_WINDOW_TC or CLX_WINDOW_CT");
    if (rows < 1u || rows > kMaxRows) return CLX_CMVN_STATS_WHO("rows must be 1..8192");
    if (T > kMaxT) return CLX_CMVN_STATS_WHO("T must be below 2^31");
    if (n_groups < 1u || n_groups > kMaxGroups) return CLX_CMVN_STATS_WHO("n_groups must be 1..65536");
    if (!d_stats) return CLX_CMVN_STATS_WHO("null d_stats");
    if ((uintptr_t)d_stats & 7u) return CLX_CMVN_STATS_WHO("d_stats must be 8-byte aligned");
    return nullptr;
}

inline const char* clx_cmvn_stats_check_windows(int who, const void* data, size_t n_windows, uint32_t T, const uint32_t* valid, const int32_t* group,
                                                uint32_t n_groups) {
    if (!data) return CLX_CMVN_STATS_WHO("null d_data");
    if (!valid) return CLX_CMVN_STATS_WHO("null valid");
    if (n_windows > 0x7fffffffull) return CLX_CMVN_STATS_WHO("too many blocks in one call");
    for (size_t k = 0; k < n_windows; ++k) {
        if (valid[k] > T) return CLX_CMVN_STATS_WHO("valid[k] is larger than T");
        if (group && (group[k] < -1 || group[k] >= (int64_t)n_groups)) return CLX_CMVN_STATS_WHO("group[k] must be -1..n_groups - 1");
    }
    return nullptr;
}

// The host side of clx_cmvn_stats_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the
// launch shape (p->launch == 0: nothing to launch; a reset still zeroes p->stats_bytes of the accumulator).
inline const char* clx_cmvn_stats_check(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                        const int32_t* group, uint32_t n_groups, const void* d_stats, const clx_cmvn_stats_opts* o,
                                        clx_cmvn_stats_plan* p) {
    using namespace clx_cmvn_stats;
    const int who = 0;
    *p = clx_cmvn_stats_plan();
    if (!o) return "clx_cmvn_stats_windows: null options";
    if (o->reserved != 0u) return "clx_cmvn_stats_windows: reserved must be 0";
    if (o->accumulate > 1u) return "clx_cmvn_stats_windows: accumulate must be 0 or 1";
    if (const char* why = clx_cmvn_stats_check_shape(who, layout, rows, T, n_groups, d_stats)) return why;
    p->stats_bytes = (uint64_t)n_groups * 2u * (rows + 1u) * sizeof(double);
    if (n_windows == 0 || T == 0) return nullptr;
    if (const char* why = clx_cmvn_stats_check_windows(who, data, n_windows, T, valid, group, n_groups)) return why;
    const uint64_t nc = ((uint64_t)T + kChunk - 1u) / kChunk;
    const uint32_t tc = layout == CLX_WINDOW_TC && rows > 1u ? 1u : 0u;
    const uint64_t rgroups = (rows + kTcRows - 1u) / kTcRows;
    const uint64_t units = (uint64_t)n_windows * rows * nc;
    const uint64_t sum_blocks = tc ? (uint64_t)n_windows * nc * rgroups : (units + 3u) / 4u;
    const uint64_t fold_blocks = ((uint64_t)n_windows * 2u * (rows + 1u) + kThreads - 1u) / kThreads;    // (every window a group of its own)
    if (units > 0x7fffffffull || sum_blocks > 0x7fffffffull || fold_blocks > 0x7fffffffull) return "clx_cmvn_stats_windows: too many blocks in one call";
    p->launch = 1u; p->n_chunks = (uint32_t)nc; p->tc = tc; p->n_rgroups = (uint32_t)rgroups; p->sum_blocks = (uint32_t)sum_blocks;
    p->partials = units * 2u;
    p->table_words = table_words(n_windows, true);
    return nullptr;
}

// The host side of clx_cmvn_grouped_windows, likewise.
inline const char* clx_cmvn_grouped_check(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                          const int32_t* group, uint32_t n_groups, const void* d_stats, const void* d_shift_scale,
                                          const clx_cmvn_grouped_opts* o, clx_cmvn_stats_plan* p) {
    using namespace clx_cmvn_stats;
    const int who = 1;
    *p = clx_cmvn_stats_plan();
    if (!o) return "clx_cmvn_grouped_windows: null options";
    if (o->reserved != 0u) return "clx_cmvn_grouped_windows: reserved must be 0";
    if (o->norm_vars > 1u) return "clx_cmvn_grouped_windows: norm_vars must be 0 or 1";
    if (!std::isfinite(o->pad)) return "clx_cmvn_grouped_windows: pad must be finite";
    if (const char* why = clx_cmvn_stats_check_shape(who, layout, rows, T, n_groups, d_stats)) return why;
    if (!d_shift_scale) return "clx_cmvn_grouped_windows: null d_shift_scale";
    if ((uintptr_t)d_shift_scale & 3u) return "clx_cmvn_grouped_windows: d_shift_scale must be 4-byte aligned";
    if (n_windows == 0 || T == 0) return nullptr;
    if (const char* why = clx_cmvn_stats_check_windows(who, data, n_windows, T, valid, group, n_groups)) return why;
    const uint64_t cells = (uint64_t)rows * T, tiles = (((cells + 6u) >> 2) + kVecs - 1u) / kVecs;       // (at most (cells + 6) / 4 vectors)
    if (tiles * (uint64_t)n_windows > 0x7fffffffull) return "clx_cmvn_grouped_windows: too many blocks in one call";
    p->launch = 1u; p->n_tiles = (uint32_t)tiles; p->tc = layout == CLX_WINDOW_TC ? 1u : 0u;
    p->solve_blocks = (uint32_t)(((uint64_t)n_groups * rows + kThreads - 1u) / kThreads);
    p->table_words = table_words(n_windows, false);
    return nullptr;
}
#undef CLX_CMVN_STATS_WHO

// The per-call table of checked arguments into `tab`: V, G, and with csr the present groups and their windows (a stable counting
// sort: the groups in the order of their first window, each group's windows ascending).  `slot` is the caller's work array: it
// comes and goes as zeros, n_groups words at the least once it has grown.  Returns n_present (0 without csr).
inline uint32_t clx_cmvn_stats_fill_table(uint32_t* tab, size_t n_windows, const uint32_t* valid, const int32_t* group, uint32_t n_groups, bool csr,
                                          std::vector<uint32_t>& slot) {
    const size_t n = n_windows;
    for (size_t k = 0; k < n; ++k) { tab[k] = valid[k]; tab[n + k] = (uint32_t)(group ? group[k] : 0); }
    if (!csr) return 0u;
    uint32_t* const gid = tab + 2u * n;
    uint32_t* const start = gid + n;
    uint32_t* const list = start + n + 1u;
    if (slot.size() < n_groups) slot.resize(n_groups, 0u);
    for (size_t k = 0; k < n; ++k) { gid[k] = 0u; start[k] = 0u; list[k] = 0u; }
    start[n] = 0u;
    uint32_t present = 0u;
    for (size_t k = 0; k < n; ++k) {                           // the groups as they first appear; start[j + 1] counts group j's windows
        const int32_t g = (int32_t)tab[n + k];
        if (g < 0) continue;
        if (!slot[g]) { gid[present] = (uint32_t)g; slot[g] = ++present; }
        ++start[slot[g]];
    }
    for (uint32_t j = 0; j < present; ++j) start[j + 1u] += start[j];
    for (size_t k = 0; k < n; ++k) {                           // ascending k into each group's run: start[j] walks to start[j + 1] ..
        const int32_t g = (int32_t)tab[n + k];
        if (g < 0) continue;
        list[start[slot[g] - 1u]++] = (uint32_t)k;
    }
    for (uint32_t j = present; j > 0u; --j) start[j] = start[j - 1u];      // .. and is moved back
    start[0] = 0u;
    for (uint32_t j = 0; j < present; ++j) slot[gid[j]] = 0u;
    return present;
}
