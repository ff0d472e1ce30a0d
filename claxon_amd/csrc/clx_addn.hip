// clx_addn.hip -- several placed or looped noises added to a dense float32 batch in one pass, each at its own signal-to-noise
// ratio against the signal as it arrives: clx_addn_windows.  claxon_hip.h has the definition; this is how it is computed
// (DESIGN.md 4.25).  It stands behind clx_norm.hip and clx_add.hip in clx_api.hip and takes the order of its sums from the former
// (chunks, strands, xor fold, ascending chunk fold) and the gain's arithmetic from the latter.
//
// Three launches on one stream, each reading what the one before left in tables the context keeps:
//   sum     clx_k_addn_sum / clx_k_addn_sum_tc   per (signal window or term, row, chunk) the sum of the squared cells, a double
//   gain    clx_k_addn_gain                      one lane per term: the row sums in order, Es and En_m, the double arithmetic, g_m
//   apply   clx_k_addn_apply                     x = fmaf(g_m, n_m, x) through the window's terms, one load and one store a cell
// The per-call table (clx_addn_fill, uploaded once): a record per term (clx_addn::rec: q, the noise window's address, the offset,
// the period P, the cover's length Nc and the window), then per window Vs (0 where no term has a cover: no pass reads a cell of
// it), the CSR first[], and the hull [lo, hi) of the window's covers; behind that (device only) the M gains.
//
// Sum.  CT (also TC with rows == 1): a wave is one chunk of one row of a signal window or of a term's noise as the term reads it:
// lane l adds i = l, l + 64, .. of the chunk, and for a term that wraps (Nc > P) the lane's noise index is i mod P -- one 32-bit
// division a lane a chunk, then a step of 64 mod P with a conditional subtraction.  TC (rows 2..8): a wave is one chunk with all
// its rows, as clx_k_add_sum_tc.  Four waves a block, no LDS, no barrier.
// Apply: clx_k_add_apply's tiling -- a block is kApplyVecs 16-byte vectors of the window's 16-byte grid.  A lane loads the cells of
// its vector that lie inside the hull once, carries them through the window's terms in ascending order and stores them once.  The
// term records are read through the scalar path (their addresses depend on the block alone): no LDS, no barrier.  A vector whose
// four cells lie inside a term's cover on one side of its wrap point takes the term as one noise vector (four loads where the
// noise is off the 16-byte grid) and four fmaf; every other one goes cell by cell, the noise index stepped from the one division
// the vector has.
//
// clx_addn_check and clx_addn_fill are the host side (plain C++, shared with the wave simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include "../../include/claxon_hip.h"

// the launch shape clx_addn_check gives (n_chunks == 0: nothing to launch)
struct clx_addn_plan {
    uint32_t n_chunks = 0;       // chunks of the time axis
    uint32_t tc = 0;             // 1: the TC sum kernel (layout TC with rows > 1)
    uint32_t n_terms = 0;        // M
    uint64_t units = 0;          // waves of the sum pass
    uint32_t sum_blocks = 0;     // ... and its blocks
    uint32_t gain_blocks = 0;    // blocks of the gain step
    uint32_t n_tiles = 0;        // tiles of a window in the apply pass (n_windows * n_tiles blocks)
    uint64_t partials = 0;       // doubles of the per-call table: [n_windows + M][rows][n_chunks]
    uint64_t table_bytes = 0;    // the staged table; the device's has the M gains behind it
};

namespace clx_addn {

using clx_norm::kThreads;
using clx_norm::kStrands;
using clx_norm::kChunk;
using clx_norm::kApplyVecs;
using clx_norm::f4;
using clx_add::kMaxRows;
using clx_add::kMaxSnr;
using clx_add::fma_rn;
using clx_add::dsqrt_rn;
using clx_add::sq;
constexpr uint32_t kMaxTerms = 16u, kMaxBatches = 8u;

// a term as the kernels read it.  nc == 0: the term adds nothing (and nw may be null)
struct rec {
    double q;                    // clx_add_fill's q
    const float* nw;             // the noise window
    uint32_t off, P, nc, k;      // the offset, the period, the cover's length, the signal window
};
static_assert(sizeof(rec) == 32, "the table's records are 32 bytes");

// the per-call table of n windows and m terms
struct table { const rec* term; const uint32_t* vs; const uint32_t* first; const uint32_t* lo; const uint32_t* hi; };
__host__ __device__ __forceinline__ table table_of(const void* tab, size_t n, size_t m) {
    table t;
    t.term = (const rec*)tab;
    t.vs = (const uint32_t*)(t.term + m);
    t.first = t.vs + n;
    t.lo = t.first + n + 1u;
    t.hi = t.lo + n;
    return t;
}
__host__ __device__ __forceinline__ size_t table_bytes(size_t n, size_t m) { return m * sizeof(rec) + (4u * n + 1u) * sizeof(uint32_t); }

// the step of a lane's noise index from one round of the strands to the next: 64 mod P
__device__ __forceinline__ uint32_t strand_step(uint32_t P) { return P > kStrands ? kStrands : kStrands % P; }
// (idx + step) mod P for idx, step < P
__device__ __forceinline__ uint32_t wrap_add(uint32_t idx, uint32_t step, uint32_t P) { return idx >= P - step ? idx - (P - step) : idx + step; }

}  // namespace clx_addn

// Wave u of the grid: chunk u % n_chunks of row (u / n_chunks) % rows of unit w = u / (rows * n_chunks): signal window w, or term
// w - n_windows.  part is [n_windows + n_terms][rows][n_chunks].  A chunk without a live cell is neither read nor written.
extern "C" __global__ __launch_bounds__(256) void clx_k_addn_sum(const float* __restrict__ x, const void* __restrict__ tab, double* part,
                                                                 uint32_t n_windows, uint32_t n_terms, uint32_t rows, uint32_t T, uint32_t n_chunks,
                                                                 uint64_t units) {
    using namespace clx_addn;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t u = (uint64_t)blockIdx.x * (kThreads / kStrands) + (threadIdx.x >> 6);
    if (u >= units) return;                                    // (the whole wave)
    const uint64_t kr = u / n_chunks, w = kr / rows;
    const uint32_t c = (uint32_t)(u - kr * n_chunks), r = (uint32_t)(kr - w * rows);
    const table t = table_of(tab, n_windows, n_terms);
    const uint64_t t0 = (uint64_t)c * kChunk;
    double acc = 0.0;
    if (w < n_windows) {
        const uint32_t n = t.vs[w];
        if (t0 >= n) return;                                   // (the whole wave; n == 0: the window gets nothing)
        const float* const row = x + (w * rows + r) * T;
        const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
        for (uint64_t i = t0 + lane; i < end; i += kStrands) acc = clx_norm::dadd_rn(acc, sq(row[i]));
    } else {
        const rec m = t.term[w - n_windows];
        const uint32_t n = m.nc, P = m.P;
        if (t0 >= n) return;                                   // (the whole wave)
        const float* const row = m.nw + (uint64_t)r * T;
        const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
        uint32_t idx = (uint32_t)t0 + lane;                    // (below 2^32: t0 < n)
        if (n > P) idx %= P;                                   // (the whole wave: the term wraps)
        const uint32_t step = strand_step(P);
        for (uint64_t i = t0 + lane; i < end; i += kStrands) {
            acc = clx_norm::dadd_rn(acc, sq(row[idx]));
            idx = wrap_add(idx, step, P);
        }
    }
    acc = clx_norm::fold_strands(acc);
    if (lane == 0u) part[kr * n_chunks + c] = acc;
}

// Wave u: chunk u % n_chunks of unit u / n_chunks, every row; the windows are [T][rows].
extern "C" __global__ __launch_bounds__(256) void clx_k_addn_sum_tc(const float* __restrict__ x, const void* __restrict__ tab, double* part,
                                                                    uint32_t n_windows, uint32_t n_terms, uint32_t rows, uint32_t T,
                                                                    uint32_t n_chunks, uint64_t units) {
    using namespace clx_addn;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t u = (uint64_t)blockIdx.x * (kThreads / kStrands) + (threadIdx.x >> 6);
    if (u >= units) return;                                    // (the whole wave)
    const uint64_t w = u / n_chunks;
    const uint32_t c = (uint32_t)(u - w * n_chunks);
    const table t = table_of(tab, n_windows, n_terms);
    const uint64_t t0 = (uint64_t)c * kChunk;
    double acc[kMaxRows] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (w < n_windows) {
        const uint32_t n = t.vs[w];
        if (t0 >= n) return;                                   // (the whole wave)
        const float* const base = x + w * rows * T;
        const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
        for (uint64_t i = t0 + lane; i < end; i += kStrands) {
            const float* const p = base + i * rows;
#pragma unroll
            for (uint32_t r = 0; r < kMaxRows; ++r)
                if (r < rows) acc[r] = clx_norm::dadd_rn(acc[r], sq(p[r]));
        }
    } else {
        const rec m = t.term[w - n_windows];
        const uint32_t n = m.nc, P = m.P;
        if (t0 >= n) return;                                   // (the whole wave)
        const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
        uint32_t idx = (uint32_t)t0 + lane;
        if (n > P) idx %= P;                                   // (the whole wave: the term wraps)
        const uint32_t step = strand_step(P);
        for (uint64_t i = t0 + lane; i < end; i += kStrands) {
            const float* const p = m.nw + (uint64_t)idx * rows;
#pragma unroll
            for (uint32_t r = 0; r < kMaxRows; ++r)
                if (r < rows) acc[r] = clx_norm::dadd_rn(acc[r], sq(p[r]));
            idx = wrap_add(idx, step, P);
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < kMaxRows; ++r) {
        if (r >= rows) break;                                  // (the whole wave)
        const double a = clx_norm::fold_strands(acc[r]);
        if (lane == 0u) part[(w * rows + r) * n_chunks + c] = a;
    }
}

// Lane m of the grid: term m's gain, into gain (the context's) and gains (the caller's, may be null).
extern "C" __global__ __launch_bounds__(256) void clx_k_addn_gain(const void* __restrict__ tab, const double* __restrict__ part, float* gain,
                                                                  float* gains, uint32_t n_windows, uint32_t n_terms, uint32_t rows,
                                                                  uint32_t n_chunks) {
    using namespace clx_addn;
    using namespace clx_norm;
    const uint64_t m = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (m >= n_terms) return;
    const table t = table_of(tab, n_windows, n_terms);
    const uint32_t nc = t.term[m].nc;
    float g = 0.f;
    if (nc != 0u) {
        const uint32_t k = t.term[m].k, vs = t.vs[k];
        const double* const Ps = part + (uint64_t)k * rows * n_chunks;
        const double* const Pn = part + ((uint64_t)n_windows + m) * rows * n_chunks;
        const uint32_t ls = live_chunks(vs), ln = live_chunks(nc);
        double es = 0.0, en = 0.0;
        for (uint32_t r = 0; r < rows; ++r) {
            es = dadd_rn(es, fold_chunks(Ps + (uint64_t)r * n_chunks, ls));
            en = dadd_rn(en, fold_chunks(Pn + (uint64_t)r * n_chunks, ln));
        }
        if (es != 0.0 && en != 0.0)
            g = to_f32(dsqrt_rn(ddiv_rn(dmul_rn(dmul_rn(es, (double)nc), t.term[m].q), dmul_rn(en, (double)vs))));
    }
    gain[m] = g;
    if (gains) gains[m] = g;
}

// The apply pass, in place.  Block b: tile b % n_tiles of window b / n_tiles; the window's `rows * T` cells lie [rows][T] (tc == 0)
// or [T][rows] (tc == 1), the noise windows' too.
extern "C" __global__ __launch_bounds__(256) void clx_k_addn_apply(float* x, const void* __restrict__ tab, const float* __restrict__ gain,
                                                                   uint32_t n_windows, uint32_t n_terms, uint32_t rows, uint32_t T, uint32_t tc,
                                                                   uint32_t n_tiles) {
    using namespace clx_addn;
    const uint32_t tid = threadIdx.x, k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const table t = table_of(tab, n_windows, n_terms);
    if (t.vs[k] == 0u) return;                                 // (the whole block: no term of the window has a cover)
    const uint32_t m_lo = t.first[k], m_hi = t.first[k + 1u], lo = t.lo[k], hi = t.hi[k];
    bool any = false;
    for (uint32_t m = m_lo; m < m_hi; ++m) any = any || gain[m] != 0.f;
    if (!any) return;                                          // (the whole block: the window is not rewritten)
    const uint64_t cells = (uint64_t)rows * T;
    float* const w = x + (uint64_t)k * cells;
    const uint32_t head = (uint32_t)(((uintptr_t)w >> 2) & 3u);
    const uint64_t vectors = (cells + head + 3u) >> 2;
    const uint64_t v_lo = (uint64_t)tl * kApplyVecs;
    if (v_lo >= vectors) return;                               // (the whole block: n_tiles is sized for the largest head)
    const uint64_t v_hi = v_lo + kApplyVecs < vectors ? v_lo + kApplyVecs : vectors;
    // (the whole block: TC's cells inside the hull are the window's cells lo * rows .. hi * rows - 1)
    if (tc && (v_lo * 4u >= (uint64_t)hi * rows + head || v_hi * 4u <= (uint64_t)lo * rows + head)) return;
    const uint32_t inner = tc ? rows : T;                      // the cells of the faster axis
    for (uint32_t i = 0; i < kApplyVecs / kThreads; ++i) {
        const uint64_t v = v_lo + i * kThreads + tid;
        if (v >= v_hi) break;
        const int64_t e0 = (int64_t)(v * 4u) - (int64_t)head;
        float* const p = w + e0;                               // 16-byte aligned
        const uint64_t e = e0 < 0 ? 0u : (uint64_t)e0;         // the vector's first cell of the window: cell b0 of line a0
        uint32_t a0, b0;
        if (cells <= 0xffffffffull) { a0 = (uint32_t)e / inner; b0 = (uint32_t)e - a0 * inner; }
        else { a0 = (uint32_t)(e / inner); b0 = (uint32_t)(e - (uint64_t)a0 * inner); }
        uint32_t live = 0u;                                    // bit j: cell j of the vector is a cell of the window with lo <= t < hi
        {
            uint32_t a = a0, b = b0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e0 + j < 0 || (uint64_t)(e0 + j) >= cells) continue;
                const uint32_t tt = tc ? a : b;
                if (tt >= lo && tt < hi) live |= 1u << j;
                if (++b == inner) { b = 0u; ++a; }
            }
        }
        if (live == 0u) continue;
        const bool whole = live == 15u;
        // a whole vector whose cells' times ascend: t_first .. t_last (CT: the vector lies in one row)
        const bool ascending = whole && (tc || T - b0 > 3u);
        const uint32_t t_first = tc ? a0 : b0, t_last = tc ? a0 + (b0 + 3u) / rows : b0 + 3u;
        f4 q = { 0.f, 0.f, 0.f, 0.f };
        if (whole) q = *reinterpret_cast<const f4*>(p);
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live >> j & 1u) q[j] = p[j];
        }
        uint32_t touched = 0u;                                 // bit j: a term has been added to cell j
        for (uint32_t m = m_lo; m < m_hi; ++m) {
            const float g = gain[m];
            if (g == 0.f) continue;                            // (the whole block)
            const rec tm = t.term[m];
            const uint32_t off = tm.off, P = tm.P, end = off + tm.nc;
            if (ascending && (t_last < off || t_first >= end)) continue;
            uint32_t idx = 0u;                                 // the noise index of the cell at hand, once its time has reached off
            if (t_first >= off) {
                idx = t_first - off;
                if (idx >= P) idx %= P;                        // (the vector's one division)
            }
            if (ascending && t_first >= off && t_last < end && (uint64_t)idx + (t_last - t_first) < P) {
                const float* const pn = tc ? tm.nw + ((uint64_t)idx * rows + b0) : tm.nw + ((uint64_t)a0 * T + idx);
                f4 n4;
                if ((((uintptr_t)pn) & 15u) == 0u) n4 = *reinterpret_cast<const f4*>(pn);
                else { n4[0] = pn[0]; n4[1] = pn[1]; n4[2] = pn[2]; n4[3] = pn[3]; }
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = fma_rn(g, n4[j], q[j]);
                touched = 15u;
                continue;
            }
            uint32_t a = a0, b = b0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e0 + j < 0 || (uint64_t)(e0 + j) >= cells) continue;
                const uint32_t tt = tc ? a : b, r = tc ? b : a;
                if ((live >> j & 1u) && tt >= off && tt < end) {
                    const float nv = tc ? tm.nw[(uint64_t)idx * rows + r] : tm.nw[(uint64_t)r * T + idx];
                    q[j] = fma_rn(g, nv, q[j]);
                    touched |= 1u << j;
                }
                if (++b == inner) { b = 0u; ++a; }
                const uint32_t tn = tc ? a : b;                // the next cell's time: the same, one more, or 0 (CT: the next row)
                if (tn == tt + 1u) {
                    if (tn > off && ++idx == P) idx = 0u;
                } else if (tn != tt) idx = 0u;
            }
        }
        if (touched == 0u) continue;
        if (whole) *reinterpret_cast<f4*>(p) = q;
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (touched >> j & 1u) p[j] = q[j];
        }
    }
}

// The host side of clx_addn_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the launch
// shape (p->n_chunks == 0: nothing to launch).
inline const char* clx_addn_check(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const void* const* noise,
                                  const size_t* n_noise, uint32_t n_batches, const uint32_t* noise_valid, const uint32_t* term_first,
                                  const clx_addn_term* terms, uint32_t layout, const clx_addn_opts* o, clx_addn_plan* p) {
    using namespace clx_addn;
    *p = clx_addn_plan();
    if (o && o->reserved != 0u) return "clx_addn_windows: opts must be NULL or all zero";
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return "clx_addn_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT";
    if (rows < 1u || rows > kMaxRows) return "clx_addn_windows: rows must be 1..8";
    if (n_batches > kMaxBatches) return "clx_addn_windows: more than 8 noise batches";
    if (n_windows == 0 || T == 0) return nullptr;
    if (!valid) return "clx_addn_windows: valid is null";
    if (!term_first) return "clx_addn_windows: term_first is null";
    if (n_windows > 0x7fffffffull) return "clx_addn_windows: too many windows in one call";
    if (term_first[0] != 0u) return "clx_addn_windows: term_first[0] must be 0";
    for (size_t k = 0; k < n_windows; ++k) {
        if (term_first[k + 1] < term_first[k]) return "clx_addn_windows: term_first must not descend";
        if (term_first[k + 1] - term_first[k] > kMaxTerms) return "clx_addn_windows: more than 16 terms in a window";
        if (valid[k] > T) return "clx_addn_windows: valid[k] is larger than T";
    }
    const uint32_t M = term_first[n_windows];
    if (M == 0u) return nullptr;
    if (!terms) return "clx_addn_windows: terms is null";
    if (n_batches > 0u && !n_noise) return "clx_addn_windows: n_noise is null";
    uint64_t total = 0;
    for (uint32_t b = 0; b < n_batches; ++b) {
        if (n_noise[b] > 0x7fffffffull) return "clx_addn_windows: too many windows in one call";
        total += n_noise[b];
    }
    bool work = false;
    for (uint32_t m = 0; m < M; ++m) {
        const clx_addn_term& tm = terms[m];
        if (tm.loop > 1u) return "clx_addn_windows: terms[m].loop must be 0 or 1";
        const float s = tm.snr_db;
        if (std::isnan(s)) return "clx_addn_windows: terms[m].snr_db is NaN";
        if (std::isinf(s) ? s < 0.f : std::fabs((double)s) > kMaxSnr) return "clx_addn_windows: terms[m].snr_db must be within -200 .. 200, or +inf";
        if (tm.index < -1) return "clx_addn_windows: terms[m].index is below -1";
        if (tm.index < 0) continue;
        if (tm.batch < 0 || (uint32_t)tm.batch >= n_batches) return "clx_addn_windows: terms[m].batch must be 0 .. n_batches - 1";
        if ((uint64_t)tm.index >= n_noise[tm.batch]) return "clx_addn_windows: terms[m].index is outside its batch (n_noise[batch])";
        work = true;
    }
    if (!work) return nullptr;
    if (!data) return "clx_addn_windows: d_data is null";
    if (!noise) return "clx_addn_windows: d_noise is null";
    if (!noise_valid) return "clx_addn_windows: noise_valid is null";
    for (uint32_t m = 0; m < M; ++m)
        if (terms[m].index >= 0 && !noise[terms[m].batch]) return "clx_addn_windows: a term names a noise batch whose pointer is null";
    for (uint64_t j = 0; j < total; ++j)
        if (noise_valid[j] > T) return "clx_addn_windows: noise_valid[j] is larger than T";
    const uint64_t nc = ((uint64_t)T + kChunk - 1u) / kChunk;
    const uint32_t tc = layout == CLX_WINDOW_TC && rows > 1u ? 1u : 0u;
    const uint64_t partials = ((uint64_t)n_windows + M) * rows * nc;
    const uint64_t units = tc ? ((uint64_t)n_windows + M) * nc : partials;
    const uint64_t sum_blocks = (units + 3u) / 4u;
    const uint64_t cells = (uint64_t)rows * T, tiles = (((cells + 6u) >> 2) + kApplyVecs - 1u) / kApplyVecs;   // (at most (cells + 6) / 4 vectors)
    if (partials > 0x7fffffffull || tiles * (uint64_t)n_windows > 0x7fffffffull) return "clx_addn_windows: too many windows in one call";
    p->n_chunks = (uint32_t)nc; p->tc = tc; p->n_terms = M; p->units = units; p->sum_blocks = (uint32_t)sum_blocks;
    p->gain_blocks = (uint32_t)((M + kThreads - 1u) / kThreads); p->n_tiles = (uint32_t)tiles; p->partials = partials;
    p->table_bytes = table_bytes(n_windows, M);
    return nullptr;
}

// The per-call table of checked arguments, clx_addn::table_bytes(n_windows, M) bytes, into `tab` (8-byte aligned).
inline void clx_addn_fill(void* tab, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const void* const* noise,
                          const size_t* n_noise, uint32_t n_batches, const uint32_t* noise_valid, const uint32_t* term_first,
                          const clx_addn_term* terms) {
    using namespace clx_addn;
    const uint32_t M = term_first[n_windows];
    rec* const term = (rec*)tab;
    uint32_t* const vs = (uint32_t*)(term + M);
    uint32_t* const first = vs + n_windows;
    uint32_t* const lo = first + n_windows + 1u;
    uint32_t* const hi = lo + n_windows;
    uint64_t base[kMaxBatches + 1u] = { 0 };                   // where a batch's windows start in noise_valid
    for (uint32_t b = 0; b < n_batches; ++b) base[b + 1u] = base[b] + n_noise[b];
    for (size_t k = 0; k < n_windows; ++k) {
        const uint32_t Vs = valid[k];
        uint32_t l = 0xffffffffu, h = 0u;
        for (uint32_t m = term_first[k]; m < term_first[k + 1]; ++m) {
            const clx_addn_term& tm = terms[m];
            rec& r = term[m];
            r.q = std::isinf(tm.snr_db) ? 0.0 : pow(10.0, -(double)tm.snr_db / 10.0);
            r.nw = nullptr; r.off = tm.offset; r.P = 0u; r.nc = 0u; r.k = (uint32_t)k;
            if (tm.index < 0 || r.q == 0.0) continue;
            r.P = noise_valid[base[tm.batch] + (uint32_t)tm.index];
            if (tm.offset >= Vs || r.P == 0u) continue;
            const uint64_t e = tm.loop || (uint64_t)tm.offset + r.P > Vs ? Vs : (uint64_t)tm.offset + r.P;
            r.nc = (uint32_t)e - tm.offset;
            r.nw = (const float*)noise[tm.batch] + (uint64_t)(uint32_t)tm.index * rows * T;
            l = tm.offset < l ? tm.offset : l;
            h = (uint32_t)e > h ? (uint32_t)e : h;
        }
        first[k] = term_first[k];
        vs[k] = h ? Vs : 0u;
        lo[k] = h ? l : 0u;
        hi[k] = h;
    }
    first[n_windows] = M;
}
