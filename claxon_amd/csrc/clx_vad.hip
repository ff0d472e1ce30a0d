// clx_vad.hip -- Kaldi's energy VAD (compute-vad) over one row of a dense float32 feature batch, clx_vad_windows, and the selection of
// the frames a byte mask names (select-voiced-frames, or any mask), clx_select_windows: a stream compaction along the time axis.
// claxon_hip.h has the definitions; this is how they are computed.  The sum of the energy row is clx_norm's: this
// file stands behind clx_norm.hip in a translation unit and uses its dadd_rn, ddiv_rn, dmul_rn, to_f32, fold_strands, fold_chunks
// and live_chunks, so the order of the sum is that file's, chunk for chunk.
//
// The decision, two launches (one when energy_mean_scale == 0: nothing is summed then):
//   clx_k_vad_sum     a wave is one chunk (kChunk = 4096 frames) of one window's energy row: clx_norm's sum_ct over that row alone,
//                     the cells `stride` floats apart (1 in CT, rows in TC).  Partials [n_windows][n_chunks] doubles.  No LDS.
//   clx_k_vad_decide  a block is a tile of kTile = 256 frames [t0, t0 + 256) of one window.  A tile with t0 >= V stores zero bytes
//                     and loads nothing.  Otherwise every lane folds the window's partials into thr (one address a wave) and the
//                     block of tile 0 stores it.  The tile's span is the frames [max(t0 - c, 0), min(t0 + 256 + c, V)), at most
//                     kSpan = 512: two cells a lane, their `above` flags taken by two ballots a wave.  A lane's inclusive count in
//                     its wave's 64 frames is one popcount of the ballot under a lane mask; the eight segment totals cross LDS
//                     (32 bytes) and every lane adds those in front of its segment: s_pre[i] = the number of `above` among the
//                     span's frames 0..i, 512 words.  Then one lane a frame: num = s_pre[hi - lo0] - s_pre[lo - lo0 - 1], two
//                     LDS reads at consecutive addresses across the lanes (no bank conflict), whatever c is: no lane loops over
//                     its context.  One byte store a frame.  LDS: 2 080 bytes.
//
// The selection, three launches:
//   clx_k_select_rank  a block is a tile of 256 source frames: the ballot of the live mask bytes, the four waves' popcounts through
//                      LDS (16 bytes), their sum into tile_counts[n_windows][n_tiles].
//   clx_k_select_scan  a wave is one window: the exclusive ascending scan of its tile counts, 64 at a step (six shuffles), into
//                      tile_base; the total into count[n_windows] (and the caller's d_counts).  No LDS.
//   clx_k_select_move  a block is a source tile again.  It takes the ballots once more (256 mask bytes: cheaper than a table of
//                      ranks through memory); a selected frame's place in the tile is the popcount of the ballot below its lane
//                      plus the earlier waves' counts, and the tile's list of selected source frames is left in LDS (1 KiB).  The
//                      lanes then run along the OUTPUT's contiguous axis: in CT lane j takes output frame tile_base + j and walks
//                      the rows (stores of consecutive words; loads gathered from at most 1 KiB of a source row), in TC the lanes
//                      run over the cnt * rows contiguous words of the tile's output run (loads contiguous inside a frame).
//                      Block i also stores the pad into output frames [max(count, 256 i), min(256 (i + 1), T)): every output
//                      cell has exactly one writer.  Words are copied as 32-bit integers.  LDS: 1 040 bytes.
// The scan stays a launch of its own: folded into the mover's prologue every block would add up the counts in front of its tile,
// which is quadratic in the tiles of a long window; merged into the rank it would need a second pass or a wait between blocks.
//
// No scratch, no spills, wave64, blocks of 256 (tests/test_code_object_vad.py reads them from the code object).
// clx_vad_check and clx_select_check are the host side (plain C++, shared with the wave simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>

#include "../../include/claxon_hip.h"

// the launch shapes clx_vad_check / clx_select_check give (n_tiles == 0: nothing to launch)
struct clx_vad_plan {
    uint32_t n_tiles = 0;        // tiles of a window (n_windows * n_tiles blocks)
    uint32_t n_chunks = 0;       // decision: chunks of the time axis
    uint32_t sum_blocks = 0;     // decision: blocks of the sum pass (0: energy_mean_scale == 0, no sum pass)
    uint32_t scan_blocks = 0;    // selection: blocks of the scan
    uint32_t tc = 0;             // 1: [n_windows][T][rows]
    uint64_t partials = 0;       // decision: doubles of the partial sums, [n_windows][n_chunks]
    uint64_t table_words = 0;    // 32-bit words of the per-call table: V[n_windows]; selection: then count[n_windows],
                                 // tile_counts[n_windows][n_tiles], tile_base[n_windows][n_tiles]
};

namespace clx_vad {

constexpr uint32_t kThreads = 256u, kTile = 256u, kMaxContext = 128u, kMaxRows = 8192u, kMaxT = 0x7fffffffu;
constexpr uint32_t kSpan = kTile + 2u * kMaxContext;                       // 512 frames
constexpr uint32_t kSegs = kSpan / 64u;                                    // 8 wave-sized segments of a span
constexpr uint32_t kSumLdsBytes = 0u, kScanLdsBytes = 0u;
constexpr uint32_t kDecideLdsBytes = kSpan * 4u + kSegs * 4u;              // 2 080
constexpr uint32_t kRankLdsBytes = (kThreads / 64u) * 4u;                  // 16
constexpr uint32_t kMoveLdsBytes = kTile * 4u + (kThreads / 64u) * 4u;     // 1 040
static_assert(kTile == kThreads && kSpan == 2u * kThreads, "a lane is one frame of the tile and two of the span");
static_assert(kDecideLdsBytes == 2080u && kMoveLdsBytes == 1040u, "the header states these");

// one float32 product, rounded once
#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
#else
inline float mul_rn(float a, float b) { return a * b; }
#endif

// the context [lo, hi] of live frame t < V (claxon_hip.h): 0 <= lo <= t <= hi < V, hi - lo + 1 == 2 c + 1 away from the edges
__host__ __device__ __forceinline__ void context(uint32_t t, uint32_t V, uint32_t c, uint32_t* lo, uint32_t* hi) {
    *lo = t > c ? t - c : 0u;
    *hi = V - 1u - t > c ? t + c : V - 1u;
}

// thr of a window with V > 0 live frames whose energy row sums to S
__device__ __forceinline__ float threshold(float E, float s, double S, uint32_t V) {
    using namespace clx_norm;
    return to_f32(dadd_rn((double)E, dmul_rn((double)s, ddiv_rn(S, (double)V))));
}

}  // namespace clx_vad

// Wave u of the grid: chunk u % n_chunks of the energy row of window u / n_chunks.  part is [n_windows][n_chunks].  A chunk
// without a live frame is neither read nor written.
extern "C" __global__ __launch_bounds__(256) void clx_k_vad_sum(const float* __restrict__ x, const uint32_t* __restrict__ valid, double* part,
                                                                uint32_t rows, uint32_t T, uint32_t row, uint32_t tc, uint32_t n_chunks,
                                                                uint64_t units) {
    using namespace clx_norm;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t u = (uint64_t)blockIdx.x * (clx_vad::kThreads / kStrands) + (threadIdx.x >> 6);
    if (u >= units) return;                                    // (the whole wave)
    const uint64_t k = u / n_chunks;
    const uint32_t c = (uint32_t)(u - k * n_chunks), n = valid[k];
    const uint64_t t0 = (uint64_t)c * kChunk;
    if (t0 >= n) return;                                       // (the whole wave)
    const float* const e = x + k * rows * T + (tc ? (uint64_t)row : (uint64_t)row * T);
    const uint64_t stride = tc ? rows : 1u;
    const uint64_t end = t0 + kChunk < n ? t0 + kChunk : n;
    double acc = 0.0;
    for (uint64_t t = t0 + lane; t < end; t += kStrands) acc = dadd_rn(acc, (double)e[t * stride]);
    acc = fold_strands(acc);
    if (lane == 0u) part[k * n_chunks + c] = acc;
}

// Block b: tile b % n_tiles of window b / n_tiles.  mask is [n_windows][T] bytes, thresholds (may be null) [n_windows].
extern "C" __global__ __launch_bounds__(256) void clx_k_vad_decide(const float* __restrict__ x, const uint32_t* __restrict__ valid,
                                                                   const double* __restrict__ part, uint8_t* mask, float* thresholds,
                                                                   clx_vad_opts o, uint32_t rows, uint32_t T, uint32_t tc, uint32_t n_chunks,
                                                                   uint32_t n_tiles) {
    using namespace clx_vad;
    __shared__ uint32_t s_pre[kSpan];
    __shared__ uint32_t s_seg[kSegs];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const uint32_t V = valid[k];
    const uint32_t t0 = tl * kTile, t1 = T - t0 < kTile ? T : t0 + kTile, t = t0 + tid;
    uint8_t* const m = mask + (uint64_t)k * T;
    if (t0 >= V) {                                             // (the whole block) only zero bytes; tile 0 of an empty window: thr = E
        if (tl == 0u && tid == 0u && thresholds) thresholds[k] = o.energy_threshold;
        if (t < t1) m[t] = 0u;
        return;
    }
    float thr = o.energy_threshold;
    if (o.energy_mean_scale != 0.f)
        thr = threshold(o.energy_threshold, o.energy_mean_scale, clx_norm::fold_chunks(part + (uint64_t)k * n_chunks, clx_norm::live_chunks(V)), V);
    if (tl == 0u && tid == 0u && thresholds) thresholds[k] = thr;
    const uint32_t c = o.frames_context;
    const uint32_t lo0 = t0 > c ? t0 - c : 0u, hi0 = V - t0 > kTile + c ? t0 + kTile + c : V, n_span = hi0 - lo0;   // (n_span <= kSpan)
    const float* const e = x + (uint64_t)k * rows * T + (tc ? (uint64_t)o.row : (uint64_t)o.row * T);
    const uint64_t stride = tc ? rows : 1u;
    uint32_t incl[2];
#pragma unroll
    for (uint32_t q = 0; q < 2u; ++q) {                        // frame i of the span: segment q * 4 + w
        const uint32_t i = q * kThreads + tid;
        const bool above = i < n_span && e[(uint64_t)(lo0 + i) * stride] > thr;
        const unsigned long long b = __ballot(above);
        incl[q] = (uint32_t)__popcll(b & (~0ull >> (63u - lane)));
        if (lane == 0u) s_seg[q * 4u + w] = (uint32_t)__popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < 2u; ++q) {
        uint32_t base = 0u;
        for (uint32_t g = 0; g < q * 4u + w; ++g) base += s_seg[g];
        s_pre[q * kThreads + tid] = base + incl[q];
    }
    __syncthreads();
    if (t >= t1) return;
    uint32_t voiced = 0u;
    if (t < V) {
        uint32_t lo, hi;
        context(t, V, c, &lo, &hi);
        const uint32_t num = s_pre[hi - lo0] - (lo > lo0 ? s_pre[lo - lo0 - 1u] : 0u), den = hi - lo + 1u;
        voiced = (float)num >= mul_rn((float)den, o.proportion_threshold) ? 1u : 0u;
    }
    m[t] = (uint8_t)voiced;
}

// Block b: tile b % n_tiles of window b / n_tiles; tile_counts[b] = the selected frames of the tile.
extern "C" __global__ __launch_bounds__(256) void clx_k_select_rank(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ valid,
                                                                    uint32_t* tile_counts, uint32_t T, uint32_t n_tiles) {
    using namespace clx_vad;
    __shared__ uint32_t s_w[kThreads / 64u];
    const uint32_t tid = threadIdx.x, k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const uint32_t V = valid[k], t = tl * kTile + tid;
    const bool sel = t < V && mask[(uint64_t)k * T + t] != 0u;
    const unsigned long long b = __ballot(sel);
    if ((tid & 63u) == 0u) s_w[tid >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (tid == 0u) tile_counts[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// Wave u of the grid: window u.  tile_base[u][i] = the tile counts in front of tile i; count[u] (and d_counts[u]) = their total.
extern "C" __global__ __launch_bounds__(256) void clx_k_select_scan(const uint32_t* __restrict__ tile_counts, uint32_t* tile_base, uint32_t* count,
                                                                    uint32_t* d_counts, uint32_t n_windows, uint32_t n_tiles) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k = (uint64_t)blockIdx.x * (clx_vad::kThreads / 64u) + (threadIdx.x >> 6);
    if (k >= n_windows) return;                                // (the whole wave)
    const uint32_t* const cn = tile_counts + k * n_tiles;
    uint32_t* const bs = tile_base + k * n_tiles;
    uint32_t run = 0u;
    for (uint32_t i0 = 0; i0 < n_tiles; i0 += 64u) {           // (the bound is the whole wave's)
        const uint32_t i = i0 + lane, v = i < n_tiles ? cn[i] : 0u;
        uint32_t s = v;
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(s, d);
            if (lane >= d) s += up;
        }
        if (i < n_tiles) bs[i] = run + s - v;
        run += __shfl(s, 63);
    }
    if (lane == 0u) {
        count[k] = run;
        if (d_counts) d_counts[k] = run;
    }
}

// Block b: source tile b % n_tiles of window b / n_tiles.  src and dst are [n_windows][rows][T] (tc == 0) or [n_windows][T][rows]
// words; pad is the word of every output frame from count on.
extern "C" __global__ __launch_bounds__(256) void clx_k_select_move(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                                    const uint8_t* __restrict__ mask, const uint32_t* __restrict__ valid,
                                                                    const uint32_t* __restrict__ tile_base, const uint32_t* __restrict__ count,
                                                                    uint32_t rows, uint32_t T, uint32_t pad, uint32_t tc, uint32_t n_tiles) {
    using namespace clx_vad;
    __shared__ uint32_t s_list[kTile];
    __shared__ uint32_t s_w[kThreads / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t k = blockIdx.x / n_tiles, tl = blockIdx.x - k * n_tiles;
    const uint32_t V = valid[k], t0 = tl * kTile, t1 = T - t0 < kTile ? T : t0 + kTile, t = t0 + tid;
    const bool sel = t < V && mask[(uint64_t)k * T + t] != 0u;
    const unsigned long long b = __ballot(sel);
    if (lane == 0u) s_w[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t g = 0; g < w; ++g) before += s_w[g];
    const uint32_t cnt = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    if (sel) s_list[before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = t;
    __syncthreads();
    const uint32_t base = tile_base[blockIdx.x], total = count[k];         // (base + cnt <= total <= V)
    const uint32_t* const x = src + (uint64_t)k * rows * T;
    uint32_t* const y = dst + (uint64_t)k * rows * T;
    const uint32_t p0 = total > t0 ? total : t0;                           // the pad of this tile: output frames [p0, t1)
    if (!tc) {
        if (tid < cnt) {
            const uint32_t* const xs = x + s_list[tid];
            uint32_t* const yo = y + base + tid;
#pragma unroll 4
            for (uint32_t r = 0; r < rows; ++r) yo[(uint64_t)r * T] = xs[(uint64_t)r * T];
        }
        if (t >= p0 && t < t1) {
            uint32_t* const yo = y + t;
#pragma unroll 4
            for (uint32_t r = 0; r < rows; ++r) yo[(uint64_t)r * T] = pad;
        }
    } else {
        const uint32_t n = cnt * rows;                                     // (at most 256 * 8192 words)
        uint32_t* const yo = y + (uint64_t)base * rows;
        for (uint32_t e = tid; e < n; e += kThreads) {
            const uint32_t j = e / rows, r = e - j * rows;
            yo[e] = x[(uint64_t)s_list[j] * rows + r];
        }
        if (p0 < t1) {
            const uint32_t np = (t1 - p0) * rows;
            uint32_t* const yp = y + (uint64_t)p0 * rows;
            for (uint32_t e = tid; e < np; e += kThreads) yp[e] = pad;
        }
    }
}

// What both calls refuse alike; `who` is 0 for the decision and 1 for the selection.
#define CLX_VAD_WHO(text) (who ? "clx_select_windows: " text : "clx_vad_windows: " text)
inline const char* clx_vad_check_common(int who, uint32_t layout, uint32_t rows, uint32_t T) {
    using namespace clx_vad;
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return CLX_VAD_WHO("layout must be CLX_WINDOW_TC or CLX_WINDOW_CT");
    if (rows < 1u || rows > kMaxRows) return CLX_VAD_WHO("rows must be 1..8192");
    if (T > kMaxT) return CLX_VAD_WHO("n_frames must be below 2^31");
    return nullptr;
}

inline const char* clx_vad_check_valid(int who, size_t n_windows, uint32_t T, const uint32_t* valid, uint64_t* tiles) {
    for (size_t k = 0; k < n_windows; ++k)
        if (valid[k] > T) return CLX_VAD_WHO("valid[k] is larger than n_frames");
    *tiles = ((uint64_t)T + clx_vad::kTile - 1u) / clx_vad::kTile;
    if (n_windows > 0x7fffffffull || *tiles * (uint64_t)n_windows > 0x7fffffffull) return CLX_VAD_WHO("too many tiles in one call");
    return nullptr;
}
#undef CLX_VAD_WHO

// The host side of clx_vad_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the launch
// shape (p->n_tiles == 0: nothing to launch).
inline const char* clx_vad_check(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                 const clx_vad_opts* o, const void* mask, clx_vad_plan* p) {
    using namespace clx_vad;
    *p = clx_vad_plan();
    if (!o) return "clx_vad_windows: null options";
    if (o->reserved[0] != 0u || o->reserved[1] != 0u || o->reserved[2] != 0u) return "clx_vad_windows: reserved must be 0";
    if (!std::isfinite(o->energy_threshold)) return "clx_vad_windows: energy_threshold must be finite";
    if (!std::isfinite(o->energy_mean_scale)) return "clx_vad_windows: energy_mean_scale must be finite";
    if (!(o->proportion_threshold > 0.f && o->proportion_threshold < 1.f)) return "clx_vad_windows: proportion_threshold must be above 0 and below 1";
    if (o->frames_context > kMaxContext) return "clx_vad_windows: frames_context must be 0..128";
    if (const char* why = clx_vad_check_common(0, layout, rows, T)) return why;
    if (o->row >= rows) return "clx_vad_windows: row must be below rows";
    if (n_windows == 0 || T == 0) return nullptr;
    if (!data || !valid || !mask) return "clx_vad_windows: null argument";
    uint64_t tiles = 0;
    if (const char* why = clx_vad_check_valid(0, n_windows, T, valid, &tiles)) return why;
    const uint64_t nc = ((uint64_t)T + clx_norm::kChunk - 1u) / clx_norm::kChunk, units = (uint64_t)n_windows * nc;
    p->n_tiles = (uint32_t)tiles; p->n_chunks = (uint32_t)nc; p->tc = layout == CLX_WINDOW_TC ? 1u : 0u;
    if (o->energy_mean_scale != 0.f) { p->sum_blocks = (uint32_t)((units + 3u) / 4u); p->partials = units; }
    p->table_words = (uint64_t)n_windows;
    return nullptr;
}

// The host side of clx_select_windows, likewise.
inline const char* clx_select_check(const void* src, const void* dst, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid,
                                    const void* mask, uint32_t layout, const clx_select_opts* o, clx_vad_plan* p) {
    using namespace clx_vad;
    *p = clx_vad_plan();
    if (!o) return "clx_select_windows: null options";
    if (o->reserved[0] != 0u || o->reserved[1] != 0u || o->reserved[2] != 0u) return "clx_select_windows: reserved must be 0";
    if (const char* why = clx_vad_check_common(1, layout, rows, T)) return why;
    if (n_windows == 0 || T == 0) return nullptr;
    if (!src || !dst || !valid || !mask) return "clx_select_windows: null argument";
    uint64_t tiles = 0;
    if (const char* why = clx_vad_check_valid(1, n_windows, T, valid, &tiles)) return why;
    const uint64_t bytes = (uint64_t)n_windows * rows * T * 4u;            // (n_windows * T is below 2^40 here, rows at most 2^13: no overflow)
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    if (a < b ? b - a < bytes : a - b < bytes) return "clx_select_windows: d_dst must not overlap d_src";
    p->n_tiles = (uint32_t)tiles; p->tc = layout == CLX_WINDOW_TC ? 1u : 0u;
    p->scan_blocks = (uint32_t)(((uint64_t)n_windows + 3u) / 4u);
    p->table_words = 2u * (uint64_t)n_windows + 2u * (uint64_t)n_windows * tiles;
    return nullptr;
}
