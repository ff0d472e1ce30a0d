// clx_resample.hip -- a dense batch of fixed-length sample windows at a target sample rate, resampled from CLX_OUT_F32 audio while
// they are cut out of it, in one launch.
//
// The resampler is fixed: band-limited interpolation with a Hann-windowed sinc, lowpass_filter_width 6 and rolloff 0.99 (the
// defaults of torchaudio.functional.resample), in its direct form.  For a source rate fs and a target rate R, g = gcd(fs, R),
// o = fs / g, n = R / g, base = min(o, n) * 0.99, W = ceil(6 * o / base):
//     h(d) = sinc(t) * cos^2(pi * t / 12) * base / o      with t = d * base / o, and 0 where |t| >= 6
//     y[m] = sum over s of x[s] * h(s - m * o / n)        x = 0 outside the stream; channels are independent
// Only the 2W taps s = fc - W + 1 + k, k = 0 .. 2W - 1, fc = floor(m * o / n), can be non-zero, and their coefficients depend on the
// phase i = m mod n alone: the table of a pair is [n][2W], built on the host in double and rounded once to float32; row i entry k is
// h(floor(i * o / n) - W + 1 + k - i * o / n).  Rows are padded with zeros to a multiple of four floats so that a row is read with
// 16-byte loads.  The kernel accumulates in float32, taps in ascending k, one fmaf each.
//
// The source is channel-interleaved float32.  Window k's job says where its source span lies: src_n samples per channel from float
// src_first on, the first of them stream sample src_t0; a tap outside [src_t0, src_t0 + src_n) counts as zero and is never loaded,
// so no float outside [src_first, src_first + src_n * C) is read.  Outputs out_t0 .. out_t0 + valid - 1 of the resampled stream are
// computed, the rest of the window (up to L) is zeros: the kernel owns every float of the [B, L, C] / [B, C, L] output.  `rate`
// picks the pair from a table of (o, n, W, table offset); entry 0 is reserved for "copy" (fs == R): output m is source sample m,
// moved as a 32-bit word -- not a pass through a 1/1 filter.  One launch serves windows of different pairs, copies included.
//
// The grid is (window, tile): a tile is kTile consecutive outputs of all C channels; block b is tile b % n_tiles of window
// b / n_tiles.  m * o needs 64 bits: the block divides once, for the tile's first output, and a lane derives its own fc and phase
// from the quotient and remainder in 32-bit arithmetic (j * o + r0 < 2^32 for j < kTile: why rates are bounded by 2^20).  A lane
// takes one output float at a time, lanes along the output row in either layout, so a wave stores 64 consecutive floats; its loads
// are direct global loads: neighbouring lanes read overlapping source runs (the vector L1 serves the overlap) and one table row each.
//
// The host side (plain C++, shared with the wave simulator): clx_resample_pair and clx_resample_table (a pair's sizes and
// coefficients), clx_resample_plan (the argument checks and the launch shape), clx_resample_fill (the job and rate tables).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/claxon_hip.h"

struct clx_rs_job {
    uint64_t src_first;      // float index in the source of the span's first sample, channel 0
    int64_t src_t0;          // the stream sample that is
    uint64_t out_t0;         // the window's first output sample, counted at the target rate
    uint32_t src_n;          // samples per channel in the span
    uint32_t valid;          // outputs to compute (<= the window length); the rest of the window is zeros
    uint32_t rate;           // index into the rate table (0: copy)
    uint32_t reserved;
};

struct clx_rs_rate {
    uint32_t o, n, W;        // the reduced pair and the filter's half width in source samples (W == 0: copy)
    uint32_t off;            // the pair's table: n rows of clx_rs::row_stride(W) floats from float `off` of the coefficients
};

namespace clx_rs {

constexpr uint32_t kThreads = 256u, kTile = 1024u;
constexpr uint32_t kRateLimit = 1u << 20, kMaxEntries = 1u << 18;
constexpr uint64_t kMaxCoef = 1ull << 30;                    // floats of all the tables a cache may hold (offsets are 32-bit)
constexpr uint64_t kMaxOut = 1ull << 43;                     // out_t0 + L below this: m * o stays inside 64 bits

__host__ __device__ __forceinline__ uint32_t row_stride(uint32_t W) { return (2u * W + 3u) & ~3u; }

__device__ __forceinline__ void ld16f(float* v, const float* p) { memcpy(v, __builtin_assume_aligned(p, 16), 16); }   // (16-byte aligned)

}  // namespace clx_rs

// Block b: tile b % n_tiles of window b / n_tiles (clx_resample_plan gives n_tiles).  `out` is the dense [B, L, C] / [B, C, L] batch.
extern "C" __global__ __launch_bounds__(256) void clx_k_resample(const float* __restrict__ src, const clx_rs_job* __restrict__ jobs,
                                                      const clx_rs_rate* __restrict__ rates, const float* __restrict__ coef, uint32_t n_tiles,
                                                      uint32_t L, uint32_t C, uint32_t layout, float* __restrict__ out) {
    using namespace clx_rs;
    const uint32_t w = blockIdx.x / n_tiles, tile = blockIdx.x - w * n_tiles;
    const clx_rs_job job = jobs[w];
    const clx_rs_rate R = rates[job.rate];
    const uint32_t t_lo = tile * kTile, nT = L - t_lo < kTile ? L - t_lo : kTile;
    const float* const s = src + job.src_first;
    float* const o = out + (uint64_t)w * L * C;
    const bool tc = layout == CLX_WINDOW_TC;
    const uint32_t total = nT * C;
    const uint64_t m0 = job.out_t0 + t_lo;                        // the tile's first output

    if (R.W == 0u) {                                              // copy: output m is source sample m
        const int64_t d0 = (int64_t)m0 - job.src_t0;
        const uint32_t* const sw = reinterpret_cast<const uint32_t*>(s);
        uint32_t* const ow = reinterpret_cast<uint32_t*>(o);
        for (uint32_t e = threadIdx.x; e < total; e += kThreads) {
            const uint32_t a = e / (tc ? C : nT), b = e - a * (tc ? C : nT);
            const uint32_t j = tc ? a : b, c = tc ? b : a;
            const int64_t rel = d0 + j;
            uint32_t v = 0u;
            if (t_lo + j < job.valid && rel >= 0 && rel < (int64_t)job.src_n) v = sw[(uint64_t)rel * C + c];
            ow[tc ? (uint64_t)t_lo * C + e : (uint64_t)c * L + t_lo + j] = v;
        }
        return;
    }

    // the one 64-bit divide: m0 * o = q0 * n + r0, and the tile's first phase
    const uint64_t p0 = m0 * R.o, q0 = p0 / R.n;
    const uint32_t r0 = (uint32_t)(p0 - q0 * R.n), i0 = (uint32_t)(m0 % R.n);
    const int64_t d0 = (int64_t)q0 - (int64_t)(R.W - 1u) - job.src_t0;      // tap 0 of the tile's first output, counted from the span's start
    const int32_t taps = (int32_t)(2u * R.W);
    const uint32_t stride = row_stride(R.W);
    const float* const tab = coef + R.off;
    for (uint32_t e = threadIdx.x; e < total; e += kThreads) {
        const uint32_t a = e / (tc ? C : nT), b = e - a * (tc ? C : nT);
        const uint32_t j = tc ? a : b, c = tc ? b : a;
        float acc = 0.0f;
        if (t_lo + j < job.valid) {
            const int64_t rel = d0 + (int64_t)((r0 + j * R.o) / R.n);       // tap 0 of this output, counted from the span's start
            const int64_t lo = -rel, hi = (int64_t)job.src_n - rel;         // taps lo <= k < hi lie in the span
            const int32_t klo = lo <= 0 ? 0 : lo >= taps ? taps : (int32_t)lo;
            const int32_t khi = hi <= 0 ? 0 : hi >= taps ? taps : (int32_t)hi;
            const float* const h = tab + (uint64_t)((i0 + j) % R.n) * stride;
            for (int32_t k4 = klo & ~3; k4 < khi; k4 += 4) {
                float hv[4];
                ld16f(hv, h + k4);
                const int64_t at = (rel + k4) * (int64_t)C + c;             // the float of tap k4 (only looked at where the tap is in the span)
                if (k4 >= klo && k4 + 4 <= khi) {
                    const float x0 = s[at], x1 = s[at + C], x2 = s[at + 2 * (int64_t)C], x3 = s[at + 3 * (int64_t)C];
                    acc = fmaf(x0, hv[0], acc);
                    acc = fmaf(x1, hv[1], acc);
                    acc = fmaf(x2, hv[2], acc);
                    acc = fmaf(x3, hv[3], acc);
                } else {
#pragma unroll
                    for (int32_t i = 0; i < 4; ++i)
                        if (k4 + i >= klo && k4 + i < khi) acc = fmaf(s[at + i * (int64_t)C], hv[i], acc);
                }
            }
        }
        o[tc ? (uint64_t)t_lo * C + e : (uint64_t)c * L + t_lo + j] = acc;
    }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------

// The coefficient tables a context has built, one per (o, n): pairs[i].off is the table's first float in `coef`.
struct clx_rs_cache {
    std::vector<clx_rs_rate> pairs;
    std::vector<float> coef;
};

inline uint32_t clx_rs_gcd(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }

// The reduced pair and W of fs -> R (both rates checked by the caller: 1 .. 2^20 - 1); W = 0 for fs == R.  Returns the entries of
// the pair's [n][2W] table.
inline uint64_t clx_resample_pair(uint32_t fs, uint32_t R, clx_rs_rate* p) {
    const uint32_t g = clx_rs_gcd(fs, R);
    p->o = fs / g; p->n = R / g; p->off = 0;
    if (fs == R) { p->W = 0; return 0; }
    const double base = (double)(p->o < p->n ? p->o : p->n) * 0.99;
    p->W = (uint32_t)ceil(6.0 * (double)p->o / base);
    return (uint64_t)p->n * 2u * p->W;
}

// The pair's table: p.n rows of clx_rs::row_stride(p.W) floats, computed in double and rounded once.
inline void clx_resample_table(const clx_rs_rate& p, float* tab) {
    const double pi = 3.14159265358979323846;
    const double base = (double)(p.o < p.n ? p.o : p.n) * 0.99, scale = base / (double)p.o;
    const uint32_t stride = clx_rs::row_stride(p.W);
    for (uint32_t i = 0; i < p.n; ++i) {
        const double frac = (double)(((uint64_t)i * p.o) % p.n) / (double)p.n;       // i * o / n - floor(i * o / n)
        for (uint32_t k = 0; k < stride; ++k) {
            double h = 0.0;
            if (k < 2u * p.W) {
                const double d = (double)((int64_t)k - (int64_t)p.W + 1) - frac, t = d * scale;
                if (fabs(t) < 6.0) {
                    const double c = cos(pi * t / 12.0);
                    h = (t == 0.0 ? 1.0 : sin(pi * t) / (pi * t)) * c * c * scale;
                }
            }
            tab[(size_t)i * stride + k] = (float)h;
        }
    }
}

// The host side of clx_resample_windows, first half: checks the arguments (nullptr: fine, else the text for clx_last_error) against
// the tables `cache` holds already, lists the call's distinct source rates in `call_fs` and gives the launch shape: *n_tiles tiles
// per window (0: nothing to launch), n_windows * *n_tiles blocks of clx_rs::kThreads.  Changes nothing.
inline const char* clx_resample_plan(const clx_rs_cache& cache, const void* src, const uint64_t* src_first, const int64_t* src_t0,
                                     const uint32_t* src_n, const uint64_t* out_t0, const uint32_t* valid, const uint32_t* src_rate,
                                     size_t n_windows, uint32_t out_rate, uint32_t window_len, uint32_t channels, uint32_t layout,
                                     const void* out, std::vector<uint32_t>* call_fs, uint32_t* n_tiles) {
    *n_tiles = 0;
    call_fs->clear();
    if (channels < 1u || channels > 8u) return "clx_resample_windows: channels must be 1..8";
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return "clx_resample_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT";
    if (out_rate == 0u || out_rate >= clx_rs::kRateLimit) return "clx_resample_windows: out_rate must be 1 .. 2^20 - 1";
    if (n_windows == 0 || window_len == 0) return nullptr;
    if (!src || !src_first || !src_t0 || !src_n || !out_t0 || !valid || !src_rate || !out) return "clx_resample_windows: null argument";
    uint64_t coef = cache.coef.size();
    for (size_t k = 0; k < n_windows; ++k) {
        if (valid[k] > window_len) return "clx_resample_windows: valid[k] is larger than window_len";
        if (src_rate[k] == 0u || src_rate[k] >= clx_rs::kRateLimit) return "clx_resample_windows: src_rate[k] must be 1 .. 2^20 - 1";
        if (out_t0[k] >= clx_rs::kMaxOut - window_len) return "clx_resample_windows: out_t0[k] is too large";
        const uint32_t fs = src_rate[k];
        if (fs == out_rate || (!call_fs->empty() && call_fs->back() == fs)) continue;
        bool seen = false;
        for (uint32_t f : *call_fs) seen |= f == fs;
        if (seen) continue;
        clx_rs_rate p;
        if (clx_resample_pair(fs, out_rate, &p) > clx_rs::kMaxEntries)
            return "clx_resample_windows: the coefficient table of a rate pair would have more than 2^18 entries";
        bool cached = false;
        for (const clx_rs_rate& q : cache.pairs) cached |= q.o == p.o && q.n == p.n;
        if (!cached) coef += (uint64_t)p.n * clx_rs::row_stride(p.W);
        if (coef > clx_rs::kMaxCoef) return "clx_resample_windows: the coefficient tables of this context would exceed 2^30 floats";
        call_fs->push_back(fs);
    }
    const uint64_t tiles = ((uint64_t)window_len + clx_rs::kTile - 1u) / clx_rs::kTile;
    if (tiles * (uint64_t)n_windows > 0x7fffffffull) return "clx_resample_windows: too many windows in one call";
    *n_tiles = (uint32_t)tiles;
    return nullptr;
}

// Second half: the job table (n_windows entries) and the call's rate table (1 + call_fs.size() entries: the copy entry, then a pair
// per source rate of `call_fs`), after clx_resample_plan has passed.  A pair the cache lacks is built and appended to it.
inline void clx_resample_fill(clx_rs_cache* cache, clx_rs_job* jobs, clx_rs_rate* rates, const std::vector<uint32_t>& call_fs,
                              const uint64_t* src_first, const int64_t* src_t0, const uint32_t* src_n, const uint64_t* out_t0,
                              const uint32_t* valid, const uint32_t* src_rate, size_t n_windows, uint32_t out_rate) {
    rates[0] = clx_rs_rate{1u, 1u, 0u, 0u};
    for (size_t r = 0; r < call_fs.size(); ++r) {
        clx_rs_rate p;
        clx_resample_pair(call_fs[r], out_rate, &p);
        const clx_rs_rate* hit = nullptr;
        for (const clx_rs_rate& q : cache->pairs)
            if (q.o == p.o && q.n == p.n) hit = &q;
        if (!hit) {
            p.off = (uint32_t)cache->coef.size();
            cache->coef.resize(cache->coef.size() + (size_t)p.n * clx_rs::row_stride(p.W));
            clx_resample_table(p, cache->coef.data() + p.off);
            cache->pairs.push_back(p);
            hit = &cache->pairs.back();
        }
        rates[1 + r] = *hit;
    }
    uint32_t last = 0;
    for (size_t k = 0; k < n_windows; ++k) {
        uint32_t r = 0;
        if (src_rate[k] != out_rate) {
            if (last && call_fs[last - 1] == src_rate[k]) r = last;
            else for (size_t i = 0; i < call_fs.size(); ++i) if (call_fs[i] == src_rate[k]) r = (uint32_t)i + 1u;
            last = r;
        }
        jobs[k] = clx_rs_job{src_first[k], src_t0[k], out_t0[k], src_n[k], valid[k], r, 0u};
    }
}
