// clx_mix.hip -- clx_resample.hip's dense batch of windows with every window brought to one channel count K while it is cut (and,
// where its rate differs from the target, resampled), in one launch.
//
// A window whose stream has Cs channels reaches K channels by one of three rules (anything else is refused on the host):
//   identity   Cs == K       what clx_k_window / clx_k_resample give, bit for bit: a word copy at the native rate, the same table and
//                            the same ascending fmaf chain under resampling;
//   reduce     K == 1 < Cs   the mean of the channels in float32: s = x[t][0]; s = s + x[t][1]; ... ; s = s + x[t][Cs-1], each add
//                            rounded to nearest, then s * r with r the float32 nearest to 1 / Cs;
//   replicate  Cs == 1 < K   the mono sample goes to each of the K channels.
// With a target rate the mix comes first: the fixed resampler of clx_resample.hip runs on the mixed float32 signal, taps ascending,
// one fmaf each with the mixed value as the multiplicand, so a reduce costs one filter per output sample, not Cs, and replicated
// channels are bitwise equal.  A tap outside the window's source span counts as zero and none of its Cs floats is loaded: no float
// outside [src_first, src_first + src_n * Cs) is read.
//
// A job is a clx_rs_job with Cs in `reserved`; the rate table and the coefficient tables are clx_resample.hip's own (a pair built by
// either entry point serves both).  The grid is (window, tile of clx_rs::kTile outputs) with clx_k_resample's arithmetic: one 64-bit
// divide per tile, 32-bit phases per lane, rate entry 0 meaning copy.  A block is one window, so its rule is uniform.  Lanes run
// along E-float output rows: E = K for an identity (clx_k_resample's element mapping), E = 1 for a reduce and for a replicate
// (lanes along output samples: the sum is computed once, a replicate stores it K times).  Direct global loads, no LDS, no scratch.
//
// The host side (plain C++, shared with the wave simulator): clx_mix_plan (clx_resample_plan and the channel rules) and clx_mix_fill.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "clx_resample.hip"

namespace clx_mix {

using clx_rs::kThreads;
using clx_rs::kTile;

__device__ __forceinline__ uint32_t bits(float v) { uint32_t w; memcpy(&w, &v, 4); return w; }

// The mixed value of the sample whose floats start at p: the float itself (N == 1: p points at the channel wanted), or the mean of
// its N channels in the order the header states (1.0f / N is folded when the template is instantiated: correctly rounded).
template <uint32_t N>
__device__ __forceinline__ float take(const float* p) {
    if (N == 1u) return p[0];
    float x[N];
    memcpy(x, p, 4u * N);
    float s = x[0];
#pragma unroll
    for (uint32_t i = 1; i < N; ++i) s = s + x[i];
    return s * (1.0f / (float)N);
}

// One tile of one window.  N = Cs for a reduce, 1 otherwise; `o` is the window's first word in the output.
template <uint32_t N>
__device__ __forceinline__ void tile(const float* __restrict__ s, const clx_rs_job& job, const clx_rs_rate& R, const float* __restrict__ coef,
                                     uint32_t t_lo, uint32_t nT, uint32_t L, uint32_t K, bool tc, uint32_t* __restrict__ o) {
    const uint32_t Cs = job.reserved;
    const uint32_t E = Cs == 1u ? 1u : K;                         // floats of an output sample that lanes compute (a reduce has K == 1)
    const uint32_t reps = Cs == 1u ? K : 1u;                      // ... and the times each is stored (a replicate: K)
    const uint32_t total = nT * E;
    const uint64_t m0 = job.out_t0 + t_lo;                        // the tile's first output
    const bool copy = R.W == 0u;

    // the one 64-bit divide: m0 * o = q0 * n + r0, and the tile's first phase (a copy: output m is source sample m)
    const uint64_t p0 = m0 * R.o, q0 = copy ? m0 : p0 / R.n;
    const uint32_t r0 = (uint32_t)(p0 - q0 * R.n), i0 = (uint32_t)(m0 % R.n);
    const int64_t d0 = (int64_t)q0 - (copy ? 0 : (int64_t)(R.W - 1u)) - job.src_t0;   // tap 0 of the tile's first output, counted from the span's start
    const int32_t taps = (int32_t)(2u * R.W);
    const uint32_t stride = clx_rs::row_stride(R.W);
    const float* const tab = coef + R.off;
    const uint32_t* const sw = reinterpret_cast<const uint32_t*>(s);
    for (uint32_t e = threadIdx.x; e < total; e += kThreads) {
        const uint32_t a = e / (tc ? E : nT), b = e - a * (tc ? E : nT);
        const uint32_t j = tc ? a : b, c = tc ? b : a;
        uint32_t v = 0u;
        if (t_lo + j < job.valid) {
            if (copy) {
                const int64_t rel = d0 + j;
                if (rel >= 0 && rel < (int64_t)job.src_n) v = N == 1u ? sw[(uint64_t)rel * Cs + c] : bits(take<N>(s + (uint64_t)rel * Cs));
            } else {
                float acc = 0.0f;
                const int64_t rel = d0 + (int64_t)((r0 + j * R.o) / R.n);       // tap 0 of this output, counted from the span's start
                const int64_t lo = -rel, hi = (int64_t)job.src_n - rel;         // taps lo <= k < hi lie in the span
                const int32_t klo = lo <= 0 ? 0 : lo >= taps ? taps : (int32_t)lo;
                const int32_t khi = hi <= 0 ? 0 : hi >= taps ? taps : (int32_t)hi;
                const float* const h = tab + (uint64_t)((i0 + j) % R.n) * stride;
                for (int32_t k4 = klo & ~3; k4 < khi; k4 += 4) {
                    float hv[4];
                    clx_rs::ld16f(hv, h + k4);
                    const int64_t at = (rel + k4) * (int64_t)Cs + c;            // the float of tap k4 (only looked at where the tap is in the span)
                    if (k4 >= klo && k4 + 4 <= khi) {
                        const float x0 = take<N>(s + at), x1 = take<N>(s + at + Cs), x2 = take<N>(s + at + 2 * (int64_t)Cs),
                                    x3 = take<N>(s + at + 3 * (int64_t)Cs);
                        acc = fmaf(x0, hv[0], acc);
                        acc = fmaf(x1, hv[1], acc);
                        acc = fmaf(x2, hv[2], acc);
                        acc = fmaf(x3, hv[3], acc);
                    } else {
#pragma unroll
                        for (int32_t i = 0; i < 4; ++i)
                            if (k4 + i >= klo && k4 + i < khi) acc = fmaf(take<N>(s + at + i * (int64_t)Cs), hv[i], acc);
                    }
                }
                v = bits(acc);
            }
        }
        for (uint32_t r = 0; r < reps; ++r) o[tc ? (uint64_t)(t_lo + j) * K + c + r : (uint64_t)(c + r) * L + t_lo + j] = v;
    }
}

}  // namespace clx_mix

// Block b: tile b % n_tiles of window b / n_tiles (clx_mix_plan gives n_tiles).  `out` is the dense [B, L, K] / [B, K, L] batch.
extern "C" __global__ __launch_bounds__(256) void clx_k_mix(const float* __restrict__ src, const clx_rs_job* __restrict__ jobs,
                                                 const clx_rs_rate* __restrict__ rates, const float* __restrict__ coef, uint32_t n_tiles,
                                                 uint32_t L, uint32_t K, uint32_t layout, float* __restrict__ out) {
    using namespace clx_mix;
    const uint32_t w = blockIdx.x / n_tiles, tl = blockIdx.x - w * n_tiles;
    const clx_rs_job job = jobs[w];
    const clx_rs_rate R = rates[job.rate];
    const uint32_t t_lo = tl * kTile, nT = L - t_lo < kTile ? L - t_lo : kTile;
    const float* const s = src + job.src_first;
    uint32_t* const o = reinterpret_cast<uint32_t*>(out) + (uint64_t)w * L * K;
    const bool tc = layout == CLX_WINDOW_TC;
    switch (K == 1u ? job.reserved : 1u) {                        // (the channels one output float is the mean of)
    case 1: tile<1>(s, job, R, coef, t_lo, nT, L, K, tc, o); return;
    case 2: tile<2>(s, job, R, coef, t_lo, nT, L, K, tc, o); return;
    case 3: tile<3>(s, job, R, coef, t_lo, nT, L, K, tc, o); return;
    case 4: tile<4>(s, job, R, coef, t_lo, nT, L, K, tc, o); return;
    case 5: tile<5>(s, job, R, coef, t_lo, nT, L, K, tc, o); return;
    case 6: tile<6>(s, job, R, coef, t_lo, nT, L, K, tc, o); return;
    case 7: tile<7>(s, job, R, coef, t_lo, nT, L, K, tc, o); return;
    default: tile<8>(s, job, R, coef, t_lo, nT, L, K, tc, o); return;
    }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------

// The host side of clx_mix_windows, first half: clx_resample_plan's checks and launch shape with out_channels as the channel count
// (its texts under this call's name), then the channel rules.  Empty: fine, else the text for clx_last_error.  Changes nothing.
inline std::string clx_mix_plan(const clx_rs_cache& cache, const void* src, const uint64_t* src_first, const int64_t* src_t0,
                                const uint32_t* src_n, const uint64_t* out_t0, const uint32_t* valid, const uint32_t* src_rate,
                                const uint8_t* src_channels, size_t n_windows, uint32_t out_rate, uint32_t window_len, uint32_t out_channels,
                                uint32_t layout, const void* out, std::vector<uint32_t>* call_fs, uint32_t* n_tiles) {
    *n_tiles = 0;
    if (out_channels < 1u || out_channels > 8u) return "clx_mix_windows: out_channels must be 1..8";
    const char* why = clx_resample_plan(cache, src, src_first, src_t0, src_n, out_t0, valid, src_rate, n_windows, out_rate, window_len,
                                        out_channels, layout, out, call_fs, n_tiles);
    if (why) {
        const char* colon = strchr(why, ':');
        return std::string("clx_mix_windows") + (colon ? colon : why);
    }
    if (*n_tiles == 0) return std::string();
    const uint32_t tiles = *n_tiles;
    *n_tiles = 0;
    if (!src_channels) return "clx_mix_windows: null argument";
    for (size_t k = 0; k < n_windows; ++k) {
        const uint32_t Cs = src_channels[k];
        if (Cs < 1u || Cs > 8u) return "clx_mix_windows: src_channels[k] must be 1..8";
        if (Cs != out_channels && Cs != 1u && out_channels != 1u)
            return "clx_mix_windows: no rule brings " + std::to_string(Cs) + " channels to " + std::to_string(out_channels) + " (window " +
                   std::to_string(k) + "): equal counts, any count to 1 and 1 to any count are the rules";
    }
    *n_tiles = tiles;
    return std::string();
}

// Second half: clx_resample_fill's tables, each job with its window's channel count.
inline void clx_mix_fill(clx_rs_cache* cache, clx_rs_job* jobs, clx_rs_rate* rates, const std::vector<uint32_t>& call_fs,
                         const uint64_t* src_first, const int64_t* src_t0, const uint32_t* src_n, const uint64_t* out_t0,
                         const uint32_t* valid, const uint32_t* src_rate, const uint8_t* src_channels, size_t n_windows, uint32_t out_rate) {
    clx_resample_fill(cache, jobs, rates, call_fs, src_first, src_t0, src_n, out_t0, valid, src_rate, n_windows, out_rate);
    for (size_t k = 0; k < n_windows; ++k) jobs[k].reserved = src_channels[k];
}
