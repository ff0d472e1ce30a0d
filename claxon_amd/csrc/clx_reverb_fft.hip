// clx_reverb_fft.hip -- clx_reverb_windows_fft: the windows convolved with their responses by uniformly partitioned overlap-save.
// claxon_hip.h has the definition; this is how it is computed.  It stands behind clx_reverb.hip in clx_api.hip: the
// argument checks, the per-call table, the power sums, the gain and the scale of keep_power are clx_reverb_windows' own.
//
// Hop kHop = H = 1024, transform length kN = N = 2 H = 2048, kBins = N / 2 + 1 = 1025 kept bins a spectrum.  Two kernels of this
// method's own, then clx_reverb_windows' sum, gain and scale launches unchanged:
//   fwd     clx_k_rvfft_fwd     one workgroup a transform: the live segments of every (window, row) with a response, then the call's
//                               partitions.  The N real words go into LDS as (word, +0.0f) in bit-reversed order, the eleven radix-2
//                               stages run there, bins 0 .. N / 2 leave for the workspace: a spectrum is a line of kSpec = 1040
//                               complex words (8320 bytes, 65 lines of 128), read whole by the next kernel.  With TC the stride-`rows`
//                               loads happen here, once per word.
//   mac     clx_k_rvfft_mac     one workgroup an (window, row, block of H outputs): a lane holds bins tid, tid + 256, .. and walks
//                               the delay line, p ascending: acc = X[b - p] * Hp[p], the p = 0 product first.  The sums go into LDS
//                               with their mirror (bin N - k is the conjugate of bin k), the inverse stages run, and the real parts of
//                               the last H words, times 1 / N, leave: contiguous bytes for CT, stride `rows` for TC.  A block behind
//                               valid[k] writes zeros, a window without a response its copy.
// A lane runs four butterflies a stage; a stage ends in one barrier.  LDS: N complex words = 16 384 bytes; at most 64 vector
// registers: eight workgroups of four waves, one wave a SIMD each, share a CU's 160 KiB (eight waves a SIMD).
//
// Which taps a window reads.  Window k reads h[0 .. Lv), Lv = min(L, V).  Its partitions p < floor(Lv / H) are whole: they are the
// response's, transformed once for every window that names it (slot base_j + p).  A last partition of Lv % H taps is keyed by
// (j, Lv): windows with the same response and the same Lv share it, and a window cut short has one of its own.  So a window's words
// do not know which other windows name its response.
//
// clx_rvfft_check, clx_rvfft_plan_call, clx_rvfft_fill and clx_rvfft_twiddles are the host side (plain C++, shared with the wave
// simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/claxon_hip.h"

namespace clx_rvfft {

constexpr uint32_t kThreads = 256u, kLog = 11u, kN = 1u << kLog, kHop = kN / 2u, kBins = kN / 2u + 1u, kSpec = 1040u;
constexpr uint32_t kLdsBytes = kN * 8u;                          // 16 384
constexpr uint32_t kJobBytes = 12u;                              // a partition job: row of d_ir, first tap, live taps
constexpr uint32_t kWinBytes = clx_reverb::kTableBytesDevice + 8u;   // a window's share of the per-call table: clx_reverb's, the gain, base and last
static_assert(kSpec >= kBins && (kSpec * 8u) % 128u == 0u, "a spectrum is whole lines");
static_assert(kN / 2u == 4u * kThreads, "four butterflies a lane and stage");

struct __attribute__((aligned(8))) cf { float x, y; };           // a complex word

using clx_add::fma_rn;
using clx_reverb::mul_rn;
using clx_norm::add_rn;
using clx_norm::sub_rn;

// bits 0..10 of n, reversed
__host__ __device__ __forceinline__ uint32_t rev(uint32_t n) {
    n = ((n & 0x5555u) << 1) | ((n >> 1) & 0x5555u);
    n = ((n & 0x3333u) << 2) | ((n >> 2) & 0x3333u);
    n = ((n & 0x0f0fu) << 4) | ((n >> 4) & 0x0f0fu);
    n = ((n & 0x00ffu) << 8) | ((n >> 8) & 0x00ffu);
    return n >> (16u - kLog);
}

// The eleven stages over a[] (its words in bit-reversed order), decimation in time: stage s = 1 .. 11 has half = 2^(s - 1); the
// butterfly i = 0 .. N / 2 - 1 of a stage has k = i % half, lo = 2 (i - k) + k, hi = lo + half, w = tw[k * (N / 2) / half] (kInv:
// its conjugate), t = w * a[hi] as t.x = fmaf(w.x, v.x, -fl(w.y * v.y)), t.y = fmaf(w.x, v.y, fl(w.y * v.x)), and then
// a[lo] = u + t, a[hi] = u - t, every addition rounded once.  Called by the whole block; ends behind a barrier.
template <bool kInv>
__device__ __forceinline__ void stages(cf* a, const cf* __restrict__ tw, uint32_t tid) {
    for (uint32_t s = 1; s <= kLog; ++s) {
        const uint32_t half = 1u << (s - 1u);
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            const uint32_t i = tid + q * kThreads, k = i & (half - 1u), lo = ((i - k) << 1) + k, hi = lo + half;
            cf w = tw[k << (kLog - s)];
            if (kInv) w.y = -w.y;
            const cf u = a[lo], v = a[hi];
            const float tx = fma_rn(w.x, v.x, -mul_rn(w.y, v.y)), ty = fma_rn(w.x, v.y, mul_rn(w.y, v.x));
            a[lo] = cf{ add_rn(u.x, tx), add_rn(u.y, ty) };
            a[hi] = cf{ sub_rn(u.x, tx), sub_rn(u.y, ty) };
        }
    }
    __syncthreads();
}

// the per-call table of n windows behind clx_reverb's and the gains: base (the slot of partition 0 of the window's response) and
// last (the slot of its last, ragged partition; unused where Lv % H == 0), then the partition jobs
struct table { const uint32_t* base; const uint32_t* last; const uint32_t* jobs; };
__host__ __device__ __forceinline__ table table_of(const void* tab, size_t n) {
    table t;
    t.base = (const uint32_t*)((const char*)tab + n * clx_reverb::kTableBytesDevice);
    t.last = t.base + n;
    t.jobs = t.last + n;
    return t;
}

}  // namespace clx_rvfft

// the launch shape clx_rvfft_plan_call gives
struct clx_rvfft_plan {
    uint32_t nb = 0;             // blocks of H outputs in a row: ceil(T / H)
    uint64_t n_seg = 0;          // segment slots: n_windows * rows * nb
    std::vector<uint32_t> jobs;  // the partition jobs: (row of d_ir, first tap, live taps) each
    std::vector<uint32_t> base, last;    // per window
    uint64_t slots() const { return n_seg + jobs.size() / 3u; }
    size_t table_bytes(size_t n) const { return n * clx_rvfft::kWinBytes + jobs.size() * 4u; }
};

// The forward transforms.  Block b < n_seg: segment b % nb of row (b / nb) % rows of window b / (nb * rows) -- the samples
// (s - 1) H .. (s + 1) H - 1 of the row, those before the crop and at or behind valid[k] as +0.0f --, into slot b; it returns where
// the window has no response or the segment starts at or behind valid[k].  Block n_seg + q: partition job q, into slot n_seg + q.
extern "C" __global__ __launch_bounds__(256) void clx_k_rvfft_fwd(const float* __restrict__ x, const float* __restrict__ ir, const void* __restrict__ tab,
                                                                  const clx_rvfft::cf* __restrict__ tw, clx_rvfft::cf* __restrict__ ws, uint32_t n_windows,
                                                                  uint32_t rows, uint32_t T, uint32_t K, uint32_t tc, uint32_t nb, uint32_t n_seg) {
    using namespace clx_rvfft;
    __shared__ __attribute__((aligned(16))) cf A[kN];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < n_seg) {
        const uint32_t s = blockIdx.x % nb, kr = blockIdx.x / nb, k = kr / rows, r = kr - k * rows;
        const clx_reverb::table tb = clx_reverb::table_of(tab, n_windows);
        const uint32_t v = tb.a.vs[k];
        if (tb.len[k] == 0u || (uint64_t)s * kHop >= v) return;              // (the whole block)
        const uint64_t stride = tc ? rows : 1u;
        const float* const xr = x + (tc ? (uint64_t)k * rows * T + r : ((uint64_t)k * rows + r) * T);
        const int64_t t0 = ((int64_t)s - 1) * (int64_t)kHop;
#pragma unroll
        for (uint32_t i = 0; i < kN / kThreads; ++i) {
            const uint32_t n = tid + i * kThreads;
            const int64_t t = t0 + n;
            A[rev(n)] = cf{ t >= 0 && t < (int64_t)v ? xr[(uint64_t)t * stride] : 0.f, 0.f };
        }
    } else {
        const uint32_t* const job = table_of(tab, n_windows).jobs + (uint64_t)(blockIdx.x - n_seg) * 3u;
        const float* const h = ir + (uint64_t)job[0] * K + job[1];
        const uint32_t cnt = job[2];
#pragma unroll
        for (uint32_t i = 0; i < kN / kThreads; ++i) {
            const uint32_t n = tid + i * kThreads;
            A[rev(n)] = cf{ n < cnt ? h[n] : 0.f, 0.f };
        }
    }
    stages<false>(A, tw, tid);
    cf* const out = ws + (uint64_t)blockIdx.x * kSpec;
    for (uint32_t n = tid; n < kBins; n += kThreads) out[n] = A[n];
}

// The delay line and the inverse transform.  Block b: output block b % nb of row (b / nb) % rows of window b / (nb * rows).
extern "C" __global__ __launch_bounds__(256) void clx_k_rvfft_mac(const float* __restrict__ x, const void* __restrict__ tab, const clx_rvfft::cf* __restrict__ tw,
                                                                  const clx_rvfft::cf* __restrict__ ws, float* __restrict__ out, uint32_t n_windows,
                                                                  uint32_t rows, uint32_t T, uint32_t tc, uint32_t nb, uint32_t n_seg) {
    using namespace clx_rvfft;
    __shared__ __attribute__((aligned(16))) cf A[kN];
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x % nb, kr = blockIdx.x / nb, k = kr / rows, r = kr - k * rows;
    const clx_reverb::table tb = clx_reverb::table_of(tab, n_windows);
    const uint32_t v = tb.a.vs[k], len = tb.len[k];
    const uint64_t stride = tc ? rows : 1u;
    const uint64_t rowbase = tc ? (uint64_t)k * rows * T + r : ((uint64_t)k * rows + r) * T;
    float* const yr = out + rowbase;
    const uint64_t t0 = (uint64_t)b * kHop;
    if (len == 0u || t0 >= v) {                                // (the whole block) no response: a copy; behind the live part: zeros
        const float* const xr = x + rowbase;
#pragma unroll
        for (uint32_t i = 0; i < kHop / kThreads; ++i) {
            const uint64_t t = t0 + tid + i * kThreads;
            if (t < T) yr[t * stride] = t < v ? xr[t * stride] : 0.f;
        }
        return;
    }
    const table ft = table_of(tab, n_windows);
    const uint32_t lv = len < v ? len : v, full = lv / kHop, np = (lv + kHop - 1u) / kHop;   // the window's live taps, whole partitions, partitions
    const uint32_t pe = b + 1u < np ? b + 1u : np;             // p < pe: segment b - p exists
    const cf* const seg = ws + (uint64_t)blockIdx.x * kSpec;   // segment b's spectrum; segment b - p lies p slots before it
    const uint64_t hbase = (uint64_t)n_seg + ft.base[k], hlast = (uint64_t)n_seg + ft.last[k];
    cf acc[5];
#pragma unroll
    for (uint32_t i = 0; i < 5u; ++i) acc[i] = cf{ 0.f, 0.f };
    for (uint32_t p = 0; p < pe; ++p) {
        const cf* const X = seg - (uint64_t)p * kSpec;
        const cf* const Hp = ws + (p < full ? hbase + p : hlast) * kSpec;
#pragma unroll
        for (uint32_t i = 0; i < 5u; ++i) {
            const uint32_t n = tid + i * kThreads;
            if (n >= kBins) break;
            const cf a = X[n], h = Hp[n];
            if (p == 0u) {
                acc[i].x = fma_rn(a.x, h.x, -mul_rn(a.y, h.y));
                acc[i].y = fma_rn(a.x, h.y, mul_rn(a.y, h.x));
            } else {
                acc[i].x = fma_rn(-a.y, h.y, fma_rn(a.x, h.x, acc[i].x));
                acc[i].y = fma_rn(a.y, h.x, fma_rn(a.x, h.y, acc[i].y));
            }
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < 5u; ++i) {
        const uint32_t n = tid + i * kThreads;
        if (n >= kBins) break;
        A[rev(n)] = acc[i];
        if (n != 0u && n != kN / 2u) A[rev(kN - n)] = cf{ acc[i].x, -acc[i].y };
    }
    stages<true>(A, tw, tid);
#pragma unroll
    for (uint32_t i = 0; i < kHop / kThreads; ++i) {
        const uint32_t n = tid + i * kThreads;
        const uint64_t t = t0 + n;
        if (t < T) yr[t * stride] = t < v ? mul_rn(A[kHop + n].x, 1.f / (float)kN) : 0.f;
    }
}

// The twiddles: tw[q] = (fl32(cos(2 pi q / N)), fl32(-sin(2 pi q / N))), q = 0 .. N / 2 - 1, the cosine and the sine taken in
// double and rounded once.
inline void clx_rvfft_twiddles(clx_rvfft::cf* tw) {
    for (uint32_t q = 0; q < clx_rvfft::kN / 2u; ++q) {
        const double a = 2.0 * 3.14159265358979323846 * (double)q / (double)clx_rvfft::kN;
        tw[q].x = (float)cos(a);
        tw[q].y = (float)-sin(a);
    }
}

// The host side of clx_reverb_windows_fft: the arguments checked as clx_reverb_windows checks them, under this call's name ("":
// fine, else the text for clx_last_error), and clx_reverb_windows' launch shape.
inline std::string clx_rvfft_check(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const void* ir, size_t n_ir,
                                   uint32_t K, const uint32_t* ir_len, const int32_t* ir_index, uint32_t layout, const clx_reverb_fft_opts* o,
                                   const void* out, clx_reverb_plan* p) {
    *p = clx_reverb_plan();
    if (o && (o->keep_power > 1u || o->reserved[0] != 0u || o->reserved[1] != 0u || o->reserved[2] != 0u))
        return "clx_reverb_windows_fft: opts->keep_power must be 0 or 1 and opts->reserved 0";
    clx_reverb_opts ro;
    ro.keep_power = o ? o->keep_power : 0u; ro.reserved = 0u;
    const char* why = clx_reverb_check(data, n_windows, rows, T, valid, ir, n_ir, K, ir_len, ir_index, layout, &ro, out, p);
    if (!why) return std::string();
    const char* colon = strchr(why, ':');                      // (clx_reverb_windows' text under this call's name)
    return std::string("clx_reverb_windows_fft") + (colon ? colon : why);
}

// The transforms of a checked call: the segment slots, the partition jobs and every window's base and last ("": fine).
inline std::string clx_rvfft_plan_call(size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const uint32_t* ir_len, const int32_t* ir_index,
                                       size_t n_ir, clx_rvfft_plan* f) {
    using namespace clx_rvfft;
    *f = clx_rvfft_plan();
    f->nb = (uint32_t)(((uint64_t)T + kHop - 1u) / kHop);
    f->n_seg = (uint64_t)n_windows * rows * f->nb;
    f->base.assign(n_windows, 0u); f->last.assign(n_windows, 0u);
    std::vector<uint32_t> whole(n_ir, 0u);                     // per response: the whole partitions some window reads
    for (size_t k = 0; k < n_windows; ++k) {
        const int32_t j = ir_index[k];
        if (j < 0) continue;
        const uint32_t lv = ir_len[j] < valid[k] ? ir_len[j] : valid[k];
        if (lv / kHop > whole[j]) whole[j] = lv / kHop;
    }
    std::vector<uint32_t> first(n_ir, 0u);
    for (size_t j = 0; j < n_ir; ++j) {
        first[j] = (uint32_t)(f->jobs.size() / 3u);
        for (uint32_t p = 0; p < whole[j]; ++p) { f->jobs.push_back((uint32_t)j); f->jobs.push_back(p * kHop); f->jobs.push_back(kHop); }
    }
    std::unordered_map<uint64_t, uint32_t> ragged;             // (response, live taps) -> slot
    for (size_t k = 0; k < n_windows; ++k) {
        const int32_t j = ir_index[k];
        if (j < 0) continue;
        const uint32_t lv = ir_len[j] < valid[k] ? ir_len[j] : valid[k];
        f->base[k] = first[j];
        if (lv % kHop == 0u) continue;
        const uint64_t key = (uint64_t)(uint32_t)j << 32 | lv;
        auto it = ragged.find(key);
        if (it == ragged.end()) {
            it = ragged.emplace(key, (uint32_t)(f->jobs.size() / 3u)).first;
            f->jobs.push_back((uint32_t)j); f->jobs.push_back(lv / kHop * kHop); f->jobs.push_back(lv % kHop);
        }
        f->last[k] = it->second;
    }
    if (f->slots() > 0x7fffffffull) return "clx_reverb_windows_fft: too many windows in one call";
    return std::string();
}

// The per-call table into `tab` (8-byte aligned, f->table_bytes(n_windows) bytes): clx_reverb's, room for the gains, base, last,
// the jobs.
inline void clx_rvfft_fill(void* tab, size_t n_windows, const uint32_t* valid, const uint32_t* ir_len, const int32_t* ir_index, uint32_t keep_power,
                           const clx_rvfft_plan* f) {
    clx_reverb_fill(tab, n_windows, valid, ir_len, ir_index, keep_power);
    uint32_t* const base = (uint32_t*)((char*)tab + n_windows * clx_reverb::kTableBytesDevice);
    memset((char*)tab + n_windows * clx_reverb::kTableBytes, 0, n_windows * (clx_reverb::kTableBytesDevice - clx_reverb::kTableBytes));
    if (n_windows) {
        memcpy(base, f->base.data(), n_windows * 4u);
        memcpy(base + n_windows, f->last.data(), n_windows * 4u);
    }
    if (!f->jobs.empty()) memcpy(base + 2u * n_windows, f->jobs.data(), f->jobs.size() * 4u);
}
