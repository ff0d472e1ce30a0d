// TEST INFRASTRUCTURE: the channel-mixing window reader (claxon_amd/csrc/clx_mix.hip, unmodified) under the wave simulator:
// clx_mix_plan and clx_mix_fill, then clx_k_mix launched as clx_mix_windows launches it (clx_api.hip), with host buffers in place of
// device ones and a coefficient cache that lives as long as the library (a context's does).  clx_resample_windows is here too, on the
// same cache, as it is on a context: what an identity must equal, and a pair built by either call serves both.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <sys/mman.h>
#include <unistd.h>
#include <hip/hip_runtime.h>

#include "clx_mix.hip"

static char sim_mix_err[256];
static clx_rs_cache sim_cache;

extern "C" const char* sim_mix_error(void) { return sim_mix_err; }

// the rate pairs the cache holds, and the floats of their tables
extern "C" size_t sim_mix_cached_pairs(void) { return sim_cache.pairs.size(); }
extern "C" size_t sim_mix_cached_floats(void) { return sim_cache.coef.size(); }

// clx_mix_windows with `src` and `out` in host memory: CLX_OK, or CLX_API_ERROR with sim_mix_error() saying why
extern "C" int sim_mix_windows(const void* src, const uint64_t* src_first, const int64_t* src_t0, const uint32_t* src_n, const uint64_t* out_t0,
                               const uint32_t* valid, const uint32_t* src_rate, const uint8_t* src_channels, size_t n_windows, uint32_t out_rate,
                               uint32_t window_len, uint32_t out_channels, uint32_t layout, void* out) {
    uint32_t n_tiles = 0;
    std::vector<uint32_t> call_fs;
    const std::string why = clx_mix_plan(sim_cache, src, src_first, src_t0, src_n, out_t0, valid, src_rate, src_channels, n_windows, out_rate,
                                         window_len, out_channels, layout, out, &call_fs, &n_tiles);
    if (!why.empty()) { snprintf(sim_mix_err, sizeof sim_mix_err, "%s", why.c_str()); return CLX_API_ERROR; }
    if (n_tiles == 0) return CLX_OK;
    std::vector<clx_rs_job> jobs(n_windows);
    std::vector<clx_rs_rate> rates(1 + call_fs.size());
    clx_mix_fill(&sim_cache, jobs.data(), rates.data(), call_fs, src_first, src_t0, src_n, out_t0, valid, src_rate, src_channels, n_windows, out_rate);
    SIM_LAUNCH(clx_k_mix, n_windows * n_tiles, clx_rs::kThreads, (const float*)src, (const clx_rs_job*)jobs.data(), (const clx_rs_rate*)rates.data(),
               (const float*)sim_cache.coef.data(), n_tiles, window_len, out_channels, layout, (float*)out);
    return CLX_OK;
}

// clx_resample_windows on the same cache (tests/wavesim/sim_resample.cpp's, restated: that library has a cache of its own)
extern "C" int sim_mix_resample_windows(const void* src, const uint64_t* src_first, const int64_t* src_t0, const uint32_t* src_n,
                                        const uint64_t* out_t0, const uint32_t* valid, const uint32_t* src_rate, size_t n_windows, uint32_t out_rate,
                                        uint32_t window_len, uint32_t channels, uint32_t layout, void* out) {
    uint32_t n_tiles = 0;
    std::vector<uint32_t> call_fs;
    const char* why = clx_resample_plan(sim_cache, src, src_first, src_t0, src_n, out_t0, valid, src_rate, n_windows, out_rate, window_len, channels,
                                        layout, out, &call_fs, &n_tiles);
    if (why) { snprintf(sim_mix_err, sizeof sim_mix_err, "%s", why); return CLX_API_ERROR; }
    if (n_tiles == 0) return CLX_OK;
    std::vector<clx_rs_job> jobs(n_windows);
    std::vector<clx_rs_rate> rates(1 + call_fs.size());
    clx_resample_fill(&sim_cache, jobs.data(), rates.data(), call_fs, src_first, src_t0, src_n, out_t0, valid, src_rate, n_windows, out_rate);
    SIM_LAUNCH(clx_k_resample, n_windows * n_tiles, clx_rs::kThreads, (const float*)src, (const clx_rs_job*)jobs.data(), (const clx_rs_rate*)rates.data(),
               (const float*)sim_cache.coef.data(), n_tiles, window_len, channels, layout, (float*)out);
    return CLX_OK;
}

// One window whose source span (src_n * src_channels floats, given in `floats`) sits flush against an inaccessible page: the page
// follows the span's last float (at_end), or precedes its first.  A load on the wrong side of either end faults instead of reading
// a neighbour's bytes.
extern "C" int sim_mix_guarded(const float* floats, int64_t src_t0, uint32_t src_n, uint64_t out_t0, uint32_t valid, uint32_t src_rate,
                               uint32_t src_channels, uint32_t out_rate, uint32_t window_len, uint32_t out_channels, uint32_t layout, int at_end,
                               void* out) {
    const size_t len = (size_t)src_n * src_channels * 4u;
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), body = (len + pg - 1) / pg * pg + pg;
    uint8_t* m = (uint8_t*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == (uint8_t*)MAP_FAILED) return -1;
    mprotect(m, pg, PROT_NONE);
    mprotect(m + pg + body, pg, PROT_NONE);
    uint8_t* p = at_end ? m + pg + body - len : m + pg;
    memcpy(p, floats, len);
    const uint64_t first = 0;
    const uint8_t cs = (uint8_t)src_channels;
    const int st = sim_mix_windows(p, &first, &src_t0, &src_n, &out_t0, &valid, &src_rate, &cs, 1, out_rate, window_len, out_channels, layout, out);
    munmap(m, body + 2 * pg);
    return st;
}
