// TEST INFRASTRUCTURE: the window gather (claxon_amd/csrc/clx_window.hip, unmodified) under the wave simulator: clx_window_check, then
// clx_k_window launched as clx_gather_windows launches it (clx_api.hip), with host buffers in place of device ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <sys/mman.h>
#include <unistd.h>
#include <hip/hip_runtime.h>

#include "clx_window.hip"

static char sim_window_err[256];

extern "C" const char* sim_window_error(void) { return sim_window_err; }

// clx_gather_windows with `src` and `out` in host memory: CLX_OK, or CLX_API_ERROR with sim_window_error() saying why
extern "C" int sim_gather_windows(const void* src, const uint64_t* src_first, const uint32_t* valid, size_t n_windows, uint32_t window_len,
                                  uint32_t channels, uint32_t layout, void* out) {
    uint32_t n_tiles = 0;
    const char* why = clx_window_check(src, src_first, valid, n_windows, window_len, channels, layout, out, &n_tiles);
    if (why) { snprintf(sim_window_err, sizeof sim_window_err, "%s", why); return CLX_API_ERROR; }
    if (n_tiles == 0) return CLX_OK;
    std::vector<clx_win_job> tab(n_windows);
    clx_window_fill(tab.data(), src_first, valid, n_windows);
    SIM_LAUNCH(clx_k_window, n_windows * n_tiles, clx_win::kThreads, (const uint32_t*)src, (const clx_win_job*)tab.data(), n_tiles, window_len, channels,
               layout, (uint32_t*)out);
    return CLX_OK;
}

// One window whose valid floats (valid * channels of them, given in `floats`) sit flush against an inaccessible page: the page
// follows the last of them (at_end), or precedes the first.  A load on the wrong side of either end faults instead of reading a
// neighbour's bytes.
extern "C" int sim_window_guarded(const uint32_t* floats, uint32_t valid, uint32_t window_len, uint32_t channels, uint32_t layout, int at_end,
                                  void* out) {
    const size_t len = (size_t)valid * channels * 4u;
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), body = (len + pg - 1) / pg * pg + pg;
    uint8_t* m = (uint8_t*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == (uint8_t*)MAP_FAILED) return -1;
    mprotect(m, pg, PROT_NONE);
    mprotect(m + pg + body, pg, PROT_NONE);
    uint8_t* p = at_end ? m + pg + body - len : m + pg;
    memcpy(p, floats, len);
    const uint64_t first = 0;
    const int st = sim_gather_windows(p, &first, &valid, 1, window_len, channels, layout, out);
    munmap(m, body + 2 * pg);
    return st;
}
