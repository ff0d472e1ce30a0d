// TEST INFRASTRUCTURE: the stream MD5 (claxon_amd/csrc/clx_md5.hip, unmodified) under the wave simulator: clx_md5_plan, then
// clx_k_md5 launched per width class as clx_md5_streams launches it (clx_api.hip), with host buffers in place of device ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <sys/mman.h>
#include <unistd.h>
#include <hip/hip_runtime.h>

static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

#include "clx_md5.hip"

static char sim_md5_err[256];

extern "C" const char* sim_md5_error(void) { return sim_md5_err; }

// clx_md5_streams with `samples` and `digests` in host memory: CLX_OK, or CLX_API_ERROR with sim_md5_error() saying why
extern "C" int sim_md5_streams(const void* samples, uint32_t fmt, const uint64_t* first, const uint64_t* n, const uint8_t* bps, size_t n_streams,
                               uint8_t* digests) {
    std::vector<clx_md5_job> jobs;
    size_t cls[5];
    const char* why = clx_md5_plan(samples, fmt, first, n, bps, n_streams, digests, jobs, cls);
    if (why) { snprintf(sim_md5_err, sizeof sim_md5_err, "%s", why); return CLX_API_ERROR; }
    std::vector<uint4> dig(n_streams ? n_streams : 1);
    for (uint32_t w = 1; w <= 4; ++w) {
        const size_t lo = cls[w - 1], cnt = cls[w] - lo;
        if (cnt) SIM_LAUNCH(clx_k_md5, (cnt + 63) / 64, 64, (const uint8_t*)samples, (const clx_md5_job*)(jobs.data() + lo), (uint32_t)cnt, fmt, w, dig.data());
    }
    if (n_streams) memcpy(digests, dig.data(), 16 * n_streams);
    return CLX_OK;
}

// One stream of `len` bytes hashed from a mapping where it sits flush against an inaccessible page: after it (at_end) or before it.
// A load past either end faults instead of reading a neighbour's bytes.
extern "C" int sim_md5_guarded(const uint8_t* bytes, size_t len, uint32_t fmt, uint64_t n, uint8_t bps, int at_end, uint8_t* digest) {
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), body = (len + pg - 1) / pg * pg;
    uint8_t* m = (uint8_t*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == (uint8_t*)MAP_FAILED) return -1;
    mprotect(m, pg, PROT_NONE);
    mprotect(m + pg + body, pg, PROT_NONE);
    uint8_t* p = at_end ? m + pg + body - len : m + pg;
    memcpy(p, bytes, len);
    const uint64_t first = 0;
    const int st = sim_md5_streams(p, fmt, &first, &n, &bps, 1, digest);
    munmap(m, body + 2 * pg);
    return st;
}
