// TEST INFRASTRUCTURE: SpecAugment (claxon_amd/csrc/clx_specaug.hip, unmodified, behind clx_norm.hip whose sum kernels it uses)
// under the wave simulator: clx_specaug_check, the per-call table, then the sum, fill and apply kernels launched as
// clx_specaug_windows launches them (clx_api.hip), with host buffers in place of device ones.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "clx_norm.hip"
#include "clx_specaug.hip"

static char sim_specaug_err[256];

extern "C" const char* sim_specaug_error(void) { return sim_specaug_err; }
extern "C" uint32_t sim_specaug_tile(void) { return clx_specaug::kTile; }
extern "C" uint32_t sim_specaug_threads(void) { return clx_specaug::kThreads; }
extern "C" uint32_t sim_specaug_max_rows(void) { return clx_specaug::kMaxRows; }
extern "C" uint32_t sim_specaug_max_masks(void) { return clx_specaug::kMaxMasks; }
extern "C" uint32_t sim_specaug_max_t(void) { return clx_specaug::kMaxT; }
extern "C" uint32_t sim_specaug_lds_bytes(void) { return clx_specaug::kLdsBytes; }

// clx_specaug_windows with `in`, `out` and `fills` in host memory: CLX_OK, or CLX_API_ERROR with sim_specaug_error() saying why.
// has_opts == 0: opts == NULL.
extern "C" int sim_specaug_windows(const void* in, void* out, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                   const uint32_t* warp, const uint32_t* fmasks, const uint32_t* tmasks, int has_opts, uint32_t F, uint32_t M,
                                   uint32_t fill_mean, float fill, uint32_t reserved, void* fills) {
    clx_specaug_opts o;
    o.n_freq_masks = F; o.n_time_masks = M; o.fill_mean = fill_mean; o.fill = fill; o.reserved = reserved;
    clx_specaug_plan pl;
    const char* why = clx_specaug_check(in, out, n_windows, rows, T, valid, layout, warp, fmasks, tmasks, has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_specaug_err, sizeof sim_specaug_err, "%s", why); return CLX_API_ERROR; }
    if (pl.n_tiles == 0) return CLX_OK;
    const uint32_t Fq = fmasks ? F : 0u, Mq = tmasks ? M : 0u;
    // (the fills behind the table and the partial sums start as NaNs: one that is read before it is written shows)
    std::vector<uint32_t> tab((size_t)pl.table_words + n_windows, 0x7fc00001u);
    clx_specaug_fill_table(tab.data(), n_windows, rows, valid, warp, fmasks, Fq, tmasks, Mq);
    std::vector<double> part((size_t)pl.partials, std::nan(""));
    if (pl.mean) {
        const float* x = (const float*)in;
        if (pl.tc)
            SIM_LAUNCH(clx_k_norm_sum_tc, pl.sum_blocks, clx_norm::kThreads, x, (const uint32_t*)tab.data(), part.data(), rows, T, pl.n_chunks, pl.n_groups);
        else
            SIM_LAUNCH(clx_k_norm_sum, pl.sum_blocks, clx_norm::kThreads, x, (const uint32_t*)tab.data(), part.data(), rows, T, pl.n_chunks,
                       (uint64_t)n_windows * rows * pl.n_chunks);
        SIM_LAUNCH(clx_k_specaug_fill, pl.fill_blocks, clx_specaug::kThreads, (const uint32_t*)tab.data(), (const double*)part.data(),
                   (float*)(tab.data() + pl.table_words), (uint32_t)n_windows, rows, pl.n_chunks);
    }
    SIM_LAUNCH(clx_k_specaug, n_windows * pl.n_tiles, clx_specaug::kThreads, (const uint32_t*)in, (uint32_t*)out, (const uint32_t*)tab.data(),
               (float*)fills, (uint32_t)n_windows, rows, T, Fq, Mq, pl.mean, o.fill_mean ? 0.f : o.fill, pl.tc, pl.n_tiles);
    return CLX_OK;
}
