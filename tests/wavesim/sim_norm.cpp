// TEST INFRASTRUCTURE: the per-window normalisation (claxon_amd/csrc/clx_norm.hip, unmodified) under the wave simulator:
// clx_norm_check, then the sum, square and apply kernels launched as clx_norm_windows launches them (clx_api.hip), with host
// buffers in place of device ones.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "clx_norm.hip"

static char sim_norm_err[256];

extern "C" const char* sim_norm_error(void) { return sim_norm_err; }
extern "C" uint32_t sim_norm_chunk(void) { return clx_norm::kChunk; }
extern "C" uint32_t sim_norm_strands(void) { return clx_norm::kStrands; }
extern "C" uint32_t sim_norm_max_rows(void) { return clx_norm::kMaxRows; }
extern "C" uint32_t sim_norm_tc_lds_bytes(void) { return clx_norm::kTcLdsBytes; }
extern "C" uint32_t sim_norm_apply_lds_bytes(void) { return clx_norm::kApplyLdsBytes; }

// clx_norm_windows with `data` and `stats` in host memory: CLX_OK, or CLX_API_ERROR with sim_norm_error() saying why.  has_opts == 0:
// opts == NULL.
extern "C" int sim_norm_windows(void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout, int has_opts,
                                uint32_t mean, uint32_t var, uint32_t ddof, float eps, float pad, void* stats) {
    clx_norm_opts o;
    o.mean = mean; o.var = var; o.ddof = ddof; o.eps = eps; o.pad = pad;
    clx_norm_plan pl;
    const char* why = clx_norm_check(data, n_windows, rows, T, valid, layout, has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_norm_err, sizeof sim_norm_err, "%s", why); return CLX_API_ERROR; }
    if (pl.n_chunks == 0) return CLX_OK;
    // (the table starts as NaNs: a partial that is read before it is written shows)
    std::vector<double> part((size_t)pl.partials, std::nan(""));
    const uint64_t units = (uint64_t)n_windows * rows * pl.n_chunks;
    const float* x = (const float*)data;
    if (pl.tc) {
        SIM_LAUNCH(clx_k_norm_sum_tc, pl.sum_blocks, clx_norm::kThreads, x, valid, part.data(), rows, T, pl.n_chunks, pl.n_groups);
        if (o.var) SIM_LAUNCH(clx_k_norm_sq_tc, pl.sum_blocks, clx_norm::kThreads, x, valid, part.data(), rows, T, pl.n_chunks, pl.n_groups);
    } else {
        SIM_LAUNCH(clx_k_norm_sum, pl.sum_blocks, clx_norm::kThreads, x, valid, part.data(), rows, T, pl.n_chunks, units);
        if (o.var) SIM_LAUNCH(clx_k_norm_sq, pl.sum_blocks, clx_norm::kThreads, x, valid, part.data(), rows, T, pl.n_chunks, units);
    }
    SIM_LAUNCH(clx_k_norm_apply, n_windows * pl.n_tiles, clx_norm::kThreads, (float*)data, valid, (const double*)part.data(), (float*)stats, o, rows,
               T, pl.n_chunks, pl.tc, pl.n_tiles);
    return CLX_OK;
}
