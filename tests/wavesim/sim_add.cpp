// TEST INFRASTRUCTURE: the noise mixer (claxon_amd/csrc/clx_add.hip, unmodified, behind clx_norm.hip as in clx_api.hip) under the
// wave simulator: clx_add_check and clx_add_fill, then the sum, gain and apply kernels launched as clx_add_windows launches them
// (clx_api.hip), with host buffers in place of device ones.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "clx_norm.hip"
#include "clx_add.hip"

static char sim_add_err[256];

extern "C" const char* sim_add_error(void) { return sim_add_err; }
extern "C" uint32_t sim_add_chunk(void) { return clx_add::kChunk; }
extern "C" uint32_t sim_add_strands(void) { return clx_add::kStrands; }
extern "C" uint32_t sim_add_max_rows(void) { return clx_add::kMaxRows; }
extern "C" uint32_t sim_add_table_bytes(void) { return clx_add::kTableBytes; }

// clx_add_windows with `data`, `noise` and `gains` in host memory: CLX_OK, or CLX_API_ERROR with sim_add_error() saying why.
// has_opts == 0: opts == NULL, else opts->reserved = reserved.  *launched (may be null): whether the kernels ran.
extern "C" int sim_add_windows(void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const void* noise, size_t n_noise,
                               const uint32_t* noise_valid, const int32_t* noise_index, const float* snr_db, uint32_t layout, int has_opts,
                               uint32_t reserved, void* gains, int* launched) {
    clx_add_opts o;
    o.reserved = reserved;
    clx_add_plan pl;
    if (launched) *launched = 0;
    const char* why = clx_add_check(data, n_windows, rows, T, valid, noise, n_noise, noise_valid, noise_index, snr_db, layout, has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_add_err, sizeof sim_add_err, "%s", why); return CLX_API_ERROR; }
    if (pl.n_chunks == 0) return CLX_OK;
    if (launched) *launched = 1;
    // (the tables start as NaNs: a partial or a gain that is read before it is written shows)
    std::vector<double> part((size_t)pl.partials, std::nan(""));
    std::vector<double> tab((n_windows * clx_add::kTableBytesDevice + 7) / 8);
    clx_add_fill(tab.data(), n_windows, valid, noise_valid, noise_index, snr_db);
    float* const gain = (float*)((char*)tab.data() + n_windows * clx_add::kTableBytes);
    for (size_t k = 0; k < n_windows; ++k) gain[k] = std::nanf("");
    const float* x = (const float*)data;
    const uint32_t n = (uint32_t)n_windows;
    if (pl.tc) SIM_LAUNCH(clx_k_add_sum_tc, pl.sum_blocks, clx_add::kThreads, x, (const float*)noise, (const void*)tab.data(), part.data(), n, rows, T, pl.n_chunks, pl.units);
    else SIM_LAUNCH(clx_k_add_sum, pl.sum_blocks, clx_add::kThreads, x, (const float*)noise, (const void*)tab.data(), part.data(), n, rows, T, pl.n_chunks, pl.units);
    SIM_LAUNCH(clx_k_add_gain, pl.gain_blocks, clx_add::kThreads, (const void*)tab.data(), (const double*)part.data(), gain, (float*)gains, n, rows, pl.n_chunks);
    SIM_LAUNCH(clx_k_add_apply, n_windows * pl.n_tiles, clx_add::kThreads, (float*)data, (const float*)noise, (const void*)tab.data(), (const float*)gain, n, rows, T,
               pl.tc, pl.n_tiles);
    return CLX_OK;
}
