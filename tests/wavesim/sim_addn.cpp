// TEST INFRASTRUCTURE: the several-noise mixer (claxon_amd/csrc/clx_addn.hip, unmodified, behind clx_norm.hip and clx_add.hip as in
// clx_api.hip) under the wave simulator: clx_addn_check and clx_addn_fill, then the sum, gain and apply kernels launched as
// clx_addn_windows launches them (clx_api.hip), with host buffers in place of device ones.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "clx_norm.hip"
#include "clx_add.hip"
#include "clx_addn.hip"

static char sim_addn_err[256];

extern "C" const char* sim_addn_error(void) { return sim_addn_err; }
extern "C" uint32_t sim_addn_max_terms(void) { return clx_addn::kMaxTerms; }
extern "C" uint32_t sim_addn_max_batches(void) { return clx_addn::kMaxBatches; }
extern "C" uint32_t sim_addn_max_rows(void) { return clx_addn::kMaxRows; }
extern "C" uint32_t sim_addn_rec_bytes(void) { return (uint32_t)sizeof(clx_addn::rec); }
extern "C" uint32_t sim_addn_term_bytes(void) { return (uint32_t)sizeof(clx_addn_term); }

// clx_addn_windows with `data`, the noise batches and `gains` in host memory: CLX_OK, or CLX_API_ERROR with sim_addn_error() saying
// why.  has_opts == 0: opts == NULL, else opts->reserved = reserved.  *launched (may be null): whether the kernels ran.
extern "C" int sim_addn_windows(void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const void* const* noise,
                                const size_t* n_noise, uint32_t n_batches, const uint32_t* noise_valid, const uint32_t* term_first,
                                const clx_addn_term* terms, uint32_t layout, int has_opts, uint32_t reserved, void* gains, int* launched) {
    clx_addn_opts o;
    o.reserved = reserved;
    clx_addn_plan pl;
    if (launched) *launched = 0;
    const char* why = clx_addn_check(data, n_windows, rows, T, valid, noise, n_noise, n_batches, noise_valid, term_first, terms, layout,
                                     has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_addn_err, sizeof sim_addn_err, "%s", why); return CLX_API_ERROR; }
    if (pl.n_chunks == 0) return CLX_OK;
    if (launched) *launched = 1;
    // (the tables start as NaNs: a partial or a gain that is read before it is written shows)
    std::vector<double> part((size_t)pl.partials, std::nan(""));
    std::vector<double> tab(((size_t)pl.table_bytes + pl.n_terms * sizeof(float) + 7) / 8);
    clx_addn_fill(tab.data(), n_windows, rows, T, valid, noise, n_noise, n_batches, noise_valid, term_first, terms);
    float* const gain = (float*)((char*)tab.data() + pl.table_bytes);
    for (uint32_t m = 0; m < pl.n_terms; ++m) gain[m] = std::nanf("");
    const float* x = (const float*)data;
    const uint32_t n = (uint32_t)n_windows;
    if (pl.tc) SIM_LAUNCH(clx_k_addn_sum_tc, pl.sum_blocks, clx_addn::kThreads, x, (const void*)tab.data(), part.data(), n, pl.n_terms, rows, T, pl.n_chunks, pl.units);
    else SIM_LAUNCH(clx_k_addn_sum, pl.sum_blocks, clx_addn::kThreads, x, (const void*)tab.data(), part.data(), n, pl.n_terms, rows, T, pl.n_chunks, pl.units);
    SIM_LAUNCH(clx_k_addn_gain, pl.gain_blocks, clx_addn::kThreads, (const void*)tab.data(), (const double*)part.data(), gain, (float*)gains, n, pl.n_terms, rows,
               pl.n_chunks);
    SIM_LAUNCH(clx_k_addn_apply, n_windows * pl.n_tiles, clx_addn::kThreads, (float*)data, (const void*)tab.data(), (const float*)gain, n, pl.n_terms, rows, T, pl.tc,
               pl.n_tiles);
    return CLX_OK;
}
