// TEST INFRASTRUCTURE: global and sliding-window CMVN (claxon_amd/csrc/clx_cmvn.hip, unmodified) under the wave simulator: the
// argument checks, the per-call table, then each kernel launched as clx_cmvn_global_windows / clx_cmvn_sliding_windows launch it
// (clx_api.hip), with host buffers in place of device ones; the statistics window rule and the host builder of shift and scale.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "clx_cmvn.hip"

static char sim_cmvn_err[256];
static clx_cmvn_plan sim_cmvn_last;
static uint32_t sim_cmvn_launches;

extern "C" const char* sim_cmvn_error(void) { return sim_cmvn_err; }
extern "C" uint32_t sim_cmvn_tile(void) { return clx_cmvn::kTile; }
extern "C" uint32_t sim_cmvn_threads(void) { return clx_cmvn::kThreads; }
extern "C" uint32_t sim_cmvn_row_chunk(void) { return clx_cmvn::kRc; }
extern "C" uint32_t sim_cmvn_max_span(void) { return clx_cmvn::kMaxSpan; }
extern "C" uint32_t sim_cmvn_sliding_lds_bytes(void) { return clx_cmvn::kSlidingLdsBytes; }
extern "C" uint32_t sim_cmvn_global_lds_bytes(void) { return clx_cmvn::kGlobalLdsBytes; }
// kernels launched since the library was loaded
extern "C" uint32_t sim_cmvn_launch_count(void) { return sim_cmvn_launches; }
// the plan of the last call that launched: (n_tiles, Rc, span, table words)
extern "C" void sim_cmvn_shape(uint32_t* out) {
    out[0] = sim_cmvn_last.n_tiles; out[1] = sim_cmvn_last.Rc; out[2] = sim_cmvn_last.span; out[3] = (uint32_t)sim_cmvn_last.table_words;
}
// clx_cmvn::stat_window
extern "C" void sim_cmvn_window(uint32_t t, uint32_t V, uint32_t N, uint32_t M, uint32_t center, uint32_t* ab) {
    clx_cmvn::stat_window(t, V, N, M, center, ab, ab + 1);
}

// clx_cmvn_global_windows with `data` in host memory: CLX_OK, or CLX_API_ERROR with sim_cmvn_error() saying why.
// has_opts == 0: opts == NULL.
extern "C" int sim_cmvn_global_windows(void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                       const float* shift, const float* scale, int has_opts, float pad, uint32_t reserved) {
    clx_cmvn_global_opts o;
    o.pad = pad; o.reserved = reserved;
    clx_cmvn_plan pl;
    const char* why = clx_cmvn_check_global(data, n_windows, rows, T, valid, layout, shift, scale, has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_cmvn_err, sizeof sim_cmvn_err, "%s", why); return CLX_API_ERROR; }
    if (pl.n_tiles == 0) return CLX_OK;
    sim_cmvn_last = pl;
    std::vector<uint32_t> tab((size_t)pl.table_words, 0x7fc00001u);
    clx_cmvn_fill_table(tab.data(), n_windows, valid, rows, shift, scale);
    ++sim_cmvn_launches;
    SIM_LAUNCH(clx_k_cmvn_global, n_windows * pl.n_tiles, clx_cmvn::kThreads, (float*)data, (const uint32_t*)tab.data(), (uint32_t)n_windows, rows, T,
               o.pad, pl.tc, pl.n_tiles);
    return CLX_OK;
}

// clx_cmvn_sliding_windows with `in` and `out` in host memory, likewise.
extern "C" int sim_cmvn_sliding_windows(const void* in, void* out, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                        int has_opts, uint32_t window, uint32_t min_window, uint32_t center, uint32_t norm_vars, float pad,
                                        uint32_t reserved) {
    clx_cmvn_sliding_opts o;
    o.window = window; o.min_window = min_window; o.center = center; o.norm_vars = norm_vars; o.pad = pad; o.reserved = reserved;
    clx_cmvn_plan pl;
    const char* why = clx_cmvn_check_sliding(in, out, n_windows, rows, T, valid, layout, has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_cmvn_err, sizeof sim_cmvn_err, "%s", why); return CLX_API_ERROR; }
    if (pl.n_tiles == 0) return CLX_OK;
    sim_cmvn_last = pl;
    std::vector<uint32_t> tab((size_t)pl.table_words, 0x7fc00001u);
    clx_cmvn_fill_table(tab.data(), n_windows, valid, rows, nullptr, nullptr);
    ++sim_cmvn_launches;
    SIM_LAUNCH(clx_k_cmvn_sliding, n_windows * pl.n_tiles, clx_cmvn::kThreads, (const float*)in, (float*)out, (const uint32_t*)tab.data(), rows, T,
               o.window, o.center ? 1u : o.min_window, o.center, o.norm_vars, o.pad, pl.tc, pl.n_tiles);
    return CLX_OK;
}

extern "C" int sim_cmvn_from_stats(const double* stats, uint32_t rows, uint32_t norm_vars, float* shift, float* scale) {
    const char* why = clx_cmvn_from_stats_build(stats, rows, norm_vars, shift, scale);
    if (why) { snprintf(sim_cmvn_err, sizeof sim_cmvn_err, "%s", why); return CLX_API_ERROR; }
    return CLX_OK;
}
