// TEST INFRASTRUCTURE: the CMVN accumulator and the grouped normalisation (claxon_amd/csrc/clx_cmvn_stats.hip, unmodified, behind
// clx_norm.hip and clx_cmvn.hip as in the library) under the wave simulator: the argument checks, the per-call table, then the
// kernels launched as clx_cmvn_stats_windows / clx_cmvn_grouped_windows launch them (clx_api.hip), with host buffers in place of
// device ones; the chunk partials beside clx_norm's own sum kernels on the same data; and the solve alone.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "clx_norm.hip"
#include "clx_cmvn.hip"
#include "clx_cmvn_stats.hip"

static char sim_cs_err[256];
static clx_cmvn_stats_plan sim_cs_last;
static uint32_t sim_cs_launches, sim_cs_present;
static std::vector<uint32_t> sim_cs_slot;

extern "C" const char* sim_cmvn_stats_error(void) { return sim_cs_err; }
extern "C" uint32_t sim_cmvn_stats_threads(void) { return clx_cmvn_stats::kThreads; }
extern "C" uint32_t sim_cmvn_stats_chunk(void) { return clx_cmvn_stats::kChunk; }
extern "C" uint32_t sim_cmvn_stats_strands(void) { return clx_cmvn_stats::kStrands; }
extern "C" uint32_t sim_cmvn_stats_vecs(void) { return clx_cmvn_stats::kVecs; }
extern "C" uint32_t sim_cmvn_stats_max_groups(void) { return clx_cmvn_stats::kMaxGroups; }
extern "C" uint32_t sim_cmvn_stats_sum_lds_bytes(void) { return clx_cmvn_stats::kSumLdsBytes; }
extern "C" uint32_t sim_cmvn_stats_sum_tc_lds_bytes(void) { return clx_cmvn_stats::kSumTcLdsBytes; }
extern "C" uint32_t sim_cmvn_stats_fold_lds_bytes(void) { return clx_cmvn_stats::kFoldLdsBytes; }
extern "C" uint32_t sim_cmvn_stats_solve_lds_bytes(void) { return clx_cmvn_stats::kSolveLdsBytes; }
extern "C" uint32_t sim_cmvn_stats_apply_lds_bytes(void) { return clx_cmvn_stats::kApplyLdsBytes; }
// kernels launched since the library was loaded
extern "C" uint32_t sim_cmvn_stats_launch_count(void) { return sim_cs_launches; }
// the plan of the last call that launched: (n_chunks, tc, sum_blocks, n_tiles, solve_blocks, partials, table words, present groups)
extern "C" void sim_cmvn_stats_shape(uint32_t* out) {
    out[0] = sim_cs_last.n_chunks; out[1] = sim_cs_last.tc; out[2] = sim_cs_last.sum_blocks; out[3] = sim_cs_last.n_tiles;
    out[4] = sim_cs_last.solve_blocks; out[5] = (uint32_t)sim_cs_last.partials; out[6] = (uint32_t)sim_cs_last.table_words; out[7] = sim_cs_present;
}
// clx_cmvn_stats_fill_table with csr: tab receives 5 n + 1 words; returns the present groups; the work array must come back as zeros
extern "C" int sim_cmvn_stats_table(uint32_t* tab, size_t n_windows, const uint32_t* valid, const int32_t* group, uint32_t n_groups) {
    const uint32_t present = clx_cmvn_stats_fill_table(tab, n_windows, valid, group, n_groups, true, sim_cs_slot);
    for (uint32_t v : sim_cs_slot) if (v) return -1;
    return (int)present;
}

static void sim_cs_sum(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const clx_cmvn_stats_plan& pl, const uint32_t* tab, double* part) {
    ++sim_cs_launches;
    if (pl.tc)
        SIM_LAUNCH(clx_k_cmvn_stats_sum_tc, pl.sum_blocks, clx_cmvn_stats::kThreads, (const float*)data, tab, part, (uint32_t)n_windows, rows, T,
                   pl.n_chunks, pl.n_rgroups);
    else
        SIM_LAUNCH(clx_k_cmvn_stats_sum, pl.sum_blocks, clx_cmvn_stats::kThreads, (const float*)data, tab, part, (uint32_t)n_windows, rows, T,
                   pl.n_chunks, (uint64_t)n_windows * rows * pl.n_chunks);
}

// clx_cmvn_stats_windows with `data` and `stats` in host memory: CLX_OK, or CLX_API_ERROR with sim_cmvn_stats_error() saying why.
// has_opts == 0: opts == NULL.
extern "C" int sim_cmvn_stats_windows(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                      const int32_t* group, uint32_t n_groups, void* stats, int has_opts, uint32_t accumulate, uint32_t reserved) {
    clx_cmvn_stats_opts o;
    o.accumulate = accumulate; o.reserved = reserved;
    clx_cmvn_stats_plan pl;
    const char* why = clx_cmvn_stats_check(data, n_windows, rows, T, valid, layout, group, n_groups, stats, has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_cs_err, sizeof sim_cs_err, "%s", why); return CLX_API_ERROR; }
    if (!pl.launch && o.accumulate) return CLX_OK;
    if (!pl.launch) { memset(stats, 0, (size_t)pl.stats_bytes); return CLX_OK; }
    sim_cs_last = pl;
    std::vector<uint32_t> tab((size_t)pl.table_words, 0x7fc00001u);
    const uint32_t present = clx_cmvn_stats_fill_table(tab.data(), n_windows, valid, group, n_groups, true, sim_cs_slot);
    sim_cs_present = present;
    if (!o.accumulate) memset(stats, 0, (size_t)pl.stats_bytes);
    if (!present) return CLX_OK;
    // (the partial sums start as NaNs: one that is read before it is written shows)
    std::vector<double> part((size_t)pl.partials, std::nan(""));
    sim_cs_sum(data, n_windows, rows, T, pl, tab.data(), part.data());
    const uint64_t lanes = (uint64_t)present * 2u * (rows + 1u);
    ++sim_cs_launches;
    SIM_LAUNCH(clx_k_cmvn_stats_fold, (lanes + clx_cmvn_stats::kThreads - 1u) / clx_cmvn_stats::kThreads, clx_cmvn_stats::kThreads,
               (const double*)part.data(), (const uint32_t*)tab.data(), (double*)stats, (uint32_t)n_windows, rows, pl.n_chunks, lanes);
    return CLX_OK;
}

// clx_cmvn_grouped_windows with `data`, `stats` and `ss` in host memory, likewise.
extern "C" int sim_cmvn_grouped_windows(void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                        const int32_t* group, uint32_t n_groups, const void* stats, void* ss, int has_opts, uint32_t norm_vars, float pad,
                                        uint32_t reserved) {
    clx_cmvn_grouped_opts o;
    o.norm_vars = norm_vars; o.pad = pad; o.reserved = reserved;
    clx_cmvn_stats_plan pl;
    const char* why = clx_cmvn_grouped_check(data, n_windows, rows, T, valid, layout, group, n_groups, stats, ss, has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_cs_err, sizeof sim_cs_err, "%s", why); return CLX_API_ERROR; }
    if (!pl.launch) return CLX_OK;
    sim_cs_last = pl;
    std::vector<uint32_t> tab((size_t)pl.table_words, 0x7fc00001u);
    (void)clx_cmvn_stats_fill_table(tab.data(), n_windows, valid, group, n_groups, false, sim_cs_slot);
    sim_cs_launches += 2u;
    SIM_LAUNCH(clx_k_cmvn_stats_solve, pl.solve_blocks, clx_cmvn_stats::kThreads, (const double*)stats, (float*)ss, n_groups, rows, o.norm_vars);
    SIM_LAUNCH(clx_k_cmvn_grouped, n_windows * pl.n_tiles, clx_cmvn_stats::kThreads, (float*)data, (const uint32_t*)tab.data(), (const float*)ss,
               (uint32_t)n_windows, rows, T, o.pad, pl.tc, pl.n_tiles);
    return CLX_OK;
}

// clx_k_cmvn_stats_solve alone: stats [n_groups][2][rows + 1] doubles into ss [n_groups][2][rows] floats
extern "C" void sim_cmvn_stats_solve(const double* stats, uint32_t n_groups, uint32_t rows, uint32_t norm_vars, float* ss) {
    const uint64_t blocks = ((uint64_t)n_groups * rows + clx_cmvn_stats::kThreads - 1u) / clx_cmvn_stats::kThreads;
    ++sim_cs_launches;
    SIM_LAUNCH(clx_k_cmvn_stats_solve, blocks, clx_cmvn_stats::kThreads, stats, ss, n_groups, rows, norm_vars);
}

// The chunk partials [n_windows][rows][2][n_chunks] of this file's sum kernel into `mine` and of clx_norm's own sum kernel
// (clx_k_norm_sum / clx_k_norm_sum_tc, launched as clx_norm_windows launches them; the Q half is left alone) into `norms`, over the
// same data; what neither writes keeps what the caller put there.  Returns n_chunks, or -1 with sim_cmvn_stats_error().
extern "C" int sim_cmvn_stats_partials(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                       double* mine, double* norms) {
    uint8_t dummy[8] __attribute__((aligned(8)));
    clx_cmvn_stats_opts o;
    o.accumulate = 1u; o.reserved = 0u;
    clx_cmvn_stats_plan pl;
    const char* why = clx_cmvn_stats_check(data, n_windows, rows, T, valid, layout, nullptr, 1u, dummy, &o, &pl);
    if (why) { snprintf(sim_cs_err, sizeof sim_cs_err, "%s", why); return -1; }
    if (!pl.launch) return 0;
    std::vector<uint32_t> tab((size_t)pl.table_words, 0x7fc00001u);
    (void)clx_cmvn_stats_fill_table(tab.data(), n_windows, valid, nullptr, 1u, true, sim_cs_slot);
    sim_cs_sum(data, n_windows, rows, T, pl, tab.data(), mine);
    if (pl.tc) SIM_LAUNCH(clx_k_norm_sum_tc, pl.sum_blocks, clx_norm::kThreads, (const float*)data, valid, norms, rows, T, pl.n_chunks, pl.n_rgroups);
    else SIM_LAUNCH(clx_k_norm_sum, pl.sum_blocks, clx_norm::kThreads, (const float*)data, valid, norms, rows, T, pl.n_chunks,
                    (uint64_t)n_windows * rows * pl.n_chunks);
    return (int)pl.n_chunks;
}
