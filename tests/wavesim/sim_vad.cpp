// TEST INFRASTRUCTURE: the energy VAD and the frame selection (claxon_amd/csrc/clx_vad.hip, unmodified, behind clx_norm.hip as in
// the library) under the wave simulator: the argument checks, then the kernels launched as clx_vad_windows / clx_select_windows
// launch them (clx_api.hip), with host buffers in place of device ones; and the context rule.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "clx_norm.hip"
#include "clx_vad.hip"

static char sim_vad_err[256];
static clx_vad_plan sim_vad_last;
static uint32_t sim_vad_launches;

extern "C" const char* sim_vad_error(void) { return sim_vad_err; }
extern "C" uint32_t sim_vad_tile(void) { return clx_vad::kTile; }
extern "C" uint32_t sim_vad_threads(void) { return clx_vad::kThreads; }
extern "C" uint32_t sim_vad_span(void) { return clx_vad::kSpan; }
extern "C" uint32_t sim_vad_max_context(void) { return clx_vad::kMaxContext; }
extern "C" uint32_t sim_vad_sum_lds_bytes(void) { return clx_vad::kSumLdsBytes; }
extern "C" uint32_t sim_vad_decide_lds_bytes(void) { return clx_vad::kDecideLdsBytes; }
extern "C" uint32_t sim_vad_rank_lds_bytes(void) { return clx_vad::kRankLdsBytes; }
extern "C" uint32_t sim_vad_scan_lds_bytes(void) { return clx_vad::kScanLdsBytes; }
extern "C" uint32_t sim_vad_move_lds_bytes(void) { return clx_vad::kMoveLdsBytes; }
// kernels launched since the library was loaded
extern "C" uint32_t sim_vad_launch_count(void) { return sim_vad_launches; }
// the plan of the last call that launched: (n_tiles, n_chunks, sum_blocks, scan_blocks, partials, table words)
extern "C" void sim_vad_shape(uint32_t* out) {
    out[0] = sim_vad_last.n_tiles; out[1] = sim_vad_last.n_chunks; out[2] = sim_vad_last.sum_blocks; out[3] = sim_vad_last.scan_blocks;
    out[4] = (uint32_t)sim_vad_last.partials; out[5] = (uint32_t)sim_vad_last.table_words;
}
// clx_vad::context
extern "C" void sim_vad_context(uint32_t t, uint32_t V, uint32_t c, uint32_t* lh) { clx_vad::context(t, V, c, lh, lh + 1); }

// clx_vad_windows with `data`, `mask` and `thresholds` in host memory: CLX_OK, or CLX_API_ERROR with sim_vad_error() saying why.
// has_opts == 0: opts == NULL.
extern "C" int sim_vad_windows(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout, int has_opts,
                               float E, float s, uint32_t c, float p, uint32_t row, const uint32_t* reserved, void* mask, void* thresholds) {
    clx_vad_opts o;
    o.energy_threshold = E; o.energy_mean_scale = s; o.frames_context = c; o.proportion_threshold = p; o.row = row;
    for (int i = 0; i < 3; ++i) o.reserved[i] = reserved ? reserved[i] : 0u;
    clx_vad_plan pl;
    const char* why = clx_vad_check(data, n_windows, rows, T, valid, layout, has_opts ? &o : nullptr, mask, &pl);
    if (why) { snprintf(sim_vad_err, sizeof sim_vad_err, "%s", why); return CLX_API_ERROR; }
    if (pl.n_tiles == 0) return CLX_OK;
    sim_vad_last = pl;
    std::vector<uint32_t> tab(valid, valid + n_windows);
    // (the partial sums start as NaNs: one that is read before it is written shows)
    std::vector<double> part((size_t)pl.partials + 1u, std::nan(""));
    if (pl.sum_blocks) {
        ++sim_vad_launches;
        SIM_LAUNCH(clx_k_vad_sum, pl.sum_blocks, clx_vad::kThreads, (const float*)data, (const uint32_t*)tab.data(), part.data(), rows, T, o.row, pl.tc,
                   pl.n_chunks, (uint64_t)n_windows * pl.n_chunks);
    }
    ++sim_vad_launches;
    SIM_LAUNCH(clx_k_vad_decide, n_windows * pl.n_tiles, clx_vad::kThreads, (const float*)data, (const uint32_t*)tab.data(), (const double*)part.data(),
               (uint8_t*)mask, (float*)thresholds, o, rows, T, pl.tc, pl.n_chunks, pl.n_tiles);
    return CLX_OK;
}

// clx_select_windows with everything in host memory, likewise; `counts` plays d_counts and counts alike.
extern "C" int sim_select_windows(const void* src, void* dst, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const void* mask,
                                  uint32_t layout, int has_opts, float pad, const uint32_t* reserved, uint32_t* counts) {
    clx_select_opts o;
    o.pad = pad;
    for (int i = 0; i < 3; ++i) o.reserved[i] = reserved ? reserved[i] : 0u;
    clx_vad_plan pl;
    const char* why = clx_select_check(src, dst, n_windows, rows, T, valid, mask, layout, has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_vad_err, sizeof sim_vad_err, "%s", why); return CLX_API_ERROR; }
    if (pl.n_tiles == 0) {
        if (counts) memset(counts, 0, n_windows * sizeof(uint32_t));
        return CLX_OK;
    }
    sim_vad_last = pl;
    std::vector<uint32_t> tab((size_t)pl.table_words, 0x7fc00001u);
    memcpy(tab.data(), valid, n_windows * sizeof(uint32_t));
    uint32_t* const d_count = tab.data() + n_windows;
    uint32_t* const d_tile_counts = d_count + n_windows;
    uint32_t* const d_tile_base = d_tile_counts + n_windows * (size_t)pl.n_tiles;
    uint32_t pad_word;
    memcpy(&pad_word, &o.pad, sizeof pad_word);
    sim_vad_launches += 3u;
    SIM_LAUNCH(clx_k_select_rank, n_windows * pl.n_tiles, clx_vad::kThreads, (const uint8_t*)mask, (const uint32_t*)tab.data(), d_tile_counts, T,
               pl.n_tiles);
    SIM_LAUNCH(clx_k_select_scan, pl.scan_blocks, clx_vad::kThreads, (const uint32_t*)d_tile_counts, d_tile_base, d_count, counts, (uint32_t)n_windows,
               pl.n_tiles);
    SIM_LAUNCH(clx_k_select_move, n_windows * pl.n_tiles, clx_vad::kThreads, (const uint32_t*)src, (uint32_t*)dst, (const uint8_t*)mask,
               (const uint32_t*)tab.data(), (const uint32_t*)d_tile_base, (const uint32_t*)d_count, rows, T, pad_word, pl.tc, pl.n_tiles);
    return CLX_OK;
}
