// TEST INFRASTRUCTURE: frame splicing (claxon_amd/csrc/clx_splice.hip, unmodified) under the wave simulator: clx_splice_check, the
// per-call table, then the kernel launched as clx_splice_windows launches it (clx_api.hip), with host buffers in place of device
// ones; and the host builder of the delta plan.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "clx_splice.hip"

static char sim_splice_err[256];
static clx_splice_plan sim_splice_last;

extern "C" const char* sim_splice_error(void) { return sim_splice_err; }
extern "C" uint32_t sim_splice_tile(void) { return clx_splice::kTile; }
extern "C" uint32_t sim_splice_threads(void) { return clx_splice::kThreads; }
extern "C" uint32_t sim_splice_stage_words(void) { return clx_splice::kStageWords; }
extern "C" uint32_t sim_splice_lds_bytes(void) { return clx_splice::kLdsBytes; }
// the sub-tile of the last call that launched: (Fs, Rc, H)
extern "C" void sim_splice_shape(uint32_t* out) { out[0] = sim_splice_last.Fs; out[1] = sim_splice_last.Rc; out[2] = sim_splice_last.H; }

// clx_splice_windows with `in` and `out` in host memory: CLX_OK, or CLX_API_ERROR with sim_splice_error() saying why.
// has_opts == 0: opts == NULL.
extern "C" int sim_splice_windows(const void* in, void* out, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, uint32_t layout,
                                  const clx_splice_block* blocks, const float* coefs, int has_opts, uint32_t K, uint32_t stride, float pad,
                                  uint32_t reserved) {
    clx_splice_opts o;
    o.n_blocks = K; o.stride = stride; o.pad = pad; o.reserved = reserved;
    clx_splice_plan pl;
    const char* why = clx_splice_check(in, out, n_windows, rows, T, valid, layout, blocks, coefs, has_opts ? &o : nullptr, &pl);
    if (why) { snprintf(sim_splice_err, sizeof sim_splice_err, "%s", why); return CLX_API_ERROR; }
    if (pl.n_tiles == 0) return CLX_OK;
    sim_splice_last = pl;
    std::vector<uint32_t> tab((size_t)pl.table_words, 0x7fc00001u);
    clx_splice_fill_table(tab.data(), n_windows, valid, blocks, coefs, K);
    uint32_t padw;
    memcpy(&padw, &o.pad, sizeof padw);
    SIM_LAUNCH(clx_k_splice, n_windows * pl.n_tiles, clx_splice::kThreads, (const uint32_t*)in, (uint32_t*)out, (const uint32_t*)tab.data(),
               (uint32_t)n_windows, rows, T, pl.T_out, K, stride, pl.H, pl.n_coefs, padw, pl.tc, pl.n_tiles, pl.Fs, pl.Rc);
    return CLX_OK;
}

extern "C" int sim_splice_deltas(uint32_t order, uint32_t window, clx_splice_block* blocks, float* coefs, uint32_t* n_coefs) {
    const char* why = clx_splice_deltas_build(order, window, blocks, coefs, n_coefs);
    if (why) { snprintf(sim_splice_err, sizeof sim_splice_err, "%s", why); return CLX_API_ERROR; }
    return CLX_OK;
}
