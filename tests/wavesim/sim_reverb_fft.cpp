// TEST INFRASTRUCTURE: the partitioned FFT reverberator (claxon_amd/csrc/clx_reverb_fft.hip, unmodified, behind clx_norm.hip,
// clx_add.hip and clx_reverb.hip as in clx_api.hip) under the wave simulator: clx_rvfft_check, clx_rvfft_plan_call and
// clx_rvfft_fill, then the forward and the multiply-accumulate kernels, clx_add's sum kernels, the gain and the scale kernels
// launched as clx_reverb_windows_fft launches them (clx_api.hip), with host buffers in place of device ones.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "clx_norm.hip"
#include "clx_add.hip"
#include "clx_reverb.hip"
#include "clx_reverb_fft.hip"

static char sim_rvfft_err[256];

extern "C" const char* sim_rvfft_error(void) { return sim_rvfft_err; }
extern "C" uint32_t sim_rvfft_hop(void) { return clx_rvfft::kHop; }
extern "C" uint32_t sim_rvfft_n(void) { return clx_rvfft::kN; }
extern "C" uint32_t sim_rvfft_bins(void) { return clx_rvfft::kBins; }
extern "C" uint32_t sim_rvfft_spec(void) { return clx_rvfft::kSpec; }
extern "C" uint32_t sim_rvfft_lds_bytes(void) { return clx_rvfft::kLdsBytes; }
extern "C" uint32_t sim_rvfft_win_bytes(void) { return clx_rvfft::kWinBytes; }
// the N / 2 twiddles as (re, im) float32 pairs: the table the device gets
extern "C" void sim_rvfft_twiddles(float* tw) { clx_rvfft_twiddles((clx_rvfft::cf*)tw); }

// clx_reverb_windows_fft with `data`, `ir`, `out` and `gains` in host memory: CLX_OK, or CLX_API_ERROR with sim_rvfft_error() saying
// why.  has_opts == 0: opts == NULL, else opts = { keep_power, { reserved, 0, reserved2 } }.  *launched (may be null): whether the
// kernels ran; *slots (may be null): the spectra of the workspace; *n_jobs: the partitions transformed.
extern "C" int sim_rvfft_windows(const void* data, size_t n_windows, uint32_t rows, uint32_t T, const uint32_t* valid, const void* ir, size_t n_ir,
                                 uint32_t K, const uint32_t* ir_len, const int32_t* ir_index, uint32_t layout, int has_opts, uint32_t keep_power,
                                 uint32_t reserved, uint32_t reserved2, void* out, void* gains, int* launched, uint64_t* slots, uint32_t* n_jobs) {
    clx_reverb_fft_opts o;
    o.keep_power = keep_power; o.reserved[0] = reserved; o.reserved[1] = 0; o.reserved[2] = reserved2;
    clx_reverb_plan pl;
    clx_rvfft_plan fp;
    if (launched) *launched = 0;
    std::string why = clx_rvfft_check(data, n_windows, rows, T, valid, ir, n_ir, K, ir_len, ir_index, layout, has_opts ? &o : nullptr, out, &pl);
    if (!why.empty()) { snprintf(sim_rvfft_err, sizeof sim_rvfft_err, "%s", why.c_str()); return CLX_API_ERROR; }
    if (pl.n_tiles == 0) return CLX_OK;
    why = clx_rvfft_plan_call(n_windows, rows, T, valid, ir_len, ir_index, n_ir, &fp);
    if (!why.empty()) { snprintf(sim_rvfft_err, sizeof sim_rvfft_err, "%s", why.c_str()); return CLX_API_ERROR; }
    if (launched) *launched = 1;
    if (slots) *slots = fp.slots();
    if (n_jobs) *n_jobs = (uint32_t)(fp.jobs.size() / 3u);
    // (the tables start as NaNs: a partial, a gain or a spectrum that is read before it is written shows)
    std::vector<double> part((size_t)pl.partials, std::nan(""));
    std::vector<double> tab((fp.table_bytes(n_windows) + 7) / 8);
    clx_rvfft_fill(tab.data(), n_windows, valid, ir_len, ir_index, has_opts ? keep_power : 0u, &fp);
    float* const gain = (float*)((char*)tab.data() + n_windows * clx_reverb::kTableBytes);
    for (size_t k = 0; k < n_windows; ++k) gain[k] = std::nanf("");
    std::vector<clx_rvfft::cf> tw(clx_rvfft::kN / 2u);
    clx_rvfft_twiddles(tw.data());
    std::vector<clx_rvfft::cf> ws((size_t)fp.slots() * clx_rvfft::kSpec, clx_rvfft::cf{ std::nanf(""), std::nanf("") });
    const float* x = (const float*)data;
    const uint32_t n = (uint32_t)n_windows;
    SIM_LAUNCH(clx_k_rvfft_fwd, fp.slots(), clx_rvfft::kThreads, x, (const float*)ir, (const void*)tab.data(), (const clx_rvfft::cf*)tw.data(), ws.data(), n, rows, T,
               K, pl.tc, fp.nb, (uint32_t)fp.n_seg);
    SIM_LAUNCH(clx_k_rvfft_mac, fp.n_seg, clx_rvfft::kThreads, x, (const void*)tab.data(), (const clx_rvfft::cf*)tw.data(), (const clx_rvfft::cf*)ws.data(),
               (float*)out, n, rows, T, pl.tc, fp.nb, (uint32_t)fp.n_seg);
    if (pl.power) {
        if (pl.tc) SIM_LAUNCH(clx_k_add_sum_tc, pl.sum_blocks, clx_add::kThreads, x, (const float*)out, (const void*)tab.data(), part.data(), n, rows, T, pl.n_chunks, pl.units);
        else SIM_LAUNCH(clx_k_add_sum, pl.sum_blocks, clx_add::kThreads, x, (const float*)out, (const void*)tab.data(), part.data(), n, rows, T, pl.n_chunks, pl.units);
    }
    if (pl.power || gains)
        SIM_LAUNCH(clx_k_reverb_gain, pl.gain_blocks, clx_reverb::kThreads, (const void*)tab.data(), (const double*)(pl.power ? part.data() : nullptr), gain,
                   (float*)gains, n, rows, pl.n_chunks);
    if (pl.power)
        SIM_LAUNCH(clx_k_reverb_scale, n_windows * pl.lines * pl.scale_tiles, clx_reverb::kThreads, (float*)out, (const void*)tab.data(), (const float*)gain, n,
                   pl.lines, pl.line_len, pl.mult, pl.scale_tiles);
    return CLX_OK;
}
