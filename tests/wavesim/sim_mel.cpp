// TEST INFRASTRUCTURE: the mel feature kernel (claxon_amd/csrc/clx_mel.hip, unmodified) under the wave simulator: clx_mel_build as
// clx_mel_create runs it, then clx_mel_check, clx_mel_fill and clx_k_mel launched as clx_mel_windows launches it (clx_api.hip), with
// host buffers in place of device ones.  A spec is a small integer here; its tables live until sim_mel_destroy.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <sys/mman.h>
#include <unistd.h>
#include <hip/hip_runtime.h>

#include "clx_mel.hip"

static char sim_mel_err[256];
static std::vector<clx_mel_tables*> sim_specs;

extern "C" const char* sim_mel_error(void) { return sim_mel_err; }
extern "C" uint32_t sim_mel_lds_bytes(void) { return clx_mel::kLdsBytes; }
extern "C" uint32_t sim_mel_group_frames(void) { return clx_mel::kF; }

static clx_mel_tables* sim_spec(int h) { return h >= 0 && (size_t)h < sim_specs.size() ? sim_specs[(size_t)h] : nullptr; }

// clx_mel_create: the spec's number, or -1 with sim_mel_error() saying why
extern "C" int sim_mel_create(uint32_t n_fft, uint32_t hop, const float* window, const float* fbank, uint32_t n_mels, uint32_t mode, float floor) {
    clx_mel_tables* t = new clx_mel_tables();
    const std::string why = clx_mel_build(n_fft, hop, window, fbank, n_mels, mode, floor, t);
    if (!why.empty()) { delete t; snprintf(sim_mel_err, sizeof sim_mel_err, "%s", why.c_str()); return -1; }
    sim_specs.push_back(t);
    return (int)sim_specs.size() - 1;
}

extern "C" void sim_mel_destroy(int h) {
    if (sim_spec(h)) { delete sim_specs[(size_t)h]; sim_specs[(size_t)h] = nullptr; }
}

// the spec's basis out of the padded table, dense: cos_out[j][n] and sin_out[j][n]; and the rows' ends ([n_mels][2])
extern "C" int sim_mel_tables(int h, float* cos_out, float* sin_out, uint32_t* ends_out) {
    const clx_mel_tables* t = sim_spec(h);
    if (!t) return -1;
    const size_t row = (size_t)t->n_pass * clx_mel::kRow;
    for (uint32_t j = 0; j < t->n_bins; ++j)
        for (uint32_t n = 0; n < t->n_fft; ++n) {
            const float* at = t->basis.data() + (size_t)n * row + (size_t)(j / clx_mel::kBins) * clx_mel::kRow + j % clx_mel::kBins;
            cos_out[(size_t)j * t->n_fft + n] = at[0];
            sin_out[(size_t)j * t->n_fft + n] = at[clx_mel::kBins];
        }
    memcpy(ends_out, t->ends.data(), t->ends.size() * 4u);
    // everything else in the table is padding and must be zero
    size_t nonzero = 0;
    for (float v : t->basis) nonzero += v != 0.f || std::signbit(v);
    size_t dense = 0;
    for (uint32_t j = 0; j < t->n_bins; ++j)
        for (uint32_t n = 0; n < t->n_fft; ++n) {
            const size_t i = (size_t)j * t->n_fft + n;
            dense += (cos_out[i] != 0.f || std::signbit(cos_out[i])) + (sin_out[i] != 0.f || std::signbit(sin_out[i]));
        }
    return nonzero == dense ? 0 : 1;
}

// clx_mel_windows with `audio` and `out` in host memory: CLX_OK, or CLX_API_ERROR with sim_mel_error() saying why
extern "C" int sim_mel_windows(int h, const void* audio, size_t n_windows, uint32_t window_len, const uint32_t* valid, uint32_t n_frames,
                               uint32_t layout, void* out) {
    const clx_mel_tables* t = sim_spec(h);
    uint32_t n_groups = 0;
    const char* why = clx_mel_check(t, audio, n_windows, window_len, valid, n_frames, layout, out, &n_groups);
    if (why) { snprintf(sim_mel_err, sizeof sim_mel_err, "%s", why); return CLX_API_ERROR; }
    if (n_groups == 0) return CLX_OK;
    std::vector<uint32_t> vf(n_windows);
    clx_mel_fill(vf.data(), valid, n_windows, t->hop, n_frames);
    const clx_mel_dev dev = clx_mel_args(*t, t->basis.data(), t->fbank.data(), t->ends.data());
    SIM_LAUNCH(clx_k_mel, n_windows * n_groups, clx_mel::kThreads, (const float*)audio, (const uint32_t*)vf.data(), dev, n_groups, window_len, n_frames,
               layout, (float*)out);
    return CLX_OK;
}

// The batch (n_windows * window_len floats, given in `floats`) sits flush against an inaccessible page: the page follows its last
// float (at_end), or precedes its first.  A load on the wrong side of either end faults instead of reading a neighbour's bytes.
extern "C" int sim_mel_guarded(int h, const float* floats, size_t n_windows, uint32_t window_len, const uint32_t* valid, uint32_t n_frames,
                               uint32_t layout, int at_end, void* out) {
    const size_t len = n_windows * (size_t)window_len * 4u;
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), body = (len + pg - 1) / pg * pg + pg;
    uint8_t* m = (uint8_t*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == (uint8_t*)MAP_FAILED) return -1;
    mprotect(m, pg, PROT_NONE);
    mprotect(m + pg + body, pg, PROT_NONE);
    uint8_t* p = at_end ? m + pg + body - len : m + pg;
    memcpy(p, floats, len);
    const int st = sim_mel_windows(h, p, n_windows, window_len, valid, n_frames, layout, out);
    munmap(m, body + 2 * pg);
    return st;
}

// the last step of the kernel on its own: out[i] = finish(mode, floor, m[i]) (the simulator's logf / log10f, for LOG_ULPS)
extern "C" void sim_mel_finish(uint32_t mode, float floor, const float* m, size_t n, float* out) {
    for (size_t i = 0; i < n; ++i) out[i] = clx_mel::finish(mode, floor, m[i]);
}
