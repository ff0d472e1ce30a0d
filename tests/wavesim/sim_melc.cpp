// TEST INFRASTRUCTURE: the centred and range-scaled mel features (claxon_amd/csrc/clx_mel.hip, unmodified) under the wave simulator:
// clx_mel_build with options as clx_mel_create_ex runs it, then clx_mel_check, the table fill and clx_k_mel / clx_k_mel_c /
// clx_k_mel_range launched as clx_mel_windows launches them (clx_api.hip), with host buffers in place of device ones.  A spec is a
// small integer here; its tables live until sim_melc_destroy.
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

static char sim_melc_err[256];
static std::vector<clx_mel_tables*> sim_specs;

extern "C" const char* sim_melc_error(void) { return sim_melc_err; }
extern "C" uint32_t sim_melc_lds_bytes(void) { return clx_mel::kLdsBytes; }
extern "C" uint32_t sim_melc_range_vectors(void) { return clx_mel::kRangeVecs; }

static clx_mel_tables* sim_spec(int h) { return h >= 0 && (size_t)h < sim_specs.size() ? sim_specs[(size_t)h] : nullptr; }

// clx_mel_create_ex (has_opts == 0: opts == NULL, i.e. clx_mel_create): the spec's number, or -1 with sim_melc_error() saying why
extern "C" int sim_melc_create(uint32_t n_fft, uint32_t hop, const float* window, const float* fbank, uint32_t n_mels, uint32_t mode, float floor,
                               int has_opts, uint32_t center, uint32_t pad, uint32_t range, float range_width, float shift, float scale) {
    clx_mel_opts o;
    o.center = center; o.pad = pad; o.range = range; o.range_width = range_width; o.shift = shift; o.scale = scale;
    clx_mel_tables* t = new clx_mel_tables();
    const std::string why = clx_mel_build(n_fft, hop, window, fbank, n_mels, mode, floor, t, has_opts ? &o : nullptr);
    if (!why.empty()) { delete t; snprintf(sim_melc_err, sizeof sim_melc_err, "%s", why.c_str()); return -1; }
    sim_specs.push_back(t);
    return (int)sim_specs.size() - 1;
}

extern "C" void sim_melc_destroy(int h) {
    if (sim_spec(h)) { delete sim_specs[(size_t)h]; sim_specs[(size_t)h] = nullptr; }
}

// the spec's tables as they are: sizes first (out == NULL), then the words of basis, fbank and ends one after the other
extern "C" size_t sim_melc_table_words(int h, uint32_t* out) {
    const clx_mel_tables* t = sim_spec(h);
    if (!t) return 0;
    const size_t n = t->basis.size() + t->fbank.size() + t->ends.size();
    if (out) {
        memcpy(out, t->basis.data(), t->basis.size() * 4u);
        memcpy(out + t->basis.size(), t->fbank.data(), t->fbank.size() * 4u);
        memcpy(out + t->basis.size() + t->fbank.size(), t->ends.data(), t->ends.size() * 4u);
    }
    return n;
}

// clx_mel_windows with `audio` and `out` in host memory: CLX_OK, or CLX_API_ERROR with sim_melc_error() saying why.  vframes_out
// (may be NULL) receives valid_frames, wmax_out (may be NULL) the table's encoded maxima after the feature launch.
extern "C" int sim_melc_windows(int h, const void* audio, size_t n_windows, uint32_t window_len, const uint32_t* valid, uint32_t n_frames,
                                uint32_t layout, void* out, uint32_t* vframes_out, uint32_t* wmax_out) {
    const clx_mel_tables* t = sim_spec(h);
    uint32_t n_groups = 0, n_tiles = 0;
    const char* why = clx_mel_check(t, audio, n_windows, window_len, valid, n_frames, layout, out, &n_groups, &n_tiles);
    if (why) { snprintf(sim_melc_err, sizeof sim_melc_err, "%s", why); return CLX_API_ERROR; }
    if (n_groups == 0) return CLX_OK;
    const clx_mel_dev dev = clx_mel_args(*t, t->basis.data(), t->fbank.data(), t->ends.data());
    if (!clx_mel_is_c(*t)) {
        std::vector<uint32_t> vf(n_windows);
        clx_mel_fill(vf.data(), valid, n_windows, t->hop, n_frames);
        if (vframes_out) memcpy(vframes_out, vf.data(), n_windows * 4u);
        SIM_LAUNCH(clx_k_mel, n_windows * n_groups, clx_mel::kThreads, (const float*)audio, (const uint32_t*)vf.data(), dev, n_groups, window_len,
                   n_frames, layout, (float*)out);
        return CLX_OK;
    }
    std::vector<uint32_t> table(3u * n_windows);
    clx_mel_fill_c(table.data(), valid, n_windows, *t, window_len, n_frames);
    if (vframes_out) memcpy(vframes_out, table.data(), n_windows * 4u);
    SIM_LAUNCH(clx_k_mel_c, n_windows * n_groups, clx_mel::kThreads, (const float*)audio, table.data(), (uint32_t)n_windows, dev, clx_mel_cargs(*t),
               n_groups, window_len, n_frames, layout, (float*)out);
    if (wmax_out) memcpy(wmax_out, table.data() + 2u * n_windows, n_windows * 4u);
    if (n_tiles)
        SIM_LAUNCH(clx_k_mel_range, n_windows * n_tiles, clx_mel::kThreads, (float*)out, (const uint32_t*)(table.data() + 2u * n_windows),
                   (uint64_t)t->n_mels * n_frames, n_tiles, t->range_width, t->shift, t->scale);
    return CLX_OK;
}

// The batch (n_windows * window_len floats, given in `floats`) sits flush against an inaccessible page: the page follows its last
// float (at_end), or precedes its first.  A load on the wrong side of either end faults instead of reading a neighbour's bytes.
extern "C" int sim_melc_guarded(int h, const float* floats, size_t n_windows, uint32_t window_len, const uint32_t* valid, uint32_t n_frames,
                                uint32_t layout, int at_end, void* out) {
    const size_t len = n_windows * (size_t)window_len * 4u;
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), body = (len + pg - 1) / pg * pg + pg;
    uint8_t* m = (uint8_t*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == (uint8_t*)MAP_FAILED) return -1;
    mprotect(m, pg, PROT_NONE);
    mprotect(m + pg + body, pg, PROT_NONE);
    uint8_t* p = at_end ? m + pg + body - len : m + pg;
    memcpy(p, floats, len);
    const int st = sim_melc_windows(h, p, n_windows, window_len, valid, n_frames, layout, out, nullptr, nullptr);
    munmap(m, body + 2 * pg);
    return st;
}

// the encoding of a float that the kernel folds into wmax, and back
extern "C" uint32_t sim_melc_enc(float v) { return clx_mel::enc(v); }
extern "C" float sim_melc_dec(uint32_t e) { return clx_mel::dec(e); }
