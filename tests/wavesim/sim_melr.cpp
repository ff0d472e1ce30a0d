// TEST INFRASTRUCTURE: reflected mel specs (claxon_amd/csrc/clx_mel.hip, unmodified) under the wave simulator: clx_mel_build_reflected as
// clx_mel_create_reflected runs it (or clx_mel_build_framed / clx_mel_build_cepstral for the snipped sibling with the same tables), then
// clx_mel_check, the spec's table (clx_mel_fill_r, or clx_mel_fill with the sibling's rule) and clx_k_mel_fr / clx_k_mel_qr / clx_k_mel_f /
// clx_k_mel_q / clx_k_mel launched as clx_mel_windows launches them (clx_api.hip), with host buffers in place of device ones.  A spec is
// a small integer here; its tables live until sim_melr_destroy.
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

static char sim_melr_err[256];
static std::vector<clx_mel_tables*> sim_specs;

extern "C" const char* sim_melr_error(void) { return sim_melr_err; }
extern "C" uint32_t sim_melr_lds_bytes(void) { return clx_mel::kLdsBytes; }

static clx_mel_tables* sim_spec(int h) { return h >= 0 && (size_t)h < sim_specs.size() ? sim_specs[(size_t)h] : nullptr; }

// reflected != 0: clx_mel_create_reflected (has_opts == 0: opts == NULL; has_cep == 0: cep == NULL, an fbank spec).  reflected == 0: the
// snipped sibling, clx_mel_create_cepstral with has_cep, else clx_mel_create_framed.  The spec's number, or -1 with sim_melr_error()
// saying why.
extern "C" int sim_melr_create(int reflected, uint32_t n_fft, uint32_t win_length, uint32_t hop, const float* window, const float* fbank,
                               uint32_t n_bins, uint32_t n_mels, uint32_t mode, float floor, int has_opts, uint32_t remove_dc, uint32_t whole_frames,
                               float preemph, int has_cep, uint32_t n_ceps, const float* dct, const float* lifter, uint32_t energy,
                               float energy_scale, float energy_floor) {
    clx_mel_frame_opts o;
    o.remove_dc = remove_dc; o.whole_frames = whole_frames; o.preemph = preemph;
    clx_mel_cep_opts q;
    q.n_ceps = n_ceps; q.dct = dct; q.lifter = lifter; q.energy = energy; q.energy_scale = energy_scale; q.energy_floor = energy_floor;
    clx_mel_tables* t = new clx_mel_tables();
    const clx_mel_frame_opts* po = has_opts ? &o : nullptr;
    const std::string why =
        reflected ? clx_mel_build_reflected(n_fft, win_length, hop, window, fbank, n_bins, n_mels, mode, floor, t, po, has_cep ? &q : nullptr)
        : has_cep ? clx_mel_build_cepstral(n_fft, win_length, hop, window, fbank, n_bins, n_mels, mode, floor, t, po, &q)
                  : clx_mel_build_framed(n_fft, win_length, hop, window, fbank, n_bins, n_mels, mode, floor, t, nullptr, po);
    if (!why.empty()) { delete t; snprintf(sim_melr_err, sizeof sim_melr_err, "%s", why.c_str()); return -1; }
    sim_specs.push_back(t);
    return (int)sim_specs.size() - 1;
}

extern "C" void sim_melr_destroy(int h) {
    if (sim_spec(h)) { delete sim_specs[(size_t)h]; sim_specs[(size_t)h] = nullptr; }
}

// which kernel clx_mel_windows launches for the spec: 0 clx_k_mel, 1 clx_k_mel_f, 2 clx_k_mel_q, 3 clx_k_mel_fr, 4 clx_k_mel_qr (-1: no
// such spec)
extern "C" int sim_melr_kernel(int h) {
    const clx_mel_tables* t = sim_spec(h);
    if (!t) return -1;
    if (clx_mel_is_r(*t)) return clx_mel_is_q(*t) ? 4 : 3;
    return clx_mel_is_q(*t) ? 2 : clx_mel_is_f(*t) ? 1 : 0;
}

extern "C" uint32_t sim_melr_rows(int h) {
    const clx_mel_tables* t = sim_spec(h);
    return t ? clx_mel_rows(*t) : 0u;
}

extern "C" int32_t sim_melr_origin(int h) {
    const clx_mel_tables* t = sim_spec(h);
    return t ? clx_mel_origin(*t) : 0;
}

// the spec's basis, filterbank, row ends, dct and lifter as the builder left them (out == NULL: the count of words)
extern "C" size_t sim_melr_table_words(int h, uint32_t* out) {
    const clx_mel_tables* t = sim_spec(h);
    if (!t) return 0;
    const size_t nb = t->basis.size(), nf = t->fbank.size(), ne = t->ends.size(), nd = t->dct.size(), nl = t->lifter.size();
    if (out) {
        memcpy(out, t->basis.data(), nb * 4u);
        memcpy(out + nb, t->fbank.data(), nf * 4u);
        memcpy(out + nb + nf, t->ends.data(), ne * 4u);
        memcpy(out + nb + nf + ne, t->dct.data(), nd * 4u);
        memcpy(out + nb + nf + ne + nd, t->lifter.data(), nl * 4u);
    }
    return nb + nf + ne + nd + nl;
}

// clx_mel_windows with `audio` and `out` in host memory: CLX_OK, or CLX_API_ERROR with sim_melr_error() saying why.  vframes_out
// (may be NULL) receives valid_frames.
extern "C" int sim_melr_windows(int h, const void* audio, size_t n_windows, uint32_t window_len, const uint32_t* valid, uint32_t n_frames,
                                uint32_t layout, void* out, uint32_t* vframes_out) {
    const clx_mel_tables* t = sim_spec(h);
    uint32_t n_groups = 0;
    const char* why = clx_mel_check(t, audio, n_windows, window_len, valid, n_frames, layout, out, &n_groups);
    if (why) { snprintf(sim_melr_err, sizeof sim_melr_err, "%s", why); return CLX_API_ERROR; }
    if (n_groups == 0) return CLX_OK;
    const clx_mel_dev dev = clx_mel_args(*t, t->basis.data(), t->fbank.data(), t->ends.data());
    std::vector<uint32_t> tb(2u * n_windows);
    const bool is_r = clx_mel_is_r(*t);
    if (is_r) clx_mel_fill_r(tb.data(), valid, n_windows, *t, n_frames);
    else clx_mel_fill(tb.data(), valid, n_windows, t->hop, n_frames, 0u, clx_mel_whole(*t));
    if (vframes_out) memcpy(vframes_out, tb.data(), n_windows * 4u);
    if (is_r && clx_mel_is_q(*t))
        SIM_LAUNCH(clx_k_mel_qr, n_windows * n_groups, clx_mel::kThreads, (const float*)audio, (const uint32_t*)tb.data(), (uint32_t)n_windows, dev,
                   clx_mel_fargs(*t), clx_mel_qargs(*t, t->dct.data(), t->lifter.data()), clx_mel_origin(*t), n_groups, window_len, n_frames, layout,
                   (float*)out);
    else if (is_r)
        SIM_LAUNCH(clx_k_mel_fr, n_windows * n_groups, clx_mel::kThreads, (const float*)audio, (const uint32_t*)tb.data(), (uint32_t)n_windows, dev,
                   clx_mel_fargs(*t), clx_mel_origin(*t), n_groups, window_len, n_frames, layout, (float*)out);
    else if (clx_mel_is_q(*t))
        SIM_LAUNCH(clx_k_mel_q, n_windows * n_groups, clx_mel::kThreads, (const float*)audio, (const uint32_t*)tb.data(), dev, clx_mel_fargs(*t),
                   clx_mel_qargs(*t, t->dct.data(), t->lifter.data()), n_groups, window_len, n_frames, layout, (float*)out);
    else if (clx_mel_is_f(*t))
        SIM_LAUNCH(clx_k_mel_f, n_windows * n_groups, clx_mel::kThreads, (const float*)audio, (const uint32_t*)tb.data(), dev, clx_mel_fargs(*t),
                   n_groups, window_len, n_frames, layout, (float*)out);
    else
        SIM_LAUNCH(clx_k_mel, n_windows * n_groups, clx_mel::kThreads, (const float*)audio, (const uint32_t*)tb.data(), dev, n_groups, window_len,
                   n_frames, layout, (float*)out);
    return CLX_OK;
}

// The batch (n_windows * window_len floats, given in `floats`) sits flush against an inaccessible page: the page follows its last
// float (at_end), or precedes its first.  A load on the wrong side of either end faults instead of reading a neighbour's bytes.
extern "C" int sim_melr_guarded(int h, const float* floats, size_t n_windows, uint32_t window_len, const uint32_t* valid, uint32_t n_frames,
                                uint32_t layout, int at_end, void* out) {
    const size_t len = n_windows * (size_t)window_len * 4u;
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), body = (len + pg - 1) / pg * pg + pg;
    uint8_t* m = (uint8_t*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == (uint8_t*)MAP_FAILED) return -1;
    mprotect(m, pg, PROT_NONE);
    mprotect(m + pg + body, pg, PROT_NONE);
    uint8_t* p = at_end ? m + pg + body - len : m + pg;
    memcpy(p, floats, len);
    const int st = sim_melr_windows(h, p, n_windows, window_len, valid, n_frames, layout, out, nullptr);
    munmap(m, body + 2 * pg);
    return st;
}
