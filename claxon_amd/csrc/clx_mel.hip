// clx_mel.hip -- mel filterbank features of a dense mono batch [B, L] in one launch: framing, a windowed DFT as an fp32 GEMM against a
// basis table, the power, the band sums and the log, all in clx_k_mel.  claxon_hip.h (clx_mel_create, clx_mel_windows) has the
// definition; this is how it is computed.
//
// A block is one frame group of one window: kF = 32 consecutive frames, all J bins, all bands.  Its work is the GEMM
// [32 frames x N] . [N x 2J] done in passes of kBins = 256 bins and, inside a pass, in K-slices of kKS = 16 samples:
//   lane tile   4 bins (cos and sin: 8 basis columns) x 8 frames = 64 accumulators in registers.  Lane q of a wave owns bins
//               4q .. 4q+3 of the pass, wave w of the block owns frames 8w .. 8w+7 of the group.
//   basis       the table is stored padded for exactly this: row n holds, for every pass, 256 cos columns then 256 sin columns
//               (zeros past bin J and in the rows from N up to a multiple of 16), so a K-slice of a pass is 16 runs of 2 KiB that the
//               block copies with unmasked 16-byte loads into LDS.  A lane reads its 4 cos and 4 sin as two 16-byte LDS reads,
//               consecutive over the lanes of the wave.
//   audio       the K-slice of the group's frames is staged unfolded, xs[kk][f] = a[(f0 + f) * H + 16 s + kk] (lanes along kk: 64-byte
//               runs of the window), so a wave reads its 8 frames as two 16-byte LDS reads at one address.  Overlapping frames are
//               read from global memory again (N / H times over the K loop: 2.5 at 400 / 160) and not held as one span: the hop
//               has no upper bound, the span (kF - 1) * H + N has none either, and the audio is 1 / 2J of the operand traffic.
//   per k       a lane reads 32 bytes of basis and 32 bytes of audio from LDS for 64 fmaf: 1 multiply-add per LDS byte read (the
//               audio reads are one address per wave).  A basis float comes from the L2 once per 32 frames, not once per frame:
//               32 multiply-adds per byte of L2 traffic against 0.25 for one bin per lane and one frame per block.
//   prefetch    the next slice's 8 + 2 global loads are issued into registers before the current slice's 1024 fmaf per lane.
// After a pass's K loop the lanes square their tile into P[f][bin] in LDS (aliasing the staging area), and the block turns to the
// band sums: cell (band m, frame f) adds fb[m][j] * P[f][j] over the bins of the pass that lie between the row's first and last
// non-zero bin, j ascending, one fmaf each.  Cells are dealt to the lanes along the output row of the layout (frames for CT, bands
// for TC), so the stores are contiguous.  With more than one pass (J > 256: n_fft from 512 up) a cell's sum waits in its own place
// of the output between passes: the lane that stored it loads it again, nobody else touches it, and the last pass stores the result.
// A frame at or past valid_frames[k] is stored as +0.0 and costs nothing: its audio is not read, a wave whose 8 frames are all past
// it skips its fmaf, a block whose 32 are only stores zeros.  No float of the audio outside a live frame is read.
//
// LDS: 35 072 bytes, the staging area (16 x 512 basis floats + 16 x 36 audio floats; P, 32 x 260 floats, fits inside): four
// workgroups share a CU's 160 KiB.
//
// The kernel body is a template on the framing.  clx_k_mel is the plain instantiation: frame t starts at sample t * H, a dead frame is
// +0.0.  clx_k_mel_c serves a spec that is centred and/or range scaled (claxon_hip.h, clx_mel_create_ex) and differs
// in two places.  The audio staging address: the two loads per slice go through the index map p[t * H + n - P] (64-bit signed: t * H
// passes 2^32) -- reflected about 0 and L - 1, or not loaded at all outside [0, valid[k]) in zero mode; lim[k] is that upper end (L
// in reflect mode), so a tap is loaded only from [0, lim[k]) whatever the arguments are.  The last step: when ranged, a dead cell
// takes y0 = finish(0) and not +0.0, every cell of the last pass is folded into a running maximum in an order-preserving unsigned
// encoding of the float, the block reduces it (a wave by shuffles, the four waves through four words of the staging area) and one
// lane folds it into wmax[k] with one atomicMax: a maximum does not depend on the order, so the result is deterministic.
// clx_k_mel_range then clamps every cell of window k to wmax[k] - D and applies the affine, in place, behind it on the same stream:
// pure streaming, 16-byte accesses on the window's 16-byte grid, the ragged head and tail vectors float by float.
//
// clx_k_mel_f is the third instantiation: a framed spec that conditions each frame before the window (claxon_hip.h,
// clx_mel_create_framed), which is Kaldi's fbank.  Frames overlap, so the conditioning cannot be done once on the
// batch; it happens where a frame's slice is staged.  A prologue gives the block's live frames their sums: 8 lanes per frame, lane i
// of the 8 adds the frame's samples i, i + 8, ... in ascending order, three shuffles fold the 8 partial sums (xor 4, 2, 1), the
// mean is one correctly rounded division.  The 32 means cross the block through the first 32 words of the staging area, which
// nothing else uses yet, and stay in two registers of the lane that stages the frames they belong to: LDS stays 35 072 bytes.  The
// staged value is then y[n], from a[.. + n], a[.. + n - 1] (a[.. + n] itself at n = 0) and the frame's mean -- two more loads per
// lane and slice, of floats the neighbouring lane loads anyway, and three rounded operations.  A frame shorter than the transform,
// a bank that stops below the Nyquist bin and the whole-frame rule need no kernel of their own: the table has rows (slices) for
// win_length taps and passes for n_bins bins only, and clx_k_mel runs a framed spec that does not condition.
//
// clx_k_mel_q is the fourth: a cepstral spec (claxon_hip.h, clx_mel_create_cepstral), which is Kaldi's MFCC.  It frames
// and conditions as clx_k_mel_f does and differs in two places.  The prologue: with `energy` the 8 lanes of a frame make a second pass
// over it once the means have crossed the block, lane i adding the squares of d[i], d[i + 8], ... with one fmaf each; three shuffles
// fold them, and the frame's log energy waits in a register of the frame's first lane.  The last step: a lane keeps its finished
// log-mel cells -- at most 16, which is where the limit of 128 bands comes from -- in the registers the GEMM's accumulators have
// left; behind one barrier (P has been read) they go to Y[f][m] in the staging area, rows kYRow = 129 floats apart (1 mod 32: the 32
// frames a half-wave reads at one m lie in 32 banks), and the 32 log energies go behind them; behind a second barrier cell (i, f)
// of the n_ceps x 32 output cells, dealt to the lanes along the output row as the band cells are, runs dct[i][.] . Y[f][.] as one
// fmaf chain, m ascending, the dct row from global memory (it is a few KiB and stays in the caches), and applies the lifter or
// takes the energy.  One pass only: a cepstral spec has n_bins <= 256, for a cepstral output has no rows to park partial band sums in.
//
// clx_k_mel_fr and clx_k_mel_qr are the reflected forms of those two (claxon_hip.h, clx_mel_create_reflected), which is
// Kaldi's snip_edges=false: frame t's tap n is index t * H + H / 2 - Nw / 2 + n of the window's valid[k] samples continued on both sides
// by reflection with the edge sample repeated, as often as it takes.  They differ from clx_k_mel_f / clx_k_mel_q in the loads alone: the
// prologue's sums, the energy pass and the two staged loads with their two pre-emphasis neighbours.  A block whose live frames lie
// wholly inside [0, valid[k]) -- all but the first and last group or two of a window -- is told so once, before the pass loop, by a
// block-uniform flag, and addresses its taps directly as clx_k_mel_f does; an edge block sends each tap through clx_mel::rtap, where a
// tap inside [0, valid[k]) costs one 64-bit compare and a tap outside is folded with 32-bit arithmetic (the distance past the edge is
// at most win_length / 2 + 1).  The call's table is vframes[B] then vlen[B] = valid[k]; the origin H / 2 - Nw / 2 is a kernel argument.
//
// clx_mel_build / clx_mel_build_framed / clx_mel_build_cepstral / clx_mel_check / clx_mel_fill / clx_mel_fill_c are the host side (plain C++, shared with the
// wave simulator).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/claxon_hip.h"

// what the kernel needs of a spec (passed by value)
struct clx_mel_dev {
    const float* basis;      // [n_pad][n_pass][2][256]: cos then sin of the pass's 256 bins, zero padded
    const float* fbank;      // [n_mels][J]
    const uint32_t* ends;    // [n_mels][2]: a row's first non-zero bin and one past its last (equal: an all-zero row)
    uint32_t n_fft, hop, n_mels, n_bins, n_pass, n_slices, mode;   // (n_fft: the taps of a frame, win_length of a framed spec)
    float floor;
};

// what clx_k_mel_f needs on top of it (passed by value, uniform): whether the frame's mean is removed, and the pre-emphasis
// coefficient (0: none)
struct clx_mel_fdev {
    uint32_t remove_dc;
    float preemph;
};

// what clx_k_mel_q needs on top of both (passed by value, uniform): the DCT [n_ceps][n_mels], the lifter [n_ceps] (null: none), whether
// row 0 is the frame's log energy, the factor of the energy and the floor of it (0: none)
struct clx_mel_qdev {
    const float* dct;
    const float* lifter;
    uint32_t n_ceps, energy;
    float energy_scale, energy_floor;
};

// what clx_k_mel_c needs on top of it (passed by value): P = n_fft / 2 of a centred spec (else 0), zero = 1 for CLX_MEL_PAD_ZERO
// of a centred spec, range = 1 for a range-scaled one
struct clx_mel_cdev {
    uint32_t P, zero, range;
};

// a spec's tables on the host, as clx_mel_build leaves them
struct clx_mel_tables {
    uint32_t n_fft = 0, hop = 0, n_mels = 0, n_bins = 0, n_pass = 0, n_slices = 0, mode = 0;
    float floor = 0.f;
    uint32_t center = 0, pad = 0, range = 0;                 // clx_mel_opts (all zero: the plain spec)
    float range_width = 0.f, shift = 0.f, scale = 0.f;
    uint32_t win = 0, remove_dc = 0, whole = 0;              // clx_mel_create_framed: win_length (else n_fft) and clx_mel_frame_opts
    float preemph = 0.f;
    uint32_t n_ceps = 0, has_lifter = 0, energy = 0;         // clx_mel_create_cepstral: clx_mel_cep_opts (n_ceps == 0: not cepstral)
    float energy_scale = 1.f, energy_floor = 0.f;
    uint32_t reflect = 0;                                    // clx_mel_create_reflected
    std::vector<float> dct, lifter;
    std::vector<float> basis, fbank;
    std::vector<uint32_t> ends;
};

namespace clx_mel {

constexpr uint32_t kThreads = 256u, kF = 32u, kBins = 256u, kKS = 16u, kRow = 2u * kBins, kXsRow = 36u, kPRow = 260u, kMaxMels = 256u;
constexpr uint32_t kMaxCepMels = 128u, kYRow = kMaxCepMels + 1u, kQCells = kMaxCepMels * kF / kThreads;   // clx_k_mel_q: 16 cells a lane
constexpr uint32_t kStage = kKS * kRow + kKS * kXsRow;          // floats of the staging area (P aliases it)
constexpr uint32_t kLdsBytes = kStage * 4u;                     // 35 072
constexpr uint32_t kRangeVecs = 1024u;                          // 16-byte vectors of a clx_k_mel_range block: 4 per lane
static_assert(kF * kPRow <= kStage, "P fits in the staging area");
static_assert(kF * kYRow + kF <= kStage, "Y and the 32 log energies fit in the staging area");
static_assert(kThreads == 8u * kF, "the prologue of clx_k_mel_f sums a frame with 8 lanes");
static_assert(2u * kLdsBytes <= 160u * 1024u, "two workgroups share a CU's LDS");

// four floats moved as one 16-byte value (a vector type, so that a copy is a load and a store and never a memcpy through a stack slot)
#if defined(__clang__)
typedef float f4 __attribute__((ext_vector_type(4)));
#else
typedef float f4 __attribute__((vector_size(16)));
#endif

__device__ __forceinline__ float finish(uint32_t mode, float floor, float m) {
    if (mode == CLX_MEL_LN) return logf(fmaxf(m, floor));
    if (mode == CLX_MEL_LOG10) return log10f(fmaxf(m, floor));
    return m;
}

__device__ __forceinline__ uint32_t bits_of(float v) { uint32_t b; __builtin_memcpy(&b, &v, 4); return b; }
__device__ __forceinline__ float float_of(uint32_t b) { float v; __builtin_memcpy(&v, &b, 4); return v; }

// the order-preserving encoding of a float for an unsigned atomicMax (a < b as floats <=> enc(a) < enc(b) as unsigned; -0 < +0), and back
__device__ __forceinline__ uint32_t enc(float v) { const uint32_t b = bits_of(v); return b ^ ((b & 0x80000000u) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float dec(uint32_t e) { return float_of((e & 0x80000000u) ? e ^ 0x80000000u : ~e); }
constexpr uint32_t kEncNegInf = 0x007fffffu;                    // enc(-inf): what the host puts into wmax[k] before the launch

// a subtract, an add, a multiply and a divide that are each rounded once and never contracted (the wave simulator's host build is compiled
// without contraction)
#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
#else
inline float sub_rn(float a, float b) { return a - b; }
inline float add_rn(float a, float b) { return a + b; }
inline float mul_rn(float a, float b) { return a * b; }
inline float div_rn(float a, float b) { return a / b; }
#endif

// d - c * p with the product and the difference each rounded once.  __fmul_rn and __fsub_rn are a plain * and - to hipcc, and a
// product that feeds a difference is contracted into one fma unless the two operations themselves are compiled with contraction
// off, which is what this function is for (the steps of clx_k_mel_range are a sum feeding a product: nothing to contract).
__device__ __forceinline__ float msub_rn(float d, float c, float p) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float m = c * p;
    return d - m;
}

// The index map of a centred frame: tap i = t * H + n - P of the window p[] that continues a[0 .. L) on both sides -- by reflection
// about 0 and L - 1, or (zero) by zeros.  Only a float of [0, lim) is loaded: lim = L in reflect mode (clx_mel_check's conditions
// keep every reflected index inside it), lim = valid[k] in zero mode, where the window is zeros from there on anyway.
__device__ __forceinline__ float tap(const float* a, int64_t i, uint32_t L, uint32_t lim, uint32_t zero) {
    if (!zero) { if (i < 0) i = -i; else if (i >= (int64_t)L) i = 2 * ((int64_t)L - 1) - i; }
    return (uint64_t)i < (uint64_t)lim ? a[i] : 0.f;
}

// The index map of a reflected frame (clx_k_mel_fr, clx_k_mel_qr): sample r(i) of a window of V >= 1 valid samples, r being Kaldi's
// loop -- while i is outside [0, V): i = -i - 1 below 0, i = 2 V - 1 - i from V up.  A tap inside costs the compare.  Outside, e is
// the distance past the edge (0: the edge sample's first repeat); the live frames of a window keep it to win_length / 2 + 1 at most,
// so it is taken as 32 bits: e < V is one reflection, else e mod 2 V says how far into which image of the window the tap lies (2 V
// fits 32 bits there, V being at most e).  Whatever i is, the float loaded is one of a[0 .. V).
__device__ __forceinline__ float rtap(const float* a, int64_t i, uint32_t V) {
    if ((uint64_t)i >= (uint64_t)V) {
        const bool below = i < 0;
        uint32_t e = (uint32_t)(below ? -i - 1 : i - (int64_t)V);
        bool flip = !below;                                    // (flip: counted down from V - 1; else up from 0)
        if (e >= V) {
            e %= 2u * V;
            if (e >= V) { e -= V; flip = !flip; }
        }
        i = flip ? (int64_t)(V - 1u - e) : (int64_t)e;
    }
    return a[i];
}

// cell c of the block's n_mels x kF cells: lanes run along the layout's output row
__device__ __forceinline__ void cell(uint32_t c, uint32_t layout, uint32_t n_mels, uint32_t* m, uint32_t* f) {
    if (layout == CLX_WINDOW_CT) { *f = c % kF; *m = c / kF; }
    else { *m = c % n_mels; *f = c / n_mels; }
}

}  // namespace clx_mel

// Block b: frame group b % n_groups of window b / n_groups (clx_mel_check gives n_groups).  `audio` is [B, L], vframes[k] =
// valid_frames[k] <= n_frames, `out` is [B, n_mels, n_frames] (CLX_WINDOW_CT) or [B, n_frames, n_mels] (CLX_WINDOW_TC).  kC: the
// centred and/or ranged form (X, lim[k] and wmax[k] are used by it alone).  kFr: the conditioning form (F is used by it alone).
// kQ (with kFr): the cepstral form (Q is used by it alone); `out` has n_ceps in place of n_mels.  kR (with kFr): the reflected form
// (lim[k] = valid[k] and org = H / 2 - Nw / 2 are used by it alone).
namespace clx_mel {
template <bool kC, bool kFr, bool kQ, bool kR = false>
__device__ __forceinline__ void body(const float* __restrict__ audio, const uint32_t* __restrict__ vframes,
                                     const clx_mel_dev S, const clx_mel_cdev X, const clx_mel_fdev F, const clx_mel_qdev Q, const uint32_t* __restrict__ lim,
                                     uint32_t* wmax, uint32_t n_groups, uint32_t L, uint32_t n_frames, uint32_t layout, float* __restrict__ out,
                                     int32_t org = 0) {
    __shared__ __attribute__((aligned(16))) float s_stage[kStage];
    const uint32_t tid = threadIdx.x, k = blockIdx.x / n_groups, f0 = (blockIdx.x - k * n_groups) * kF;
    const uint32_t vf = vframes[k];
    const uint32_t nf_out = n_frames - f0 < kF ? n_frames - f0 : kF;                 // the group's frames that exist
    const uint32_t nf_live = vf > f0 ? (vf - f0 < kF ? vf - f0 : kF) : 0u;           // ... and those that are computed (<= nf_out)
    const uint32_t n_out = kQ ? Q.n_ceps : S.n_mels;           // the rows of the output
    const uint32_t cells = S.n_mels * kF;
    float* const o = out + (uint64_t)k * n_out * n_frames;
    float y0 = 0.f;                                            // a dead cell: +0.0, or the silence value of a ranged spec
    if constexpr (kC) if (X.range) y0 = finish(S.mode, S.floor, 0.f);
    if (nf_live == 0u) {
        for (uint32_t c = tid; c < n_out * kF; c += kThreads) {
            uint32_t m, f;
            cell(c, layout, n_out, &m, &f);
            if (f < nf_out) o[layout == CLX_WINDOW_CT ? (uint64_t)m * n_frames + f0 + f : (uint64_t)(f0 + f) * n_out + m] = kC ? y0 : 0.f;
        }
        if constexpr (kC) if (X.range && tid == 0u) atomicMax(wmax + k, enc(y0));      // (every cell of the block is y0)
        return;
    }
    const float* const a = audio + (uint64_t)k * L;
    float* const bs = s_stage;
    float* const xs = s_stage + kKS * kRow;
    const uint32_t q = tid & 63u, w = tid >> 6;
    const bool wave_live = 8u * w < nf_live;
    // staging duties: basis rows (tid >> 7) + 2 i of the slice, 16 bytes at float 4 * (tid & 127) of the row; audio kk = tid & 15 of
    // frames (tid >> 4) and (tid >> 4) + 16
    const uint32_t b_row = tid >> 7, b_col = 4u * (tid & 127u), x_kk = tid & 15u, x_f = tid >> 4;
    const uint64_t row_stride = (uint64_t)S.n_pass * kRow;
    // kC: the taps of this lane's two frames at n = x_kk, and the end of what may be loaded
    int64_t i0 = 0, i1 = 0;
    uint32_t lm = 0u, emax = 0u;                               // (emax: the running maximum of the lane's cells, encoded; 0 is below all)
    if constexpr (kC) {
        i0 = (int64_t)((uint64_t)(f0 + x_f) * S.hop) + (int64_t)x_kk - (int64_t)X.P;
        i1 = i0 + (int64_t)(16ull * S.hop);
        lm = lim[k];
    }
    // kFr: the means of this lane's two frames (0 when the mean stays), and the frames' first samples
    float mu0 = 0.f, mu1 = 0.f;
    const float* a0 = a;
    const float* a1 = a;
    // kR: the window's valid samples, the index of the block's first tap, whether every tap of the block's live frames lies inside
    // [0, V) (uniform over the block: such a block addresses its taps as clx_k_mel_f does), and the first taps of this lane's two frames
    uint32_t V = 0u;
    int64_t g0 = 0, b0 = 0, b1 = 0;
    bool direct = false;
    if constexpr (kR) {
        V = lim[k];
        g0 = (int64_t)((uint64_t)f0 * S.hop) + (int64_t)org;
        direct = g0 >= 0 && g0 + (int64_t)((uint64_t)(nf_live - 1u) * S.hop) + (int64_t)S.n_fft <= (int64_t)V;
        b0 = g0 + (int64_t)((uint64_t)x_f * S.hop);
        b1 = b0 + (int64_t)(16ull * S.hop);
    }
    if constexpr (kFr) {
        if constexpr (!kR) {
            a0 = a + (uint64_t)(f0 + x_f) * S.hop;
            a1 = a + (uint64_t)(f0 + x_f + 16u) * S.hop;
        }
        if (F.remove_dc) {                                     // (uniform over the block)
            const uint32_t sf = tid >> 3;                      // lanes 8 sf .. 8 sf + 7 sum frame sf
            float sum = 0.f;
            if (sf < nf_live) {
                if constexpr (kR) {
                    const int64_t b = g0 + (int64_t)((uint64_t)sf * S.hop);
                    if (direct) for (uint32_t n = tid & 7u; n < S.n_fft; n += 8u) sum = add_rn(sum, a[b + n]);
                    else for (uint32_t n = tid & 7u; n < S.n_fft; n += 8u) sum = add_rn(sum, rtap(a, b + n, V));
                } else {
                    const float* const fr = a + (uint64_t)(f0 + sf) * S.hop;
                    for (uint32_t n = tid & 7u; n < S.n_fft; n += 8u) sum = add_rn(sum, fr[n]);
                }
            }
            sum = add_rn(sum, __shfl_xor(sum, 4));
            sum = add_rn(sum, __shfl_xor(sum, 2));
            sum = add_rn(sum, __shfl_xor(sum, 1));
            if ((tid & 7u) == 0u) s_stage[sf] = div_rn(sum, (float)S.n_fft);
            __syncthreads();
            mu0 = s_stage[x_f];
            mu1 = s_stage[x_f + 16u];                          // (read before the first round's barrier, behind which the staging begins)
        }
    }
    // kQ: the log energy of frame tid >> 3 (every one of the frame's 8 lanes has it; lane 0 of them hands it on in the last step)
    float le = 0.f;
    if constexpr (kQ) {
        if (Q.energy) {                                        // (uniform over the block)
            const uint32_t sf = tid >> 3;
            float e = 0.f;
            if (sf < nf_live) {
                const float mu = F.remove_dc ? s_stage[sf] : 0.f;   // (as mu0 and mu1: read before the first round's barrier)
                if constexpr (kR) {
                    const int64_t b = g0 + (int64_t)((uint64_t)sf * S.hop);
                    for (uint32_t n = tid & 7u; n < S.n_fft; n += 8u) {
                        const float x = direct ? a[b + n] : rtap(a, b + n, V);
                        const float d = F.remove_dc ? sub_rn(x, mu) : x;
                        e = fmaf(d, d, e);
                    }
                } else {
                    const float* const fr = a + (uint64_t)(f0 + sf) * S.hop;
                    for (uint32_t n = tid & 7u; n < S.n_fft; n += 8u) {
                        const float d = F.remove_dc ? sub_rn(fr[n], mu) : fr[n];
                        e = fmaf(d, d, e);
                    }
                }
            }
            e = add_rn(e, __shfl_xor(e, 4));
            e = add_rn(e, __shfl_xor(e, 2));
            e = add_rn(e, __shfl_xor(e, 1));
            le = logf(fmaxf(mul_rn(e, Q.energy_scale), 1.1920928955078125e-07f));   // (FLT_EPSILON)
            if (Q.energy_floor > 0.f) { const float lf = logf(Q.energy_floor); if (le < lf) le = lf; }
        }
    }

    for (uint32_t p = 0; p < S.n_pass; ++p) {
        const bool lane_live = wave_live && p * kBins + 4u * q < S.n_bins;
        float re[4][8], im[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int f = 0; f < 8; ++f) { re[i][f] = 0.f; im[i][f] = 0.f; }
        const float* const bp = S.basis + (uint64_t)p * kRow + b_col;
        // round s: slice s goes from global memory into registers, slice s - 1 (in LDS) is computed, then the registers go to LDS
        for (uint32_t s = 0; s <= S.n_slices; ++s) {
            f4 pb0, pb1, pb2, pb3, pb4, pb5, pb6, pb7;
            float px0 = 0.f, px1 = 0.f;
            float pv0 = 0.f, pv1 = 0.f;                        // kFr with pre-emphasis: the samples in front of px0 and px1
            if (s < S.n_slices) {
                const float* const r = bp + ((uint64_t)s * kKS + b_row) * row_stride;
                pb0 = *reinterpret_cast<const f4*>(r);
                pb1 = *reinterpret_cast<const f4*>(r + 2u * row_stride);
                pb2 = *reinterpret_cast<const f4*>(r + 4u * row_stride);
                pb3 = *reinterpret_cast<const f4*>(r + 6u * row_stride);
                pb4 = *reinterpret_cast<const f4*>(r + 8u * row_stride);
                pb5 = *reinterpret_cast<const f4*>(r + 10u * row_stride);
                pb6 = *reinterpret_cast<const f4*>(r + 12u * row_stride);
                pb7 = *reinterpret_cast<const f4*>(r + 14u * row_stride);
                const uint32_t n = s * kKS + x_kk;
                if (n < S.n_fft) {
                    if constexpr (kC) {
                        if (x_f < nf_live) px0 = tap(a, i0 + (int64_t)(s * kKS), L, lm, X.zero);
                        if (x_f + 16u < nf_live) px1 = tap(a, i1 + (int64_t)(s * kKS), L, lm, X.zero);
                    } else if constexpr (kR) {
                        const uint32_t nb = n ? n - 1u : 0u;   // (the first tap refers to the frame's own first tap, mapped as it is)
                        if (direct) {
                            if (x_f < nf_live) { px0 = a[b0 + n]; if (F.preemph > 0.f) pv0 = a[b0 + nb]; }
                            if (x_f + 16u < nf_live) { px1 = a[b1 + n]; if (F.preemph > 0.f) pv1 = a[b1 + nb]; }
                        } else {
                            if (x_f < nf_live) { px0 = rtap(a, b0 + n, V); if (F.preemph > 0.f) pv0 = rtap(a, b0 + nb, V); }
                            if (x_f + 16u < nf_live) { px1 = rtap(a, b1 + n, V); if (F.preemph > 0.f) pv1 = rtap(a, b1 + nb, V); }
                        }
                    } else if constexpr (kFr) {
                        const uint32_t nb = n ? n - 1u : 0u;   // (the first tap refers to the frame's own first sample)
                        if (x_f < nf_live) { px0 = a0[n]; if (F.preemph > 0.f) pv0 = a0[nb]; }
                        if (x_f + 16u < nf_live) { px1 = a1[n]; if (F.preemph > 0.f) pv1 = a1[nb]; }
                    } else {
                        if (x_f < nf_live) px0 = a[(uint64_t)(f0 + x_f) * S.hop + n];
                        if (x_f + 16u < nf_live) px1 = a[(uint64_t)(f0 + x_f + 16u) * S.hop + n];
                    }
                }
            }
            if (s > 0u && lane_live) {
#pragma unroll 4
                for (uint32_t kk = 0; kk < kKS; ++kk) {
                    const f4 c4 = *reinterpret_cast<const f4*>(bs + kk * kRow + 4u * q);
                    const f4 s4 = *reinterpret_cast<const f4*>(bs + kk * kRow + kBins + 4u * q);
                    const f4 x0 = *reinterpret_cast<const f4*>(xs + kk * kXsRow + 8u * w);
                    const f4 x1 = *reinterpret_cast<const f4*>(xs + kk * kXsRow + 8u * w + 4u);
                    const float cv[4] = { c4[0], c4[1], c4[2], c4[3] }, sv[4] = { s4[0], s4[1], s4[2], s4[3] };
                    const float xv[8] = { x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3] };
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int f = 0; f < 8; ++f) {
                            re[i][f] = fmaf(xv[f], cv[i], re[i][f]);
                            im[i][f] = fmaf(xv[f], sv[i], im[i][f]);
                        }
                }
            }
            __syncthreads();                                   // (slice s - 1, or the pass before's P, has been read)
            if (s < S.n_slices) {
                float* const d = bs + b_row * kRow + b_col;
                *reinterpret_cast<f4*>(d) = pb0;
                *reinterpret_cast<f4*>(d + 2u * kRow) = pb1;
                *reinterpret_cast<f4*>(d + 4u * kRow) = pb2;
                *reinterpret_cast<f4*>(d + 6u * kRow) = pb3;
                *reinterpret_cast<f4*>(d + 8u * kRow) = pb4;
                *reinterpret_cast<f4*>(d + 10u * kRow) = pb5;
                *reinterpret_cast<f4*>(d + 12u * kRow) = pb6;
                *reinterpret_cast<f4*>(d + 14u * kRow) = pb7;
                if constexpr (kFr) {                           // d = x - mu, y = d - c * d', each step rounded once (a dead frame: 0)
                    if (s * kKS + x_kk < S.n_fft) {            // (a tap past the frame stays +0.0)
                        if (F.remove_dc) { px0 = sub_rn(px0, mu0); px1 = sub_rn(px1, mu1); }
                        if (F.preemph > 0.f) {
                            if (F.remove_dc) { pv0 = sub_rn(pv0, mu0); pv1 = sub_rn(pv1, mu1); }
                            px0 = msub_rn(px0, F.preemph, pv0);
                            px1 = msub_rn(px1, F.preemph, pv1);
                        }
                    }
                }
                xs[x_kk * kXsRow + x_f] = px0;
                xs[x_kk * kXsRow + x_f + 16u] = px1;
            }
            __syncthreads();                                   // (after the last round: P may take the staging area's place)
        }
        float* const P = s_stage;
        if (lane_live) {
#pragma unroll
            for (int f = 0; f < 8; ++f) {
                f4 v;
                v[0] = fmaf(re[0][f], re[0][f], im[0][f] * im[0][f]);
                v[1] = fmaf(re[1][f], re[1][f], im[1][f] * im[1][f]);
                v[2] = fmaf(re[2][f], re[2][f], im[2][f] * im[2][f]);
                v[3] = fmaf(re[3][f], re[3][f], im[3][f] * im[3][f]);
                *reinterpret_cast<f4*>(P + (8u * w + f) * kPRow + 4u * q) = v;
            }
        }
        __syncthreads();
        if constexpr (kQ) {                                    // (one pass: n_bins <= 256)
            float y[kQCells];
#pragma unroll
            for (uint32_t r = 0; r < kQCells; ++r) {
                y[r] = 0.f;
                const uint32_t c = tid + r * kThreads;
                uint32_t m, f;
                cell(c, layout, S.n_mels, &m, &f);
                if (c < cells && f < nf_live) {
                    float acc = 0.f;
                    const uint32_t e0 = S.ends[2u * m], e1 = S.ends[2u * m + 1u];
                    const float* const fb = S.fbank + (uint64_t)m * S.n_bins;
                    const float* const pr = P + f * kPRow;
                    for (uint32_t j = e0; j < e1; ++j) acc = fmaf(fb[j], pr[j], acc);
                    y[r] = finish(S.mode, S.floor, acc);
                }
            }
            __syncthreads();                                   // (P has been read)
            float* const Y = s_stage;
#pragma unroll
            for (uint32_t r = 0; r < kQCells; ++r) {
                const uint32_t c = tid + r * kThreads;
                uint32_t m, f;
                cell(c, layout, S.n_mels, &m, &f);
                if (c < cells) Y[f * kYRow + m] = y[r];
            }
            if (Q.energy && (tid & 7u) == 0u) Y[kF * kYRow + (tid >> 3)] = le;
            __syncthreads();
            for (uint32_t c = tid; c < Q.n_ceps * kF; c += kThreads) {
                uint32_t i, f;
                cell(c, layout, Q.n_ceps, &i, &f);
                if (f >= nf_out) continue;
                float* const at = o + (layout == CLX_WINDOW_CT ? (uint64_t)i * n_frames + f0 + f : (uint64_t)(f0 + f) * Q.n_ceps + i);
                if (f >= nf_live) { *at = 0.f; continue; }
                if (Q.energy && i == 0u) { *at = Y[kF * kYRow + f]; continue; }
                const float* const dr = Q.dct + (uint64_t)i * S.n_mels;
                const float* const yr = Y + f * kYRow;
                float acc = 0.f;
                for (uint32_t m = 0; m < S.n_mels; ++m) acc = fmaf(dr[m], yr[m], acc);
                *at = Q.lifter ? mul_rn(acc, Q.lifter[i]) : acc;
            }
            break;
        }
        const uint32_t j0 = p * kBins, j1 = j0 + kBins;
        const bool last = p + 1u == S.n_pass;
        for (uint32_t c = tid; c < cells; c += kThreads) {
            uint32_t m, f;
            cell(c, layout, S.n_mels, &m, &f);
            if (f >= nf_out) continue;
            float* const at = o + (layout == CLX_WINDOW_CT ? (uint64_t)m * n_frames + f0 + f : (uint64_t)(f0 + f) * S.n_mels + m);
            if (f >= nf_live) {
                if (last) {
                    *at = kC ? y0 : 0.f;
                    if constexpr (kC) { const uint32_t e = enc(y0); emax = e > emax ? e : emax; }
                }
                continue;
            }
            float acc = p ? *at : 0.f;                         // (this lane's own store of the pass before)
            const uint32_t e0 = S.ends[2u * m], e1 = S.ends[2u * m + 1u];
            const uint32_t lo = e0 > j0 ? e0 : j0, hi = e1 < j1 ? e1 : j1;
            const float* const fb = S.fbank + (uint64_t)m * S.n_bins;
            const float* const pr = P + f * kPRow;
            for (uint32_t j = lo; j < hi; ++j) acc = fmaf(fb[j], pr[j - j0], acc);
            if constexpr (kC) {
                if (last) {
                    const float y = finish(S.mode, S.floor, acc);
                    const uint32_t e = enc(y);
                    emax = e > emax ? e : emax;
                    *at = y;
                } else *at = acc;
            } else *at = last ? finish(S.mode, S.floor, acc) : acc;
        }
    }
    if constexpr (kC) {
        if (X.range) {                                         // (uniform over the block: every lane is still here)
            for (int d = 32; d > 0; d >>= 1) { const uint32_t e = __shfl_xor(emax, d); emax = e > emax ? e : emax; }
            uint32_t* const red = reinterpret_cast<uint32_t*>(s_stage);
            __syncthreads();                                   // (the last pass's P has been read)
            if (q == 0u) red[w] = emax;
            __syncthreads();
            if (tid == 0u) {
                const uint32_t e01 = red[0] > red[1] ? red[0] : red[1], e23 = red[2] > red[3] ? red[2] : red[3];
                atomicMax(wmax + k, e01 > e23 ? e01 : e23);
            }
        }
    }
}
}  // namespace clx_mel

extern "C" __global__ __launch_bounds__(256) void clx_k_mel(const float* __restrict__ audio, const uint32_t* __restrict__ vframes, clx_mel_dev S,
                                                            uint32_t n_groups, uint32_t L, uint32_t n_frames, uint32_t layout,
                                                            float* __restrict__ out) {
    clx_mel::body<false, false, false>(audio, vframes, S, clx_mel_cdev(), clx_mel_fdev(), clx_mel_qdev(), nullptr, nullptr, n_groups, L, n_frames, layout, out);
}

// The conditioning form of a framed spec (remove_dc and / or preemph > 0); otherwise clx_k_mel's arguments.
extern "C" __global__ __launch_bounds__(256) void clx_k_mel_f(const float* __restrict__ audio, const uint32_t* __restrict__ vframes, clx_mel_dev S,
                                                              clx_mel_fdev F, uint32_t n_groups, uint32_t L, uint32_t n_frames, uint32_t layout,
                                                              float* __restrict__ out) {
    clx_mel::body<false, true, false>(audio, vframes, S, clx_mel_cdev(), F, clx_mel_qdev(), nullptr, nullptr, n_groups, L, n_frames, layout, out);
}

// The cepstral form (every cepstral spec, whether it conditions or not): clx_k_mel_f's arguments and Q; `out` is [B, n_ceps, n_frames]
// or [B, n_frames, n_ceps].
extern "C" __global__ __launch_bounds__(256) void clx_k_mel_q(const float* __restrict__ audio, const uint32_t* __restrict__ vframes, clx_mel_dev S,
                                                              clx_mel_fdev F, clx_mel_qdev Q, uint32_t n_groups, uint32_t L, uint32_t n_frames,
                                                              uint32_t layout, float* __restrict__ out) {
    clx_mel::body<false, true, true>(audio, vframes, S, clx_mel_cdev(), F, Q, nullptr, nullptr, n_groups, L, n_frames, layout, out);
}

// The reflected forms of the two (every reflected spec runs one of them, whether it conditions or not).  `table` is the call's device
// table: vframes[B], then vlen[B] = valid[k], the samples a tap is reflected about and loaded from; org = hop / 2 - win_length / 2.
extern "C" __global__ __launch_bounds__(256) void clx_k_mel_fr(const float* __restrict__ audio, const uint32_t* __restrict__ table, uint32_t n_windows,
                                                               clx_mel_dev S, clx_mel_fdev F, int32_t org, uint32_t n_groups, uint32_t L, uint32_t n_frames,
                                                               uint32_t layout, float* __restrict__ out) {
    clx_mel::body<false, true, false, true>(audio, table, S, clx_mel_cdev(), F, clx_mel_qdev(), table + n_windows, nullptr, n_groups, L, n_frames, layout, out, org);
}

extern "C" __global__ __launch_bounds__(256) void clx_k_mel_qr(const float* __restrict__ audio, const uint32_t* __restrict__ table, uint32_t n_windows,
                                                               clx_mel_dev S, clx_mel_fdev F, clx_mel_qdev Q, int32_t org, uint32_t n_groups, uint32_t L,
                                                               uint32_t n_frames, uint32_t layout, float* __restrict__ out) {
    clx_mel::body<false, true, true, true>(audio, table, S, clx_mel_cdev(), F, Q, table + n_windows, nullptr, n_groups, L, n_frames, layout, out, org);
}

// The centred and/or ranged form.  `table` is the call's device table: vframes[B], then lim[B] (the end of what a tap may load of
// window k: valid[k] in zero mode, L otherwise), then wmax[B] (ranged: enc(-inf) on entry, the encoded maximum of window k's cells
// when the launch has finished).
extern "C" __global__ __launch_bounds__(256) void clx_k_mel_c(const float* __restrict__ audio, uint32_t* table, uint32_t n_windows, clx_mel_dev S,
                                                              clx_mel_cdev X, uint32_t n_groups, uint32_t L, uint32_t n_frames, uint32_t layout,
                                                              float* __restrict__ out) {
    clx_mel::body<true, false, false>(audio, table, S, X, clx_mel_fdev(), clx_mel_qdev(), table + n_windows, table + 2u * (uint64_t)n_windows, n_groups, L, n_frames, layout, out);
}

// The range step, in place: out[k][c] = fl32(fl32(max(out[k][c], fl32(max_k - D)) + shift) * scale) for the `cells` cells of window
// k, max_k = dec(wmax[k]).  Block b: tile b % n_tiles of window b / n_tiles; a tile is kRangeVecs vectors of the window's 16-byte
// grid (vector v holds the window's floats 4 v - head .. + 3, head = the floats of its first vector that lie in front of it), a
// whole vector is one 16-byte load and store, a ragged one (the window's head and tail) goes float by float.
extern "C" __global__ __launch_bounds__(256) void clx_k_mel_range(float* out, const uint32_t* __restrict__ wmax, uint64_t cells, uint32_t n_tiles,
                                                                  float D, float shift, float scale) {
    using namespace clx_mel;
    const uint32_t k = blockIdx.x / n_tiles, t = blockIdx.x - k * n_tiles;
    float* const o = out + (uint64_t)k * cells;
    const uint32_t head = (uint32_t)(((uintptr_t)o >> 2) & 3u);
    const uint64_t vectors = (cells + head + 3u) >> 2;
    const float lo = sub_rn(dec(wmax[k]), D);
    for (uint32_t i = 0; i < kRangeVecs / kThreads; ++i) {
        const uint64_t v = (uint64_t)t * kRangeVecs + i * kThreads + threadIdx.x;
        if (v >= vectors) break;
        const int64_t e0 = (int64_t)(v * 4u) - (int64_t)head;
        float* const p = o + e0;                               // 16-byte aligned
        if (e0 >= 0 && (uint64_t)e0 + 4u <= cells) {
            f4 x = *reinterpret_cast<const f4*>(p);
            x[0] = mul_rn(add_rn(fmaxf(x[0], lo), shift), scale);
            x[1] = mul_rn(add_rn(fmaxf(x[1], lo), shift), scale);
            x[2] = mul_rn(add_rn(fmaxf(x[2], lo), shift), scale);
            x[3] = mul_rn(add_rn(fmaxf(x[3], lo), shift), scale);
            *reinterpret_cast<f4*>(p) = x;
        } else {
            for (int j = 0; j < 4; ++j)
                if (e0 + j >= 0 && (uint64_t)(e0 + j) < cells) p[j] = mul_rn(add_rn(fmaxf(p[j], lo), shift), scale);
        }
    }
}

// The host side of clx_mel_create: checks the spec's arguments (empty: fine, else the text for clx_last_error) and builds its
// tables: the basis in double, rounded once, in the padded layout the kernel stages from; a copy of the filterbank; each row's ends.
// `opts` (clx_mel_create_ex; nullptr: all zero) is checked and copied into the tables.  The framed form (clx_mel_create_framed) has a
// window of win_length <= n_fft taps -- the table gets rows for those taps only, the angle stays over n_fft -- and a filterbank over
// the first n_bins bins -- the table gets passes for those only; `fopts` (nullptr: all zero) is checked and copied likewise.  With
// win_length == n_fft and n_bins == n_fft / 2 + 1 the tables are clx_mel_create's.
inline std::string clx_mel_build_framed(uint32_t n_fft, uint32_t win_length, uint32_t hop, const float* window, const float* fbank, uint32_t n_bins,
                                        uint32_t n_mels, uint32_t mode, float floor, clx_mel_tables* t, const clx_mel_opts* opts,
                                        const clx_mel_frame_opts* fopts) {
    if (n_fft < 2u || n_fft > 2048u) return "clx_mel_create: n_fft must be 2..2048";
    if (win_length < 1u || win_length > n_fft) return "clx_mel_create_framed: win_length must be 1..n_fft";
    if (n_bins < 1u || n_bins > n_fft / 2u + 1u) return "clx_mel_create_framed: n_bins must be 1..n_fft / 2 + 1";
    if (hop < 1u) return "clx_mel_create: hop must be at least 1";
    if (n_mels < 1u || n_mels > clx_mel::kMaxMels) return "clx_mel_create: n_mels must be 1..256";
    if (mode != CLX_MEL_POWER && mode != CLX_MEL_LN && mode != CLX_MEL_LOG10) return "clx_mel_create: mode must be CLX_MEL_POWER, CLX_MEL_LN or CLX_MEL_LOG10";
    if (mode != CLX_MEL_POWER && !(floor > 0.f)) return "clx_mel_create: floor must be greater than 0 in a log mode";
    if (!window || !fbank || !t) return "clx_mel_create: null argument";
    if (opts) {
        if (opts->center > 1u) return "clx_mel_create_ex: center must be 0 or 1";
        if (opts->range > 1u) return "clx_mel_create_ex: range must be 0 or 1";
        if (opts->pad != CLX_MEL_PAD_REFLECT && opts->pad != CLX_MEL_PAD_ZERO) return "clx_mel_create_ex: pad must be CLX_MEL_PAD_REFLECT or CLX_MEL_PAD_ZERO";
        if (opts->range) {
            if (mode == CLX_MEL_POWER) return "clx_mel_create_ex: range scaling needs a log mode";
            if (!std::isfinite(opts->range_width) || !(opts->range_width > 0.f)) return "clx_mel_create_ex: range_width must be finite and greater than 0";
            if (!std::isfinite(opts->shift)) return "clx_mel_create_ex: shift must be finite";
            if (!std::isfinite(opts->scale) || opts->scale == 0.f) return "clx_mel_create_ex: scale must be finite and not zero";
        }
        t->center = opts->center; t->pad = opts->pad; t->range = opts->range;
        t->range_width = opts->range_width; t->shift = opts->shift; t->scale = opts->scale;
    }
    if (fopts) {
        if (fopts->remove_dc > 1u) return "clx_mel_create_framed: remove_dc must be 0 or 1";
        if (fopts->whole_frames > 1u) return "clx_mel_create_framed: whole_frames must be 0 or 1";
        if (!std::isfinite(fopts->preemph) || !(fopts->preemph >= 0.f) || !(fopts->preemph <= 1.f)) return "clx_mel_create_framed: preemph must be finite and in 0..1";
        t->remove_dc = fopts->remove_dc; t->whole = fopts->whole_frames; t->preemph = fopts->preemph > 0.f ? fopts->preemph : 0.f;
    }
    using namespace clx_mel;
    const uint32_t N = n_fft, Nw = win_length, J = n_bins;
    t->n_fft = N; t->win = Nw; t->hop = hop; t->n_mels = n_mels; t->n_bins = J; t->mode = mode; t->floor = floor;
    t->n_pass = (J + kBins - 1u) / kBins;
    t->n_slices = (Nw + kKS - 1u) / kKS;
    const size_t row = (size_t)t->n_pass * kRow;
    t->basis.assign((size_t)t->n_slices * kKS * row, 0.f);
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (uint32_t n = 0; n < Nw; ++n)
        for (uint32_t j = 0; j < J; ++j) {
            const double ang = two_pi * (double)(((uint64_t)j * n) % N) / (double)N;     // (in this order: 2 pi k, then / N)
            float* const at = t->basis.data() + (size_t)n * row + (size_t)(j / kBins) * kRow + j % kBins;
            at[0] = (float)((double)window[n] * cos(ang));
            at[kBins] = (float)(-(double)window[n] * sin(ang));
        }
    t->fbank.assign(fbank, fbank + (size_t)n_mels * J);
    t->ends.assign(2u * (size_t)n_mels, 0u);
    for (uint32_t m = 0; m < n_mels; ++m) {
        uint32_t lo = J, hi = 0;
        for (uint32_t j = 0; j < J; ++j)
            if (fbank[(size_t)m * J + j] != 0.f) { if (lo == J) lo = j; hi = j + 1u; }
        if (lo == J) lo = hi = 0u;
        t->ends[2u * m] = lo; t->ends[2u * m + 1u] = hi;
    }
    return std::string();
}

// The host side of clx_mel_create_cepstral: the framed spec's checks and tables, then the cepstral options' checks and copies of the
// DCT and the lifter.
inline std::string clx_mel_build_cepstral(uint32_t n_fft, uint32_t win_length, uint32_t hop, const float* window, const float* fbank, uint32_t n_bins,
                                          uint32_t n_mels, uint32_t mode, float floor, clx_mel_tables* t, const clx_mel_frame_opts* fopts,
                                          const clx_mel_cep_opts* q) {
    if (!q) return "clx_mel_create_cepstral: null cepstral options";
    const std::string why = clx_mel_build_framed(n_fft, win_length, hop, window, fbank, n_bins, n_mels, mode, floor, t, nullptr, fopts);
    if (!why.empty()) return why;
    if (n_mels > clx_mel::kMaxCepMels) return "clx_mel_create_cepstral: a cepstral spec has at most 128 bands";
    if (n_bins > clx_mel::kBins) return "clx_mel_create_cepstral: a cepstral spec has at most 256 bins";
    if (q->n_ceps < 1u || q->n_ceps > n_mels) return "clx_mel_create_cepstral: n_ceps must be 1..n_mels";
    if (!q->dct) return "clx_mel_create_cepstral: null dct";
    if (q->energy > 1u) return "clx_mel_create_cepstral: energy must be 0 or 1";
    if (!std::isfinite(q->energy_scale) || !(q->energy_scale > 0.f)) return "clx_mel_create_cepstral: energy_scale must be finite and greater than 0";
    if (!std::isfinite(q->energy_floor) || !(q->energy_floor >= 0.f)) return "clx_mel_create_cepstral: energy_floor must be finite and not negative";
    t->n_ceps = q->n_ceps; t->energy = q->energy; t->energy_scale = q->energy_scale; t->energy_floor = q->energy_floor > 0.f ? q->energy_floor : 0.f;
    t->dct.assign(q->dct, q->dct + (size_t)q->n_ceps * n_mels);
    t->has_lifter = q->lifter ? 1u : 0u;
    if (q->lifter) t->lifter.assign(q->lifter, q->lifter + q->n_ceps);
    return std::string();
}

inline std::string clx_mel_build(uint32_t n_fft, uint32_t hop, const float* window, const float* fbank, uint32_t n_mels, uint32_t mode,
                                 float floor, clx_mel_tables* t, const clx_mel_opts* opts = nullptr) {
    return clx_mel_build_framed(n_fft, n_fft, hop, window, fbank, n_fft / 2u + 1u, n_mels, mode, floor, t, opts, nullptr);
}

// The host side of clx_mel_create_reflected: the framed spec's checks and tables, or the cepstral spec's when `q` is given, and the
// refusal of whole_frames (a reflected spec has a count rule of its own).
inline std::string clx_mel_build_reflected(uint32_t n_fft, uint32_t win_length, uint32_t hop, const float* window, const float* fbank, uint32_t n_bins,
                                           uint32_t n_mels, uint32_t mode, float floor, clx_mel_tables* t, const clx_mel_frame_opts* fopts,
                                           const clx_mel_cep_opts* q) {
    const std::string why = q ? clx_mel_build_cepstral(n_fft, win_length, hop, window, fbank, n_bins, n_mels, mode, floor, t, fopts, q)
                              : clx_mel_build_framed(n_fft, win_length, hop, window, fbank, n_bins, n_mels, mode, floor, t, nullptr, fopts);
    if (!why.empty()) return why;
    if (fopts && fopts->whole_frames != 0u) return "clx_mel_create_reflected: whole_frames must be 0, a reflected spec counts (valid + hop / 2) / hop frames";
    t->reflect = 1u;
    return std::string();
}

// The host side of clx_mel_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the launch
// shape: *n_groups frame groups per window (0: nothing to launch), n_windows * *n_groups blocks of clx_mel::kThreads.  A centred
// spec is held to torch.stft's frame count (P = n_fft / 2 < window_len, and the last frame ends inside window_len + 2 P), any other
// to (n_frames - 1) * hop + win_length <= window_len (win_length = n_fft unless the spec is framed), except a reflected spec, which
// is held to valid[k] <= window_len alone; a ranged
// one also gets *n_tiles, the tiles per window of clx_k_mel_range (n_windows * *n_tiles blocks).
inline const char* clx_mel_check(const clx_mel_tables* t, const void* audio, size_t n_windows, uint32_t window_len, const uint32_t* valid,
                                 uint32_t n_frames, uint32_t layout, const void* out, uint32_t* n_groups, uint32_t* n_tiles = nullptr) {
    *n_groups = 0;
    if (n_tiles) *n_tiles = 0;
    if (!t) return "clx_mel_windows: null spec";
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return "clx_mel_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT";
    if (n_windows == 0 || n_frames == 0) return nullptr;
    if (!audio || !valid || !out) return "clx_mel_windows: null argument";
    if (t->center) {
        const uint64_t P = t->n_fft / 2u;
        if (P >= window_len) return "clx_mel_windows: a centred spec needs n_fft / 2 less than window_len";
        if ((uint64_t)window_len + 2u * P < (uint64_t)(n_frames - 1u) * t->hop + t->n_fft) return "clx_mel_windows: window_len + 2 * (n_fft / 2) is less than (n_frames - 1) * hop + n_fft";
    } else if (!t->reflect && (uint64_t)window_len < (uint64_t)(n_frames - 1u) * t->hop + t->win)
        return t->win == t->n_fft ? "clx_mel_windows: window_len is less than (n_frames - 1) * hop + n_fft"
                                  : "clx_mel_windows: window_len is less than (n_frames - 1) * hop + win_length";
    for (size_t k = 0; k < n_windows; ++k)
        if (valid[k] > window_len) return "clx_mel_windows: valid[k] is larger than window_len";
    const uint64_t groups = ((uint64_t)n_frames + clx_mel::kF - 1u) / clx_mel::kF;
    if (groups * (uint64_t)n_windows > 0x7fffffffull) return "clx_mel_windows: too many windows in one call";
    if (t->range) {                                            // (a window's 16-byte grid has at most (cells + 6) / 4 vectors)
        const uint64_t cells = (uint64_t)t->n_mels * n_frames, tiles = (((cells + 6u) >> 2) + clx_mel::kRangeVecs - 1u) / clx_mel::kRangeVecs;
        if (tiles * (uint64_t)n_windows > 0x7fffffffull) return "clx_mel_windows: too many windows in one call";
        if (n_tiles) *n_tiles = (uint32_t)tiles;
    }
    *n_groups = (uint32_t)groups;
    return nullptr;
}

// valid_frames[k] = clamp(ceil(valid[k] / hop), 0, n_frames); centred by P: 0 for valid[k] == 0, else min(n_frames,
// ceil((valid[k] + P) / hop)), the frames with t * hop - P < valid[k].  whole_win (a framed spec that counts whole frames only: its
// win_length; else 0): 0 for valid[k] < whole_win, else min(n_frames, 1 + (valid[k] - whole_win) / hop)
inline void clx_mel_fill(uint32_t* vframes, const uint32_t* valid, size_t n_windows, uint32_t hop, uint32_t n_frames, uint32_t P = 0u,
                         uint32_t whole_win = 0u) {
    for (size_t k = 0; k < n_windows; ++k) {
        uint64_t v;
        if (whole_win) v = valid[k] < whole_win ? 0u : 1u + (uint64_t)(valid[k] - whole_win) / hop;
        else v = valid[k] ? ((uint64_t)valid[k] + P + hop - 1u) / hop : 0u;
        vframes[k] = v < n_frames ? (uint32_t)v : n_frames;
    }
}

// clx_k_mel_fr / clx_k_mel_qr run a reflected spec
inline bool clx_mel_is_r(const clx_mel_tables& t) { return t.reflect != 0u; }

// (their origin: the index of frame 0's tap 0)
inline int32_t clx_mel_origin(const clx_mel_tables& t) { return (int32_t)(t.hop / 2u) - (int32_t)(t.win / 2u); }

// their table, 2 * n_windows words: valid_frames[k] = min(n_frames, (valid[k] + hop / 2) / hop), then vlen[k] = valid[k]
inline void clx_mel_fill_r(uint32_t* table, const uint32_t* valid, size_t n_windows, const clx_mel_tables& t, uint32_t n_frames) {
    for (size_t k = 0; k < n_windows; ++k) {
        const uint64_t v = ((uint64_t)valid[k] + t.hop / 2u) / t.hop;
        table[k] = v < n_frames ? (uint32_t)v : n_frames;
        table[n_windows + k] = valid[k];
    }
}

// (clx_mel_fill's whole_win of a spec)
inline uint32_t clx_mel_whole(const clx_mel_tables& t) { return t.whole ? t.win : 0u; }

// clx_k_mel_f runs a spec that conditions its frames
inline bool clx_mel_is_f(const clx_mel_tables& t) { return t.remove_dc != 0u || t.preemph > 0.f; }

inline clx_mel_fdev clx_mel_fargs(const clx_mel_tables& t) {
    clx_mel_fdev f;
    f.remove_dc = t.remove_dc; f.preemph = t.preemph;
    return f;
}

// clx_k_mel_q runs a cepstral spec
inline bool clx_mel_is_q(const clx_mel_tables& t) { return t.n_ceps != 0u; }

// (dct and lifter: where the spec's copies are, for the kernel; lifter is ignored for a spec without one)
inline clx_mel_qdev clx_mel_qargs(const clx_mel_tables& t, const float* dct, const float* lifter) {
    clx_mel_qdev q;
    q.dct = dct; q.lifter = t.has_lifter ? lifter : nullptr;
    q.n_ceps = t.n_ceps; q.energy = t.energy; q.energy_scale = t.energy_scale; q.energy_floor = t.energy_floor;
    return q;
}

// the rows of a spec's output: n_ceps of a cepstral spec, else n_mels
inline uint32_t clx_mel_rows(const clx_mel_tables& t) { return t.n_ceps ? t.n_ceps : t.n_mels; }

inline bool clx_mel_is_c(const clx_mel_tables& t) { return t.center != 0u || t.range != 0u; }

inline clx_mel_cdev clx_mel_cargs(const clx_mel_tables& t) {
    clx_mel_cdev x;
    x.P = t.center ? t.n_fft / 2u : 0u; x.zero = t.center && t.pad == CLX_MEL_PAD_ZERO ? 1u : 0u; x.range = t.range;
    return x;
}

// clx_k_mel_c's table, 3 * n_windows words: valid_frames, then lim (valid[k] for zero padding, else window_len), then wmax
// (the encoding of -inf, so that the device needs no memset)
inline void clx_mel_fill_c(uint32_t* table, const uint32_t* valid, size_t n_windows, const clx_mel_tables& t, uint32_t window_len, uint32_t n_frames) {
    const clx_mel_cdev x = clx_mel_cargs(t);
    clx_mel_fill(table, valid, n_windows, t.hop, n_frames, x.P);
    for (size_t k = 0; k < n_windows; ++k) {
        table[n_windows + k] = x.zero ? valid[k] : window_len;
        table[2u * n_windows + k] = clx_mel::kEncNegInf;
    }
}

inline clx_mel_dev clx_mel_args(const clx_mel_tables& t, const float* basis, const float* fbank, const uint32_t* ends) {
    clx_mel_dev d;
    d.basis = basis; d.fbank = fbank; d.ends = ends;
    d.n_fft = t.win; d.hop = t.hop; d.n_mels = t.n_mels; d.n_bins = t.n_bins; d.n_pass = t.n_pass; d.n_slices = t.n_slices; d.mode = t.mode;
    d.floor = t.floor;
    return d;
}
