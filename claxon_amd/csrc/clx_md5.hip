// clx_md5.hip -- the FLAC audio MD5 (STREAMINFO's signature, metadata.rs:52-53) of many streams in one launch: one lane per stream.
//
// FLAC defines the signature over the stream's channel-interleaved samples, each written as its low ceil(bps / 8) bytes,
// little-endian (the message width w).  clx_k_md5 reads the samples from a device buffer of 1..4-byte little-endian PCM (what
// clx_batch_interleave, CLX_OUT_PCM16 and CLX_OUT_PCM24 write) or of CLX_OUT_F32 floats, scaled back exactly: v = f * 2^(bps-1).
//
// MD5 is serial within a stream; the parallelism is the number of streams.  A lane takes its stream in groups: 64 / w samples, one
// 64-byte block (w = 1, 2, 4), or 64 samples, three blocks (w = 3).  A group's source bytes come in with 16-byte loads issued before
// the previous group's compression (the chain of a block, 64 steps of 4 dependent VALU ops, is far longer than an HBM miss) and are
// unpacked into 16 message words with static indices: no LDS, no scratch.  The last partial group and the padding go through a
// generic tail that loads each sample at its own width, so no load reads past the stream's last sample byte whatever the alignment.
//
// clx_md5_plan is the host side (plain C++, shared with the wave simulator): argument checks, and the lanes' jobs sorted by width
// class, then by message length, longest first, so that the lanes of a wave finish together.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/claxon_hip.h"

struct clx_md5_job {
    uint64_t src;            // byte offset of the stream's first sample in the source buffer
    uint64_t n;              // samples
    uint32_t index;          // the stream's place in the caller's arrays: its digest goes to digests[index]
    uint32_t bps;
};

namespace clx_md5 {

__device__ __forceinline__ uint32_t rotl(uint32_t x, uint32_t s) { return (x << s) | (x >> (32u - s)); }

// one step: `t` = a + K + M is off the chain; on it: the round function, the add, the rotate, the add of b
#define CLX_MD5_STEP(F, a, b, c, d, i, s) { const uint32_t t_ = a + (kK[i] + M[kG[i]]); a = b + rotl(F(b, c, d) + t_, s); }
#define CLX_MD5_F(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define CLX_MD5_G(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define CLX_MD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define CLX_MD5_I(b, c, d) ((c) ^ ((b) | ~(d)))

__device__ __forceinline__ void block(uint32_t (&h)[4], const uint32_t (&M)[16]) {
    constexpr uint32_t kK[64] = {
        0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
        0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
        0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
        0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
        0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
        0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
        0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
        0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
    constexpr uint8_t kG[64] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,  1, 6, 11, 0, 5, 10, 15, 4, 9, 14, 3, 8, 13, 2, 7, 12,
                                5, 8, 11, 14, 1, 4, 7, 10, 13, 0, 3, 6, 9, 12, 15, 2,  0, 7, 14, 5, 12, 3, 10, 1, 8, 15, 6, 13, 4, 11, 2, 9};
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
        CLX_MD5_STEP(CLX_MD5_F, a, b, c, d, i + 0, 7) CLX_MD5_STEP(CLX_MD5_F, d, a, b, c, i + 1, 12)
        CLX_MD5_STEP(CLX_MD5_F, c, d, a, b, i + 2, 17) CLX_MD5_STEP(CLX_MD5_F, b, c, d, a, i + 3, 22)
    }
#pragma unroll
    for (int i = 16; i < 32; i += 4) {
        CLX_MD5_STEP(CLX_MD5_G, a, b, c, d, i + 0, 5) CLX_MD5_STEP(CLX_MD5_G, d, a, b, c, i + 1, 9)
        CLX_MD5_STEP(CLX_MD5_G, c, d, a, b, i + 2, 14) CLX_MD5_STEP(CLX_MD5_G, b, c, d, a, i + 3, 20)
    }
#pragma unroll
    for (int i = 32; i < 48; i += 4) {
        CLX_MD5_STEP(CLX_MD5_H, a, b, c, d, i + 0, 4) CLX_MD5_STEP(CLX_MD5_H, d, a, b, c, i + 1, 11)
        CLX_MD5_STEP(CLX_MD5_H, c, d, a, b, i + 2, 16) CLX_MD5_STEP(CLX_MD5_H, b, c, d, a, i + 3, 23)
    }
#pragma unroll
    for (int i = 48; i < 64; i += 4) {
        CLX_MD5_STEP(CLX_MD5_I, a, b, c, d, i + 0, 6) CLX_MD5_STEP(CLX_MD5_I, d, a, b, c, i + 1, 10)
        CLX_MD5_STEP(CLX_MD5_I, c, d, a, b, i + 2, 15) CLX_MD5_STEP(CLX_MD5_I, b, c, d, a, i + 3, 21)
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}
#undef CLX_MD5_STEP
#undef CLX_MD5_F
#undef CLX_MD5_G
#undef CLX_MD5_H
#undef CLX_MD5_I

// source bytes per sample of a format (1..4, CLX_SAMPLE_F32); 0: not a format
__host__ __device__ __forceinline__ uint32_t src_bytes(uint32_t fmt) {
    return fmt == CLX_SAMPLE_F32 ? 4u : (fmt >= 1u && fmt <= 4u) ? fmt : 0u;
}

// 16 source bytes at any alignment (global memory takes unaligned dword loads)
__device__ __forceinline__ uint4 ld16(const uint8_t* p) { uint4 v; memcpy(&v, p, 16); return v; }
template <int N> __device__ __forceinline__ uint32_t word(const uint4 (&c)[N], uint32_t i) {
    const uint4 q = c[i >> 2];
    return (i & 3u) == 0u ? q.x : (i & 3u) == 1u ? q.y : (i & 3u) == 2u ? q.z : q.w;
}

// The whole groups of one stream: SB source bytes per sample (F32: floats), W message bytes per sample.
template <uint32_t SB, bool F32, uint32_t W>
__device__ __forceinline__ void groups(uint32_t (&h)[4], const uint8_t* p, uint64_t n_groups, float scale) {
    constexpr uint32_t G = W == 3u ? 64u : 64u / W;            // samples per group
    constexpr uint32_t NB = G * W / 64u;                         // blocks per group
    constexpr uint32_t SQ = G * SB / 16u;                        // 16-byte loads per group
    static_assert(G * SB % 16u == 0u, "a group is whole 16-byte loads");
    if (n_groups == 0) return;
    uint4 cur[SQ];
#pragma unroll
    for (uint32_t x = 0; x < SQ; ++x) cur[x] = ld16(p + 16u * x);
    for (uint64_t g = 0; g < n_groups; ++g) {
        // the next group's loads first (the last group loads itself again: nothing past the stream's end is read)
        const uint8_t* q = p + (g + 1 < n_groups ? (g + 1) : g) * (uint64_t)(G * SB);
        uint4 nxt[SQ];
#pragma unroll
        for (uint32_t x = 0; x < SQ; ++x) nxt[x] = ld16(q + 16u * x);
        uint32_t v[F32 ? G : 1];
        if (F32) {
#pragma unroll
            for (uint32_t s = 0; s < G; ++s) v[s] = (uint32_t)(int32_t)(__uint_as_float(word(cur, s)) * scale);
        }
#pragma unroll
        for (uint32_t bl = 0; bl < NB; ++bl) {
            uint32_t M[16];
#pragma unroll
            for (uint32_t m = 0; m < 16u; ++m) {
                if (!F32 && SB == W) {
                    M[m] = word(cur, bl * 16u + m);
                } else {
                    uint32_t w = 0;
#pragma unroll
                    for (uint32_t j = 0; j < 4u; ++j) {
                        const uint32_t b = bl * 64u + 4u * m + j, s = b / W, k = b % W;      // message byte b: byte k of sample s
                        const uint32_t x = F32 ? (v[s] >> (8u * k)) & 0xffu : (word(cur, (s * SB + k) >> 2) >> (8u * ((s * SB + k) & 3u))) & 0xffu;
                        w |= x << (8u * j);
                    }
                    M[m] = w;
                }
            }
            block(h, M);
        }
#pragma unroll
        for (uint32_t x = 0; x < SQ; ++x) cur[x] = nxt[x];
    }
}

// The last r < G samples and the padding: each message byte from its own sample, loaded at the sample's width (a byte of PCM, the
// float of F32), then 0x80, zeros and the message's bit length.
__device__ __forceinline__ void tail(uint32_t (&h)[4], const uint8_t* p, uint32_t r, uint32_t sb, bool f32, uint32_t w, float scale,
                                     uint64_t bits) {
    const uint32_t tb = r * w;                                   // message bytes left
    const uint32_t nblk = (tb + 8u) / 64u + 1u;                  // blocks: the bytes, 0x80, the 8-byte length
    uint32_t s = 0, k = 0;                                       // the sample and byte of the next message byte
    for (uint32_t blk = 0; blk < nblk; ++blk) {
        uint32_t M[16];
#pragma unroll
        for (uint32_t m = 0; m < 16u; ++m) {
            uint32_t word = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t b = blk * 64u + 4u * m + j;
                uint32_t x = 0;
                if (b < tb) {
                    if (f32) {
                        uint32_t f;
                        memcpy(&f, p + 4u * s, 4);
                        x = ((uint32_t)(int32_t)(__uint_as_float(f) * scale) >> (8u * k)) & 0xffu;
                    } else {
                        x = p[s * sb + k];
                    }
                    if (++k == w) { k = 0; ++s; }
                } else if (b == tb) {
                    x = 0x80u;
                }
                word |= x << (8u * j);
            }
            M[m] = word;
        }
        if (blk + 1u == nblk) { M[14] = (uint32_t)bits; M[15] = (uint32_t)(bits >> 32); }
        block(h, M);
    }
}

template <uint32_t SB, bool F32, uint32_t W>
__device__ __forceinline__ void stream(uint32_t (&h)[4], const uint8_t* p, uint64_t n, float scale) {
    constexpr uint32_t G = W == 3u ? 64u : 64u / W;
    const uint64_t n_groups = n / G;
    groups<SB, F32, W>(h, p, n_groups, scale);
    tail(h, p + n_groups * (uint64_t)(G * SB), (uint32_t)(n - n_groups * G), SB, F32, W, scale, n * W * 8u);
}

}  // namespace clx_md5

// Lane i hashes jobs[i] (fmt: 1..4 or CLX_SAMPLE_F32; w: every job's message width, one launch per width class) and writes its
// digest to digests[jobs[i].index] with one vector store.
extern "C" __global__ __launch_bounds__(64) void clx_k_md5(const uint8_t* __restrict__ samples, const clx_md5_job* __restrict__ jobs, uint32_t n_jobs,
                                                uint32_t fmt, uint32_t w, uint4* __restrict__ digests) {
    using namespace clx_md5;
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_jobs) return;
    const clx_md5_job job = jobs[i];
    const uint8_t* p = samples + job.src;
    const float scale = (float)(1u << ((job.bps - 1u) & 31u));  // (F32 only: bps <= 24, exact)
    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    const uint32_t key = fmt == CLX_SAMPLE_F32 ? 0x50u + w : fmt * 16u + w;
    switch (key) {
    case 0x11: stream<1, false, 1>(h, p, job.n, scale); break;
    case 0x21: stream<2, false, 1>(h, p, job.n, scale); break;
    case 0x22: stream<2, false, 2>(h, p, job.n, scale); break;
    case 0x31: stream<3, false, 1>(h, p, job.n, scale); break;
    case 0x32: stream<3, false, 2>(h, p, job.n, scale); break;
    case 0x33: stream<3, false, 3>(h, p, job.n, scale); break;
    case 0x41: stream<4, false, 1>(h, p, job.n, scale); break;
    case 0x42: stream<4, false, 2>(h, p, job.n, scale); break;
    case 0x43: stream<4, false, 3>(h, p, job.n, scale); break;
    case 0x44: stream<4, false, 4>(h, p, job.n, scale); break;
    case 0x51: stream<4, true, 1>(h, p, job.n, scale); break;
    case 0x52: stream<4, true, 2>(h, p, job.n, scale); break;
    case 0x53: stream<4, true, 3>(h, p, job.n, scale); break;
    default: return;                                             // (the host refuses every other combination)
    }
    digests[job.index] = make_uint4(h[0], h[1], h[2], h[3]);
}

#include <algorithm>
#include <vector>

// The host side of clx_md5_streams: checks the arguments (nullptr: fine, else the text for clx_last_error) and makes the lanes' jobs,
// grouped by message width w = 1..4 (jobs[cls[w - 1] .. cls[w]) have width w), within a class sorted by message length, longest first.
inline const char* clx_md5_plan(const void* samples, uint32_t fmt, const uint64_t* first_sample, const uint64_t* n_samples, const uint8_t* bps,
                                size_t n, const void* digests, std::vector<clx_md5_job>& jobs, size_t cls[5]) {
    jobs.clear();
    for (int c = 0; c < 5; ++c) cls[c] = 0;
    const uint32_t sb = clx_md5::src_bytes(fmt);
    if (!sb) return "clx_md5_streams: sample_format must be 1..4 or CLX_SAMPLE_F32";
    if (n == 0) return nullptr;
    if (!samples || !first_sample || !n_samples || !bps || !digests) return "clx_md5_streams: null argument";
    if (n > 0xffffffffull) return "clx_md5_streams: too many streams in one call";
    for (size_t k = 0; k < n; ++k) {
        if (bps[k] < 1u || bps[k] > 32u) return "clx_md5_streams: bits per sample must be 1..32";
        if ((bps[k] + 7u) / 8u > sb) return "clx_md5_streams: ceil(bps / 8) is wider than the source's samples";
        if (fmt == CLX_SAMPLE_F32 && bps[k] > 24u) return "clx_md5_streams: CLX_SAMPLE_F32 holds at most 24 bits per sample exactly";
    }
    jobs.resize(n);
    for (size_t k = 0; k < n; ++k) jobs[k] = clx_md5_job{first_sample[k] * sb, n_samples[k], (uint32_t)k, bps[k]};
    auto width = [](const clx_md5_job& j) { return (j.bps + 7u) / 8u; };
    std::stable_sort(jobs.begin(), jobs.end(), [&](const clx_md5_job& a, const clx_md5_job& b) {
        const uint32_t wa = width(a), wb = width(b);
        return wa != wb ? wa < wb : a.n * wa > b.n * wb;
    });
    for (const clx_md5_job& j : jobs) ++cls[width(j)];
    for (int c = 1; c < 5; ++c) cls[c] += cls[c - 1];           // (cls[w] now counts the jobs of width <= w)
    return nullptr;
}
