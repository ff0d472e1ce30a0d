// clx_window.hip -- a dense batch of fixed-length sample windows gathered from CLX_OUT_F32 audio, in one launch.
//
// The source is channel-interleaved float32 (what CLX_OUT_F32 writes).  Window k is valid[k] <= L samples per channel from float
// src_first[k] on; the output is [B, L, C] (CLX_WINDOW_TC: a plain copy of the run) or [B, C, L] (CLX_WINDOW_CT: channels first,
// de-interleaved), with every sample from valid[k] on written as zero.  The kernel owns the whole output and reads no float of the
// source outside [src_first[k], src_first[k] + valid[k] * C).  Samples are moved as 32-bit words: nothing is computed with them.
//
// The output is a set of ROWS, each a contiguous run of floats: the whole window in TC (n = L * C floats, source stride 1), one
// channel of a window in CT (n = L floats, source stride C).  A row is cut on the 16-byte grid of its own ADDRESS, so its first and
// last vector may be shared with a neighbouring row: those two give up to three scalar stores each, every vector between them is one
// aligned 16-byte store, and the 64 lanes of a wave store 64 consecutive vectors -- eight whole 128-byte lines.  A vector takes one
// of four ways, all in the one launch:
//   whole and valid, stride 1     one 16-byte load (at the source's own 4-byte alignment), one 16-byte store;
//   whole and valid, stride C     four dword loads, one 16-byte store;
//   whole and past valid[k]       one 16-byte store of zeros, no load;
//   anything else (a row's ragged head or tail, the vector valid[k] falls in): each float on its own, loaded only below valid[k];
//                                 one 16-byte store when the vector lies inside the row, else a dword store per float of the row.
// CT with every row on the 16-byte grid (L a multiple of 4 and an aligned output: any sensible crop length) takes a shorter way for
// the vectors that are whole and valid: a lane loads its 4 samples x C channels as C consecutive 16-byte vectors -- the wave reads
// one contiguous run of 64 * 16 * C bytes -- transposes them in its registers (static indices, C is a template argument) and stores
// one 16-byte vector to each channel's row.  No LDS, no cross-lane traffic, no scratch.
//
// The grid is (window, tile): a tile is kTileVec vectors of a row's grid -- 4096 floats of a TC window, 4096 samples of all C channels
// of a CT window -- so a batch of few long windows still spreads over the device; block b is tile b % n_tiles of window b / n_tiles.
//
// clx_window_check is the host side (plain C++, shared with the wave simulator): the argument checks and the launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/claxon_hip.h"

struct clx_win_job {
    uint64_t src_first;      // float index in the source of the window's first sample, channel 0
    uint32_t valid;          // samples per channel to copy (<= the window length); the rest of the window is zeros
    uint32_t reserved;
};

namespace clx_win {

constexpr uint32_t kThreads = 256u, kVecPerLane = 4u, kTileVec = kThreads * kVecPerLane;

__device__ __forceinline__ uint4 ld16(const uint32_t* p) { uint4 v; memcpy(&v, p, 16); return v; }      // (4-byte aligned: global memory takes it)
__device__ __forceinline__ void st16(uint32_t* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; }  // (16-byte aligned)

// A row: n floats at `row`, the first nv of them src[i * stride], the rest zeros.  `head` = floats of the row's first 16-byte vector
// that lie in front of the row (0..3); vector v of the row's grid holds the row's floats 4 * v - head .. + 3.
struct Row {
    const uint32_t* src;
    uint32_t* row;
    uint64_t n, nv;
    uint32_t stride, head;
    __device__ __forceinline__ uint64_t vectors() const { return (n + head + 3u) >> 2; }
};

__device__ __forceinline__ Row make_row(const uint32_t* src, uint32_t* row, uint64_t n, uint64_t nv, uint32_t stride) {
    Row r;
    r.src = src; r.row = row; r.n = n; r.nv = nv; r.stride = stride;
    r.head = (uint32_t)(((uintptr_t)row >> 2) & 3u);
    return r;
}

// vector v of the row's grid (v < r.vectors())
__device__ __forceinline__ void put_vector(const Row& r, uint64_t v) {
    const int64_t e0 = (int64_t)(v * 4u) - (int64_t)r.head;       // the row's float in the vector's first place (-3 .. n - 1)
    uint32_t* const dst = r.row + e0;                             // 16-byte aligned
    const bool inside = e0 >= 0 && (uint64_t)e0 + 4u <= r.n;
    if (inside && (uint64_t)e0 + 4u <= r.nv) {
        uint4 q;
        if (r.stride == 1u) {
            q = ld16(r.src + e0);
        } else {
            const uint32_t* p = r.src + (uint64_t)e0 * r.stride;
            q = make_uint4(p[0], p[r.stride], p[2u * (size_t)r.stride], p[3u * (size_t)r.stride]);
        }
        st16(dst, q);
    } else if (inside && (uint64_t)e0 >= r.nv) {
        st16(dst, make_uint4(0u, 0u, 0u, 0u));
    } else {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t e = e0 + j;
            w[j] = (e >= 0 && (uint64_t)e < r.nv) ? r.src[(uint64_t)e * r.stride] : 0u;
        }
        if (inside) {
            st16(dst, make_uint4(w[0], w[1], w[2], w[3]));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t e = e0 + j;
                if (e >= 0 && (uint64_t)e < r.n) dst[j] = w[j];
            }
        }
    }
}

// the tile's vectors of one row: lane l of the block takes vectors tile * kTileVec + l, + kThreads, ...
__device__ __forceinline__ void put_tile(const Row& r, uint32_t tile) {
    const uint64_t nvec = r.vectors(), v0 = (uint64_t)tile * kTileVec + threadIdx.x;
#pragma unroll
    for (uint32_t i = 0; i < kVecPerLane; ++i) {
        const uint64_t v = v0 + i * kThreads;
        if (v < nvec) put_vector(r, v);
    }
}

// CT, every row of the window on the 16-byte grid (head 0, L a multiple of 4): src = the window's first float, out = its first row.
template <uint32_t C>
__device__ __forceinline__ void put_tile_ct(const uint32_t* src, uint32_t* out, uint32_t L, uint32_t nv, uint32_t tile) {
    const uint64_t v0 = (uint64_t)tile * kTileVec + threadIdx.x;
#pragma unroll
    for (uint32_t i = 0; i < kVecPerLane; ++i) {
        const uint64_t v = v0 + i * kThreads, t0 = v * 4u;            // samples t0 .. t0 + 3
        if (t0 >= L) continue;
        if (t0 + 4u <= nv) {
            uint4 q[C];
#pragma unroll
            for (uint32_t x = 0; x < C; ++x) q[x] = ld16(src + t0 * C + 4u * x);
            uint32_t w[4u * C];
#pragma unroll
            for (uint32_t x = 0; x < C; ++x) { w[4u * x] = q[x].x; w[4u * x + 1u] = q[x].y; w[4u * x + 2u] = q[x].z; w[4u * x + 3u] = q[x].w; }
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) st16(out + (uint64_t)c * L + t0, make_uint4(w[c], w[C + c], w[2u * C + c], w[3u * C + c]));
        } else {
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) put_vector(make_row(src + c, out + (uint64_t)c * L, L, nv, C), v);
        }
    }
}

}  // namespace clx_win

// Block b: tile b % n_tiles of window b / n_tiles (clx_window_check gives n_tiles).  `out` is the dense [B, L, C] / [B, C, L] batch.
extern "C" __global__ __launch_bounds__(256) void clx_k_window(const uint32_t* __restrict__ src, const clx_win_job* __restrict__ win, uint32_t n_tiles,
                                                    uint32_t L, uint32_t C, uint32_t layout, uint32_t* __restrict__ out) {
    using namespace clx_win;
    const uint32_t k = blockIdx.x / n_tiles, tile = blockIdx.x - k * n_tiles;
    const clx_win_job w = win[k];
    const uint32_t* s = src + w.src_first;
    uint32_t* o = out + (uint64_t)k * L * C;
    if (layout == CLX_WINDOW_TC || C == 1u) {                     // (one channel: the two layouts are the same bytes)
        put_tile(make_row(s, o, (uint64_t)L * C, (uint64_t)w.valid * C, 1u), tile);
        return;
    }
    if ((L & 3u) == 0u && ((uintptr_t)out & 15u) == 0u) {
        switch (C) {
        case 2: put_tile_ct<2>(s, o, L, w.valid, tile); return;
        case 3: put_tile_ct<3>(s, o, L, w.valid, tile); return;
        case 4: put_tile_ct<4>(s, o, L, w.valid, tile); return;
        case 5: put_tile_ct<5>(s, o, L, w.valid, tile); return;
        case 6: put_tile_ct<6>(s, o, L, w.valid, tile); return;
        case 7: put_tile_ct<7>(s, o, L, w.valid, tile); return;
        default: put_tile_ct<8>(s, o, L, w.valid, tile); return;
        }
    }
    for (uint32_t c = 0; c < C; ++c) put_tile(make_row(s + c, o + (uint64_t)c * L, L, w.valid, C), tile);
}

// The host side of clx_gather_windows: checks the arguments (nullptr: fine, else the text for clx_last_error) and gives the launch
// shape: *n_tiles tiles per window (0: nothing to launch), n_windows * *n_tiles blocks of clx_win::kThreads.
inline const char* clx_window_check(const void* src, const uint64_t* src_first, const uint32_t* valid, size_t n_windows, uint32_t window_len,
                                    uint32_t channels, uint32_t layout, const void* out, uint32_t* n_tiles) {
    *n_tiles = 0;
    if (channels < 1u || channels > 8u) return "clx_gather_windows: channels must be 1..8";
    if (layout != CLX_WINDOW_TC && layout != CLX_WINDOW_CT) return "clx_gather_windows: layout must be CLX_WINDOW_TC or CLX_WINDOW_CT";
    if (n_windows == 0 || window_len == 0) return nullptr;
    if (!src || !src_first || !valid || !out) return "clx_gather_windows: null argument";
    for (size_t k = 0; k < n_windows; ++k)
        if (valid[k] > window_len) return "clx_gather_windows: valid[k] is larger than window_len";
    // a row's grid has at most (n + 6) / 4 vectors (its address may put up to 3 floats of a neighbour in front of it)
    const uint64_t row = (layout == CLX_WINDOW_TC || channels == 1u) ? (uint64_t)window_len * channels : window_len;
    const uint64_t tiles = ((row + 6u) / 4u + clx_win::kTileVec - 1u) / clx_win::kTileVec;
    if (tiles * (uint64_t)n_windows > 0x7fffffffull) return "clx_gather_windows: too many windows in one call";
    *n_tiles = (uint32_t)tiles;
    return nullptr;
}

inline void clx_window_fill(clx_win_job* tab, const uint64_t* src_first, const uint32_t* valid, size_t n_windows) {
    for (size_t k = 0; k < n_windows; ++k) tab[k] = clx_win_job{src_first[k], valid[k], 0u};
}
