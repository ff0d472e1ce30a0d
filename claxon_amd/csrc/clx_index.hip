// clx_index.hip -- the segmented frame indexer: every stream of a shard indexed in one pass (clx_index_streams_device).
//
// The shard is one arena that holds n streams at ascending, 16-byte aligned offsets.  The answer for each stream is what the host
// indexer clx_index_frames gives for that stream alone (the grammar and the chain rule are described at K5 / K6 in clx_kernels.hip),
// so every decision is bounded by the stream's own end: nothing of a neighbour is probed, summed or accepted as a frame's end.
//
//   K8  clx_k_idx_scan     one thread per aligned 16-byte chunk of the arena (a chunk belongs to at most one stream: streams start on
//                          16 bytes).  The thread finds its stream in the sorted table by binary search and tests its 16 positions as
//                          K5 does, bounded by [begin, end) of that stream.  It writes a 16-bit hit mask per chunk -- one bit per byte
//                          position, ordered by construction, nothing to overflow -- and the workgroup writes its number of hits.
//   K9  clx_k_idx_offsets  one workgroup: the exclusive prefix sum of the workgroups' hit counts, and the total.
//   K10 clx_k_idx_compact  the masks become the ordered candidate list: position, stream, and the first 20 bytes of each (zero padded
//                          at the stream's end) for the host's authoritative header parse.
//   K11 clx_k_idx_span_crc one wave per candidate: CRC-16 of the bytes up to the next candidate of the SAME stream, or to the stream's
//                          end (as K6, with the span's end chosen per stream).
//
// The host meets the device twice per call whatever n is: once for the number of candidates (it sizes the lists), once for the lists.
// clx_idx_check (the stream table), clx_idx_chain (the authoritative parse, the chain walk and the descriptors) and clx_idx_run (the
// call's order of steps, over a `Dev` that launches the kernels and fetches their results) are the host side, plain C++ shared with
// the wave simulator: the library and the simulator differ only in their Dev.
//
// Included behind clx_kernels.hip (clx_header_probe, clx_crc16_byte, clx_gf_mulmod, clx_xpow8_64).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/claxon_hip.h"

struct clx_idx_stream {
    uint64_t off;            // the stream's first byte in the arena (a multiple of 16)
    uint64_t begin;          // where indexing begins: off + starts[k]
    uint64_t end;            // one past the stream's last byte: off + lens[k]
};

#define CLX_IDX_HDR_BYTES 20u     // bytes of a candidate handed to the host's header parse (a frame header is at most 16 long)

namespace clx_idx {

// the stream that holds arena offset `base` (a multiple of 16): the last one that starts at or before it; false when none does or
// that stream ends at or before `base` (padding between streams, empty streams)
__device__ __forceinline__ bool find_stream(const clx_idx_stream* __restrict__ tab, uint32_t n, uint64_t base, uint32_t& k, clx_idx_stream& s) {
    uint32_t lo = 0u, hi = n;                               // (tab[lo - 1].off <= base < tab[hi].off)
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (tab[mid].off <= base) lo = mid + 1u; else hi = mid;
    }
    if (lo == 0u) return false;
    k = lo - 1u;
    s = tab[k];
    return base < s.end;
}

// the 16 positions of the chunk at `base` that hold a candidate header of stream `s`, one bit each; loads stay below round16(s.end)
__device__ __forceinline__ uint32_t chunk_mask(const uint8_t* __restrict__ data, uint64_t base, const clx_idx_stream& s) {
    const uint4 v = *reinterpret_cast<const uint4*>(data + base);
    const uint32_t nxt = base + 16u < s.end ? data[base + 16u] : 0u;
    const uint32_t w[5] = { v.x, v.y, v.z, v.w, nxt };
    uint32_t mask = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t b0 = (w[i >> 2] >> (8u * (i & 3u))) & 0xffu;
        const uint32_t b1 = (w[(i + 1u) >> 2] >> (8u * ((i + 1u) & 3u))) & 0xffu;
        if (b0 == 0xffu && (b1 & 0xfeu) == 0xf8u) {
            const uint64_t p = base + i;
            if (p >= s.begin && p + 2u <= s.end && clx_header_probe(data + p, s.end - p) != 0u) mask |= 1u << i;
        }
    }
    return mask;
}

}  // namespace clx_idx

// K8: chunk c of the launch is arena bytes [(chunk0 + c) * 16, +16)
extern "C" __global__ __launch_bounds__(256)
void clx_k_idx_scan(const uint8_t* __restrict__ data, const clx_idx_stream* __restrict__ tab, uint32_t n_streams, uint64_t chunk0,
                    uint64_t n_chunks, uint16_t* __restrict__ mask, uint32_t* __restrict__ blk_count) {
    __shared__ uint32_t wave_hits[4];
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t m = 0u;
    if (c < n_chunks) {
        uint32_t k; clx_idx_stream s;
        const uint64_t base = (chunk0 + c) * 16u;
        if (clx_idx::find_stream(tab, n_streams, base, k, s)) m = clx_idx::chunk_mask(data, base, s);
        mask[c] = (uint16_t)m;
    }
    uint32_t hits = (uint32_t)__popc(m);
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) hits += __shfl_xor(hits, sft, 64);
    if ((threadIdx.x & 63u) == 0u) wave_hits[threadIdx.x >> 6] = hits;
    __syncthreads();
    if (threadIdx.x == 0u) blk_count[blockIdx.x] = wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
}

// K9: blk_base[b] = the hits of the workgroups in front of b; blk_base[n_blocks] = all of them.  One workgroup of 256.
extern "C" __global__ __launch_bounds__(256)
void clx_k_idx_offsets(const uint32_t* __restrict__ blk_count, uint32_t n_blocks, uint32_t* __restrict__ blk_base) {
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_blocks + 255u) / 256u;
    const uint32_t lo = t * per < n_blocks ? t * per : n_blocks;
    const uint32_t hi = lo + per < n_blocks ? lo + per : n_blocks;
    uint32_t sum = 0u;
    for (uint32_t b = lo; b < hi; ++b) sum += blk_count[b];
    part[t] = sum;
    __syncthreads();
    if (t == 0u) {
        uint32_t acc = 0u;
        for (uint32_t i = 0; i < 256u; ++i) { const uint32_t v = part[i]; part[i] = acc; acc += v; }
        blk_base[n_blocks] = acc;
    }
    __syncthreads();
    uint32_t acc = part[t];
    for (uint32_t b = lo; b < hi; ++b) { blk_base[b] = acc; acc += blk_count[b]; }
}

// K10: candidate number blk_base[workgroup] + (hits of the workgroup's earlier chunks) + (earlier bits of the mask) is the set bit's place
// in the list.  cand_cap bounds the stores (the host sized the lists from K9's total).
extern "C" __global__ __launch_bounds__(256)
void clx_k_idx_compact(const uint8_t* __restrict__ data, const clx_idx_stream* __restrict__ tab, uint32_t n_streams, uint64_t chunk0,
                       uint64_t n_chunks, const uint16_t* __restrict__ mask, const uint32_t* __restrict__ blk_base, uint32_t cand_cap,
                       uint64_t* __restrict__ cand_pos, uint32_t* __restrict__ cand_sid, uint8_t* __restrict__ cand_hdr) {
    __shared__ uint32_t wave_hits[4];
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t m = c < n_chunks ? (uint32_t)mask[c] : 0u;
    const uint32_t hits = (uint32_t)__popc(m);
    uint32_t incl = hits;                                    // inclusive scan over the wave
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63u) wave_hits[wave] = incl;
    __syncthreads();
    uint32_t k = blk_base[blockIdx.x] + incl - hits;
    for (uint32_t w = 0; w < wave; ++w) k += wave_hits[w];
    if (m == 0u) return;
    const uint64_t base = (chunk0 + c) * 16u;
    uint32_t sid; clx_idx_stream s;
    if (!clx_idx::find_stream(tab, n_streams, base, sid, s)) return;       // (cannot happen: the mask was made for this stream)
    for (; m != 0u && k < cand_cap; m &= m - 1u, ++k) {
        const uint64_t p = base + (uint32_t)(__ffs((int)m) - 1);
        cand_pos[k] = p;
        cand_sid[k] = sid;
        uint8_t* __restrict__ h = cand_hdr + (size_t)k * CLX_IDX_HDR_BYTES;
        for (uint32_t j = 0; j < CLX_IDX_HDR_BYTES; ++j) h[j] = p + j < s.end ? data[p + j] : (uint8_t)0u;
    }
}

// K11: span j = [cand_pos[j], the next candidate of the same stream | the stream's end); one wave per span, as K6
extern "C" __global__ __launch_bounds__(64)
void clx_k_idx_span_crc(const uint8_t* __restrict__ data, const clx_idx_stream* __restrict__ tab, const uint64_t* __restrict__ cand_pos,
                        const uint32_t* __restrict__ cand_sid, uint32_t n_cand, uint16_t* __restrict__ crc_out) {
    const uint32_t lane = threadIdx.x;
    const uint32_t j = blockIdx.x;
    if (j >= n_cand) return;
    const uint64_t p0 = cand_pos[j];
    const uint32_t sid = cand_sid[j];
    const uint64_t p1 = (j + 1u < n_cand && cand_sid[j + 1u] == sid) ? cand_pos[j + 1u] : tab[sid].end;
    const uint8_t* __restrict__ p = data + p0;
    const uint64_t nbytes = p1 - p0;
    const uint64_t per = (nbytes + 63u) / 64u;
    const uint64_t lo = (uint64_t)lane * per < nbytes ? (uint64_t)lane * per : nbytes;
    const uint64_t hi = lo + per < nbytes ? lo + per : nbytes;
    uint32_t crc = 0u;
    for (uint64_t i = lo; i < hi; ++i) crc = clx_crc16_byte(crc, p[i]);
    uint32_t contrib = (hi > lo) ? clx_gf_mulmod(crc, clx_xpow8_64(nbytes - hi)) : 0u;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) contrib ^= __shfl_xor(contrib, s, 64);
    if (lane == 0u) crc_out[j] = (uint16_t)contrib;
}

// ------------------------------------------------------------------------------------------------
// host side (plain C++, shared with the wave simulator)
// ------------------------------------------------------------------------------------------------
#include <stdio.h>
#include <string>
#include <vector>

#define CLX_IDX_MAX_ARENA 0xffffffffull      // candidate numbers are 32 bits wide: at most one candidate per two bytes of < 4 GiB

// clx_parse_frame_header's signature: the authoritative header parse (clx_api.hip), handed in so that this file stands without it
typedef int (*clx_idx_parse_fn)(const uint8_t* p, size_t avail, int check_crc, clx_frame_header* out, uint32_t* msg);

// Checks clx_index_streams_device's arguments and makes the stream table.  Empty string: fine; else the text for clx_last_error.
inline std::string clx_idx_check(const uint8_t* arena, size_t arena_len, const uint64_t* offs, const uint64_t* lens, const uint64_t* starts,
                                 size_t n, const clx_frame_desc* descs, size_t cap, const uint64_t* first_frame, const uint64_t* stop_offs,
                                 const size_t* n_found, std::vector<clx_idx_stream>& tab) {
    tab.clear();
    char buf[160];
    if (!n_found || !first_frame) return "clx_index_streams_device: null output (first_frame, n_found)";
    if (n == 0) return "";
    if (!stop_offs || (cap && !descs)) return "clx_index_streams_device: null output (descs, stop_offs)";
    if (!offs || !lens) return "clx_index_streams_device: null argument (offs, lens)";
    if (n > 0xfffffffeull) return "clx_index_streams_device: too many streams in one call";
    if (arena_len > CLX_IDX_MAX_ARENA) return "clx_index_streams_device: an arena of 4 GiB or more must be indexed in parts";
    tab.resize(n);
    uint64_t prev_end = 0;
    for (size_t k = 0; k < n; ++k) {
        const uint64_t off = offs[k], len = lens[k], st = starts ? starts[k] : 0;
        const char* why = nullptr;
        if (off & 15u) why = "does not start on a multiple of 16 bytes";
        else if (off > arena_len || len > arena_len - off) why = "lies outside the arena";
        else if (off < prev_end) why = "starts in front of its predecessor's end (streams must ascend and not overlap)";
        else if (st > len) why = "has its start offset behind its end";
        if (why) {
            snprintf(buf, sizeof buf, "clx_index_streams_device: stream %zu %s", k, why);
            tab.clear();
            return buf;
        }
        tab[k] = clx_idx_stream{off, off + st, off + len};
        prev_end = off + len;
    }
    bool any = false;
    for (const clx_idx_stream& s : tab) any = any || s.end > s.off;
    if (any && !arena) { tab.clear(); return "clx_index_streams_device: null arena"; }
    return "";
}

// The chain walk of every stream over the ordered candidate list (K10 / K11's output, on the host): each candidate's header is
// parsed by `parse` as the host indexer parses it (with what is left of ITS stream as the bytes available); frame i of a stream
// ends at the first later valid candidate of that stream, or at the stream's end, e >= its header + 2 with crc16([pos_i, e)) == 0.
// Fills descs / hdrs (arena offsets, max_bytes to the stream's end), first_frame (n + 1 entries) and stop_offs (n entries).
inline void clx_idx_chain(const std::vector<clx_idx_stream>& tab, const uint64_t* cand_pos, const uint32_t* cand_sid, const uint8_t* cand_hdr,
                          const uint16_t* cand_crc, size_t n_cand, clx_idx_parse_fn parse,
                          std::vector<clx_frame_desc>& descs, std::vector<clx_frame_header>& hdrs, uint64_t* first_frame, uint64_t* stop_offs) {
    descs.clear(); hdrs.clear();
    std::vector<clx_frame_header> h;          // of the current stream's candidates; valid[i]: the host parser accepts candidate i
    std::vector<uint8_t> valid;
    size_t c0 = 0;
    for (size_t k = 0; k < tab.size(); ++k) {
        const clx_idx_stream& s = tab[k];
        first_frame[k] = descs.size();
        stop_offs[k] = s.begin;
        while (c0 < n_cand && cand_sid[c0] < k) ++c0;
        size_t c1 = c0;
        while (c1 < n_cand && cand_sid[c1] == k) ++c1;
        const size_t m = c1 - c0;             // candidates c0 .. c1 belong to this stream; "candidate m" is the stream's end
        if (m == 0 || cand_pos[c0] != s.begin) { c0 = c1; continue; }      // no frame starts where indexing begins
        h.assign(m, clx_frame_header{}); valid.assign(m, 0);
        for (size_t i = 0; i < m; ++i) {
            uint32_t msg;
            const size_t avail = (size_t)(s.end - cand_pos[c0 + i] < CLX_IDX_HDR_BYTES ? s.end - cand_pos[c0 + i] : CLX_IDX_HDR_BYTES);
            valid[i] = parse(cand_hdr + (c0 + i) * CLX_IDX_HDR_BYTES, avail, 1, &h[i], &msg) == CLX_OK;
        }
        auto pos = [&](size_t i) { return i < m ? cand_pos[c0 + i] : s.end; };
        size_t cur = 0;
        if (!valid[0]) { c0 = c1; continue; }
        while (cur < m) {
            uint32_t acc = 0; size_t end = 0;
            for (size_t j = cur + 1; j <= m; ++j) {
                acc = clx_gf_mulmod(acc, clx_xpow8_64(pos(j) - pos(j - 1))) ^ cand_crc[c0 + j - 1];
                if (acc == 0u && (j == m || valid[j]) && pos(j) >= pos(cur) + h[cur].header_bytes + 2u) { end = j; break; }
            }
            if (!end) break;
            clx_frame_desc d;
            memset(&d, 0, sizeof d);
            d.byte_off = pos(cur);
            d.max_bytes = (uint32_t)(s.end - pos(cur) < 0xffffffffull ? s.end - pos(cur) : 0xffffffffull);
            d.header_bytes = h[cur].header_bytes;
            d.block_size = h[cur].block_size;
            d.n_channels = h[cur].n_channels;
            d.channel_assignment = h[cur].channel_assignment;
            d.bps = h[cur].bps;
            descs.push_back(d);
            hdrs.push_back(h[cur]);
            cur = end;
        }
        stop_offs[k] = pos(cur);
        c0 = c1;
    }
    first_frame[tab.size()] = descs.size();
}

// clx_index_streams_device's body.  `Dev` runs the kernels on the arena it holds and brings their results to the host:
//   bool scan(tab, chunk0, n_chunks, n_blocks, &n_cand)                       K8 + K9 over chunks [chunk0, chunk0 + n_chunks); meeting 1
//   bool lists(tab, chunk0, n_chunks, n_blocks, n_cand, pos, sid, hdr, crc)   K10 + K11 into host arrays of n_cand entries; meeting 2
// (false: it failed and has put the reason into `err`).  Returns the call's status; on CLX_API_ERROR `err` is the text for clx_last_error.
template <class Dev>
inline int clx_idx_run(Dev& dev, std::string& err, const uint8_t* arena, size_t arena_len, const uint64_t* offs, const uint64_t* lens,
                       const uint64_t* starts, size_t n_streams, clx_frame_desc* descs, clx_frame_header* headers, size_t cap,
                       uint64_t* first_frame, uint64_t* stop_offs, size_t* n_found, clx_idx_parse_fn parse) {
    std::vector<clx_idx_stream> tab;
    err = clx_idx_check(arena, arena_len, offs, lens, starts, n_streams, descs, cap, first_frame, stop_offs, n_found, tab);
    if (!err.empty()) return CLX_API_ERROR;
    *n_found = 0;
    first_frame[0] = 0;
    if (n_streams == 0) return CLX_OK;
    uint64_t lo = ~0ull, hi = 0;                          // the bytes that belong to a stream at all
    for (const clx_idx_stream& s : tab) if (s.end > s.off) { if (s.off < lo) lo = s.off; if (s.end > hi) hi = s.end; }
    std::vector<uint64_t> cand_pos; std::vector<uint32_t> cand_sid; std::vector<uint8_t> cand_hdr; std::vector<uint16_t> cand_crc;
    uint32_t n_cand = 0;
    if (hi > lo) {
        const uint64_t chunk0 = lo / 16u, n_chunks = (hi + 15u) / 16u - chunk0;
        const uint32_t n_blocks = (uint32_t)((n_chunks + 255u) / 256u);
        if (!dev.scan(tab, chunk0, n_chunks, n_blocks, &n_cand)) return CLX_API_ERROR;
        if (n_cand) {
            cand_pos.assign(n_cand, ~0ull); cand_sid.assign(n_cand, ~0u); cand_hdr.assign((size_t)n_cand * CLX_IDX_HDR_BYTES, 0); cand_crc.assign(n_cand, 0);
            if (!dev.lists(tab, chunk0, n_chunks, n_blocks, n_cand, cand_pos.data(), cand_sid.data(), cand_hdr.data(), cand_crc.data())) return CLX_API_ERROR;
        }
    }
    std::vector<clx_frame_desc> d; std::vector<clx_frame_header> h;
    clx_idx_chain(tab, cand_pos.data(), cand_sid.data(), cand_hdr.data(), cand_crc.data(), n_cand, parse, d, h, first_frame, stop_offs);
    *n_found = d.size();
    if (d.size() > cap) {
        char buf[128];
        snprintf(buf, sizeof buf, "clx_index_streams_device: %zu frames do not fit cap = %zu", d.size(), cap);
        err = buf;
        return CLX_API_ERROR;
    }
    for (size_t i = 0; i < d.size(); ++i) descs[i] = d[i];
    if (headers) for (size_t i = 0; i < h.size(); ++i) headers[i] = h[i];
    return CLX_OK;
}
