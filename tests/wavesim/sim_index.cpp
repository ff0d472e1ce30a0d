// TEST INFRASTRUCTURE: the segmented frame indexer (claxon_amd/csrc/clx_index.hip, unmodified) under the wave simulator: clx_idx_run,
// the body of clx_index_streams_device, over a device side that runs K8-K11 on host buffers.
// The authoritative header parser (clx_parse_frame_header of libclaxon_hip.so) is handed in by the caller.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <sys/mman.h>
#include <unistd.h>
#include <hip/hip_runtime.h>

#include "clx_kernels.hip"
#include "clx_index.hip"

static char sim_index_err[256];

extern "C" const char* sim_index_error(void) { return sim_index_err; }

// clx_idx_run's device side with host buffers in place of device ones
struct SimDev {
    const uint8_t* arena;
    std::vector<uint16_t> mask; std::vector<uint32_t> count, base;
    bool scan(const std::vector<clx_idx_stream>& tab, uint64_t chunk0, uint64_t n_chunks, uint32_t n_blocks, uint32_t* n_cand) {
        mask.assign(n_chunks, 0xa5a5u); count.assign(n_blocks, 0xa5a5a5a5u); base.assign(n_blocks + 1u, 0xa5a5a5a5u);
        SIM_LAUNCH(clx_k_idx_scan, n_blocks, 256, arena, (const clx_idx_stream*)tab.data(), (uint32_t)tab.size(), chunk0, n_chunks, mask.data(), count.data());
        SIM_LAUNCH(clx_k_idx_offsets, 1, 256, (const uint32_t*)count.data(), n_blocks, base.data());
        *n_cand = base[n_blocks];
        return true;
    }
    bool lists(const std::vector<clx_idx_stream>& tab, uint64_t chunk0, uint64_t n_chunks, uint32_t n_blocks, uint32_t n_cand,
               uint64_t* pos, uint32_t* sid, uint8_t* hdr, uint16_t* crc) {
        SIM_LAUNCH(clx_k_idx_compact, n_blocks, 256, arena, (const clx_idx_stream*)tab.data(), (uint32_t)tab.size(), chunk0, n_chunks,
                   (const uint16_t*)mask.data(), (const uint32_t*)base.data(), n_cand, pos, sid, hdr);
        SIM_LAUNCH(clx_k_idx_span_crc, n_cand, 64, arena, (const clx_idx_stream*)tab.data(), (const uint64_t*)pos, (const uint32_t*)sid, n_cand, crc);
        return true;
    }
};

// clx_index_streams_device with `arena` in host memory (16-byte aligned, readable up to round16(arena_len) + 32 bytes)
extern "C" int sim_index_streams(const uint8_t* arena, size_t arena_len, const uint64_t* offs, const uint64_t* lens, const uint64_t* starts,
                                 size_t n_streams, clx_frame_desc* descs, clx_frame_header* headers, size_t cap, uint64_t* first_frame,
                                 uint64_t* stop_offs, size_t* n_found, clx_idx_parse_fn parse) {
    SimDev dev{ arena };
    std::string err;
    const int st = clx_idx_run(dev, err, arena, arena_len, offs, lens, starts, n_streams, descs, headers, cap, first_frame, stop_offs, n_found, parse);
    if (st != CLX_OK) snprintf(sim_index_err, sizeof sim_index_err, "%s", err.c_str());
    return st;
}

// The same with the arena copied into a mapping whose padded end (round16(arena_len) + 32 bytes, what a device arena's allocation
// covers) sits flush against an inaccessible page: a load past it faults instead of reading a neighbour's bytes.
extern "C" int sim_index_guarded(const uint8_t* bytes, size_t arena_len, const uint64_t* offs, const uint64_t* lens, const uint64_t* starts,
                                 size_t n_streams, clx_frame_desc* descs, clx_frame_header* headers, size_t cap, uint64_t* first_frame,
                                 uint64_t* stop_offs, size_t* n_found, clx_idx_parse_fn parse) {
    const size_t padded = ((arena_len + 15) & ~(size_t)15) + 32;
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), body = (padded + pg - 1) / pg * pg;
    uint8_t* m = (uint8_t*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == (uint8_t*)MAP_FAILED) return -1;
    uint8_t* p = m + pg + body - padded;                  // (padded is a multiple of 16 and so is the page size: p is 16-byte aligned)
    memset(p, 0xff, padded);                              // (sync-looking padding: nothing behind a stream's end may count)
    memcpy(p, bytes, arena_len);
    mprotect(m, pg, PROT_NONE);
    mprotect(m + pg + body, pg, PROT_NONE);
    const int st = sim_index_streams(p, arena_len, offs, lens, starts, n_streams, descs, headers, cap, first_frame, stop_offs, n_found, parse);
    munmap(m, body + 2 * pg);
    return st;
}
