// TEST INFRASTRUCTURE: the float output (CLX_OUT_F32) of the lane path under the wave simulator.  sim_lib.cpp launches the integer
// builds of the tiers; this unit plans a batch the same way (its SimLanes) and launches what the library launches for a float batch
// (launch_lanes, clx_api.hip): the scan, clx_k_compose, clx_k_lean_f32, clx_k_lean24_f32, clx_k_left, the general kernels into staging
// rows of their own, clx_k_finalize, the CRC.
#include "sim_lib.cpp"

namespace {

// one run of the planned batch `L` (SimLanes::make_run's scratch handling) with the float kernels
int run_f32(SimLanes& L, const uint8_t* arena, size_t arena_len, float* out, clx_frame_result* results, uint64_t* tier_groups) {
    clx_runs runs;
    memset(&runs, 0, sizeof runs);
    runs.r[0] = L.make_run(arena, arena_len, reinterpret_cast<int32_t*>(out), results);
    runs.r[0].flags |= CLX_RUN_F32;
    const size_t groups = (L.n_slots + 63) / 64;
    if (L.n_multi) SIM_LAUNCH(clx_k_scan, (L.n_multi + 63) / 64, 64, runs, L.dev.data(), L.multi.data(), (uint32_t)L.n_multi);
    if (L.n_windows && L.n_multi) SIM_LAUNCH(clx_k_compose, L.n_windows, CLX_COMPOSE_THREADS, runs, L.windows.data());
    std::vector<int32_t> dump(((L.n_slots + 127) / 128) * 128 * 32 + 16);
    bool any_le16 = false;
    for (size_t i = 0; i < L.n; ++i) any_le16 = any_le16 || L.dev[i].bps <= 16u;
    if (any_le16) SIM_LAUNCH(clx_k_lean_f32, groups, 64, runs, L.dev.data(), (uint32_t)L.n_slots, dump.data());
    for (size_t g = 0; g < groups; ++g) tier_groups[0] += L.taken[g] == runs.r[0].gen;
    SIM_LAUNCH(clx_k_lean24_f32, groups, 64, runs, L.dev.data(), (uint32_t)L.n_slots, dump.data());
    for (size_t g = 0; g < groups; ++g) tier_groups[1] += L.taken[g] == runs.r[0].gen;
    SIM_LAUNCH(clx_k_left, (groups + 255) / 256, 256, runs, (uint32_t)groups, (uint32_t*)nullptr, (uint32_t*)nullptr);
    const uint32_t n_left = L.taken[groups];
    if (n_left > groups) return CLX_API_ERROR;
    const size_t ggrid = n_left >= 3 ? n_left / 3 : 1;       // (fewer workgroups than groups left: every one loops over several)
    clx_runs gruns = runs;
    L.planar.assign(ggrid * 64 * (size_t)L.stage_stride + 16, 0x2b2b2b2b);
    gruns.r[0].planar = L.planar.data();
    gruns.r[0].flags |= CLX_RUN_STAGE_BITS(L.stage_stride);
    SIM_LAUNCH(clx_k_lanes, ggrid, 64, gruns, L.dev.data(), (uint32_t)L.n_slots, dump.data());
    SIM_LAUNCH(clx_k_lanes_hi, ggrid, 64, gruns, L.dev.data(), (uint32_t)L.n_slots, dump.data());
    SIM_LAUNCH(clx_k_finalize, (L.n + 255) / 256, 256, runs, L.dev.data(), (uint32_t)L.n, (uint32_t)L.n_slots);
    if (L.taken[groups] != 0u) return CLX_API_ERROR;          // (the list is left empty for the next run)
    for (size_t i = 0; i < L.n; ++i) if (L.errkey[i] != 0xffffffffu) return CLX_API_ERROR;
    for (uint64_t s = 0; s < L.n_slots; ++s) if (L.sf_start[s] != 0xffffffffu) return CLX_API_ERROR;
    if (L.flags & CLX_VERIFY_CRC16) SIM_LAUNCH(clx_k_crc16_runs, (L.n + 3) / 4, 256, runs, L.dev.data(), (uint32_t)L.n);
    return CLX_OK;
}

}  // namespace

// Consecutive runs of ONE planned float batch on ONE set of scratch: run r decodes arenas[r] into outs[r] / results[r].  flags: the
// ABI's, CLX_OUT_F32 among them (the fused lane build is implied, as batch_plan_ does).  tier_groups: groups of 64 slots the 16-bit
// tier took, then the two tiers together, summed over the runs.
extern "C" int sim_decode_frames_f32(const uint8_t* const* arenas, size_t arena_len, size_t n_runs, const clx_frame_desc* frames, size_t n,
                                     float* const* outs, const uint64_t* out_offs, clx_frame_result* const* results, uint32_t flags,
                                     uint64_t* tier_groups) {
    if (!(flags & CLX_OUT_F32) || (flags & (CLX_OUT_PCM16 | CLX_OUT_PCM24 | CLX_PATH_WAVES | CLX_LANES_SPLIT | CLX_LANES_GENERAL))) return CLX_API_ERROR;
    flags |= CLX_PATH_LANES | CLX_LANES_FUSED;
    SimLanes L;
    if (!L.plan(frames, n, out_offs, arena_len, flags)) return CLX_API_ERROR;
    uint32_t bs_max = 1;
    for (size_t i = 0; i < n; ++i) bs_max = std::max<uint32_t>(bs_max, frames[i].block_size);
    L.stage_stride = (bs_max + 3u) & ~3u;
    tier_groups[0] = tier_groups[1] = 0;
    for (size_t r = 0; r < n_runs; ++r) {
        const int st = run_f32(L, arenas[r], arena_len, outs[r], results[r], tier_groups);
        if (st != CLX_OK) return st;
    }
    return CLX_OK;
}

// the plan's rule for the general kernels' grid (clx_plan_general_grid) with the batch's flags: the groups left for certain
extern "C" uint64_t sim_general_sure(const clx_frame_desc* frames, size_t n, const uint64_t* out_offs, uint32_t flags) {
    std::vector<clx_dev_frame> dev(n ? n : 1);
    uint64_t n_slots = 0;
    if (clx_plan_frames(frames, n, out_offs, dev.data(), &n_slots) >= 0) return ~0ull;
    std::vector<uint32_t> slot_frame(n_slots ? n_slots : 1), multi(n ? n : 1);
    clx_plan_lanes(dev.data(), n, n_slots, slot_frame.data(), multi.data());
    uint64_t sure = 0;
    clx_plan_general_grid(dev.data(), slot_frame.data(), n_slots, flags, &sure);
    return sure;
}
