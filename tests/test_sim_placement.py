"""Where the decode writes, under the wave simulator: the production kernel sources decode placement_cases' workloads with the
blocks reversed, shuffled, spread by gaps, shifted off every alignment boundary and based on odd pointers, into sentinel-filled
buffers of which EVERY element is compared with the oracle's (placement_cases.check_placed).  The same cases run on the GPU in
test_gpu_placement.py."""
import ctypes as C

import numpy as np
import pytest

import claxon_amd as cx
import placement_cases as pl

FUSED = cx.PATH_LANES | cx.LANES_FUSED
SELECTIONS = {        # name -> (flags, output mode)
    "waves": (cx.PATH_WAVES | cx.K2_LATENCY, "planar"),
    "lanes-fused": (FUSED, "planar"),
    "lanes-general": (FUSED | cx.LANES_GENERAL, "planar"),
    "lanes-composed": (FUSED | cx.COMPOSE, "planar"),
    "pcm16": (FUSED | cx.OUT_PCM16, "pcm16"),
    "pcm24": (FUSED | cx.OUT_PCM24, "pcm24"),
    "f32": (cx.OUT_F32, "f32"),
}
# (composing needs windows of stereo frames; `lean24` is 24-bit audio but for a ragged wave of eight 16-bit frames: nothing for
#  CLX_OUT_PCM16 to lay out in every residue, and on the GPU, where the workload is whole, nothing at all)
CASES = [(wl, sel) for wl in pl.WORKLOADS for sel in SELECTIONS
         if (sel != "lanes-composed" or wl in pl.STEREO_WORKLOADS) and not (wl == "lean24" and sel == "pcm16")]


def sim_decode_into(flags, out_mode):
    """placement_cases' adapter for the simulator: the buffer is the caller's numpy array, d_out a view of it from `origin` on."""
    import simlib
    import simlib_f32

    def decode_into(arena, arena_len, descs, out_offs, buf, origin, verify_crc):
        view = buf[origin:]
        assert view.ctypes.data == buf.ctypes.data + origin * buf.itemsize and buf.ctypes.data % 256 == 0
        assert view.ctypes.data % buf.itemsize == 0 and (origin == pl.GUARD) == (view.ctypes.data % 16 == 0)      # (an odd base really is one)
        if out_mode != "f32":
            _, res, _ = simlib.decode(arena, arena_len, descs, out_offs, out=view, verify_crc=verify_crc, path=flags)
            return buf, res
        _, al = simlib_f32._aligned(arena)
        res = np.zeros(descs.size, dtype=cx.FRAME_RESULT_DTYPE)
        tiers = (C.c_uint64 * 2)()
        VP = C.c_void_p * 1
        st = simlib_f32.lib().sim_decode_frames_f32(VP(al.ctypes.data), arena_len, 1, descs.ctypes.data, descs.size, VP(view.ctypes.data),
                                                    out_offs.ctypes.data, VP(res.ctypes.data), (cx.VERIFY_CRC16 if verify_crc else 0) | flags, tiers)
        assert st == 0
        return buf, res
    return decode_into


@pytest.mark.parametrize("workload,selection", CASES, ids=["%s-%s" % c for c in CASES])
def test_sim_placed(oracle, workload, selection):
    """Every layout of one workload through one kernel selection; then once more, shuffled with gaps, with a third of the frames damaged."""
    flags, out_mode = SELECTIONS[selection]
    w = pl.for_mode(pl.WORKLOADS[workload](small=True), out_mode)
    decode_into = sim_decode_into(flags, out_mode)
    for name, out_offs, length, base_shift in pl.layouts(w):
        pl.check_placed(oracle, decode_into, w, out_offs, length, out_mode, base_shift, ctx="%s %s %s" % (workload, selection, name))
    arena = pl.damaged_for(oracle, w)
    _, out_offs, length, _ = pl.layout(w, "shuffled_gaps")
    r = pl.check_placed(oracle, decode_into, w, out_offs, length, out_mode, 0, arena=arena, ctx="%s %s damaged" % (workload, selection))
    pl.assert_damage_share(r, w.n)


def test_sim_placement_reaches_the_tiers(oracle):
    """The layouts that keep every block on 32 samples keep the tiers' groups: as many groups taken shuffled as back to back, in every
    output mode; one sample off, none."""
    import simlib
    stats = (C.c_uint64 * 64).in_dll(simlib.lib(), "sim_stats")
    for workload, sel in (("lean16", "lanes-fused"), ("lean16", "pcm16"), ("lean24", "lanes-fused"), ("lean24", "pcm24"), ("ms", "lanes-fused")):
        flags, out_mode = SELECTIONS[sel]
        w = pl.for_mode(pl.WORKLOADS[workload](small=True), out_mode)
        taken = {}
        for name, offs, length in (("back to back", w.out_offs, int(w.pcm.size)), ("aligned",) + pl.shuffled_aligned(w, 2), ("shifted",) + pl.shifted(w, 1)):
            for i in range(64):
                stats[i] = 0
            pl.check_placed(oracle, sim_decode_into(flags, out_mode), w, offs, length, out_mode, ctx="%s %s %s" % (workload, sel, name))
            taken[name] = int(stats[52]) + int(stats[13])
        assert taken["aligned"] == taken["back to back"] >= 2 and taken["shifted"] == 0, (workload, sel, taken)
