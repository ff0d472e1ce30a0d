"""CLX_OUT_F32 under the wave simulator (tests/wavesim/sim_f32.cpp): the float builds of the tiers (clx_k_lean_f32, clx_k_lean24_f32),
the general kernels' float rows (clx_narrow_row) and clx_k_interleave's CLX_SAMPLE_F32 form, bit for bit against the oracle's samples
through the contract's formula, statuses as the oracle's."""
import os

import numpy as np
import pytest

import claxon_amd as cx
import f32_cases as fc
import parity_cases as pc
import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")


@pytest.fixture(scope="module")
def sim():
    import simlib_f32
    simlib_f32.build()
    return simlib_f32


@pytest.mark.parametrize("extra", [cx.NO_COMPOSE, cx.COMPOSE], ids=["stream-order", "composed"])
def test_sim_f32_16_bit_tier(oracle, sim, extra):
    """Stereo 16-bit frames of every channel assignment, constant / verbatim subframes, lone last tiles, waves that give up, mono frames,
    three-channel frames and odd block sizes (the general kernels) -- with waves in stream order and composed by content."""
    w = pc.pcm16_workload()
    assert fc.check_f32(oracle, sim.SimF32Backend(extra), w) == w.n
    c = synth.config3(96)                                    # (the bench shape: the 16-bit tier writes the groups itself)
    _, tiers = sim.decode_runs([c.arena], c.arena_len, cx.descs_from_offsets(c.arena[:c.arena_len], c.offs, c.lens, check_crc=False)[0], c.out_offs, path=extra)
    assert tiers[0] == (2 * c.n + 63) // 64, tiers


def test_sim_f32_widths_and_lone_tiles(oracle, sim):
    """8-, 12- and 16-bit stereo frames in one wave (each row its own scale), mono frames with lone last tiles, intact and damaged."""
    w = fc.narrow_widths_workload()
    descs, _ = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)
    assert fc.check_f32(oracle, sim.SimF32Backend(), w) == w.n
    _, tiers = sim.decode_runs([w.arena], w.arena_len, descs, w.out_offs)
    assert tiers[0] >= (w.n - 80) // 32, tiers
    assert fc.check_f32(oracle, sim.SimF32Backend(), w, damage=0.2, seed=4) < w.n


def test_sim_f32_split_tier(oracle, sim):
    """24-bit stereo (config 4's shape), 16-bit groups of more than 12 taps, mono 24-bit, multichannel and odd frames, config 5."""
    w = fc.split_workload()
    descs, _ = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)
    assert fc.check_f32(oracle, sim.SimF32Backend(), w) == w.n
    _, tiers = sim.decode_runs([w.arena], w.arena_len, descs, w.out_offs)
    assert tiers[1] > tiers[0], tiers                       # (the split tier's float build took groups too)


def test_sim_f32_mid_side(oracle, sim):
    """Waves of plain mid/side pairs (the movers undo them before the conversion) in both tiers, and runaway mid/side streams (left to the
    general kernels; their out-of-range values convert by the same formula, no clamping)."""
    for w in (pc.ms_mover_workload(lone_tail=True), pc.ms_mover24_workload()):
        assert fc.check_f32(oracle, sim.SimF32Backend(), w) == w.n
    w, arena = pc.ms_wild_workload(bs=256)
    descs, _ = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)
    ((out, res),), _ = sim.decode_runs([arena], w.arena_len, descs, w.out_offs)
    ref, r = fc.reference(oracle, arena, w, check_crc=False)
    assert np.array_equal(np.asarray(res["status"]), r["statuses"])
    assert int(np.abs(ref.astype(np.int64)).max()) > (1 << 29)
    want = fc.f32_of_frames(ref, descs, w.out_offs, w.pcm.size)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_sim_f32_fixtures(oracle, sim):
    for name in ("non_subset.flac", "pop.flac", "wasted_bits.flac"):
        w = fc.fixture_workload("%s/%s" % (GOLDEN, name))
        assert fc.check_f32(oracle, sim.SimF32Backend(), w) == w.n, name


def test_sim_f32_truncations_and_bit_flips(oracle, sim):
    w = synth.concat("f32 damage", [synth.config3(48), synth.config4(12), synth.small_mixed(40)])
    assert fc.check_f32(oracle, sim.SimF32Backend(), w, truncate=0.3, seed=11) < w.n
    assert fc.check_f32(oracle, sim.SimF32Backend(), w, damage=0.3, seed=12) < w.n


def test_sim_f32_consecutive_runs(oracle, sim):
    """Runs of one planned batch on one set of scratch: an intact arena, a damaged one, the intact one again."""
    w = synth.concat("f32 runs", [synth.config3(40), synth.config4(8)])
    descs, _ = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)
    bad = w.arena.copy()
    rng = np.random.default_rng(5)
    for i in range(0, w.n, 3):
        pos = int(rng.integers(8 * (int(w.offs[i]) + 8), 8 * int(w.offs[i] + w.lens[i])))
        bad[pos >> 3] ^= 0x80 >> (pos & 7)
    runs, _ = sim.decode_runs([w.arena, bad, w.arena], w.arena_len, descs, w.out_offs, verify_crc=True)
    for arena, (out, res) in zip([w.arena, bad, w.arena], runs):
        ref, r = fc.reference(oracle, arena, w)
        assert np.array_equal(np.asarray(res["status"]), r["statuses"])
        ok = np.nonzero(r["statuses"] == cx.OK)[0]
        want = fc.f32_of_frames(ref, descs, w.out_offs, w.pcm.size)
        for i in ok:
            a, n = int(w.out_offs[i]), int(w.channels[i]) * int(w.block_sizes[i])
            assert np.array_equal(out[a:a + n].view(np.uint32), want[a:a + n].view(np.uint32)), int(i)


def test_sim_interleave_sample_f32(oracle):
    """clx_k_interleave's CLX_SAMPLE_F32 form (stereo pairs as one 8-byte store, everything else per sample) equals the formula."""
    import simlib
    w = synth.concat("f32 interleave", [synth.config3(6), synth.config4(3), synth.small_mixed(30)])
    descs, _ = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)
    ref, r = fc.reference(oracle, w.arena, w)
    assert np.all(r["statuses"] == cx.OK)
    pcm = simlib.interleave(ref, descs, w.out_offs, cx.SAMPLE_F32, pcm=np.zeros(4 * w.pcm.size + 8, dtype=np.uint8))[:4 * w.pcm.size]
    want = fc.f32_of_frames(ref, descs, w.out_offs, w.pcm.size)
    assert np.array_equal(pcm.view(np.uint32), want.view(np.uint32))


def test_plan_counts_f32_groups_left_for_certain(sim):
    """clx_plan_general_grid with CLX_OUT_F32: mono frames of more than 16 bits, multichannel frames and blocks off 32 bytes are left for
    certain; aligned 16- and 24-bit stereo is not."""
    w = synth.concat("plan", [synth.config4(64)])
    descs, _ = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)
    assert sim.general_sure(descs, w.out_offs, cx.OUT_F32) == 0
    assert sim.general_sure(descs, w.out_offs + np.uint64(4), cx.OUT_F32) == (2 * w.n + 63) // 64
    assert sim.general_sure(descs, w.out_offs + np.uint64(4), 0) == 0
    m = synth.small_mixed(60)
    dm, _ = cx.descs_from_offsets(m.arena[:m.arena_len], m.offs, m.lens, check_crc=False)
    assert sim.general_sure(dm, m.out_offs, cx.OUT_F32) >= sim.general_sure(dm, m.out_offs, 0)
