"""FLAC's outer limits under the wave simulator: blocks of 4 609 .. 65 535 samples (parity_cases.long_block_workload) and escape-coded
partitions / invalid residual headers (parity_cases.escape_workload), through every kernel selection, the narrow and float outputs,
consecutive runs on one scratch, pool tickets, truncations and bit flips -- against the oracle.  The GPU runs the same cases in
test_gpu_long_blocks.py."""
import ctypes as C

import numpy as np
import pytest

import claxon_amd as cx
import parity_cases as pc
from parity_util import SimBackend

LANES = cx.PATH_LANES | cx.LANES_FUSED


@pytest.fixture(scope="module")
def long_light():
    return pc.long_block_workload(light=True)


@pytest.fixture(scope="module")
def escapes():
    return pc.escape_workload()


def _stats():
    import simlib
    simlib.build()
    stats = (C.c_uint64 * 64).in_dll(simlib.lib(), "sim_stats")
    for i in range(64):
        stats[i] = 0
    return stats


@pytest.mark.parametrize("path", [cx.PATH_WAVES | cx.K2_LATENCY, cx.PATH_WAVES | cx.K2_THROUGHPUT, cx.PATH_WAVES, cx.PATH_LANES | cx.LANES_SPLIT,
                                  LANES, LANES | cx.LANES_GENERAL, LANES | cx.COMPOSE, LANES | cx.POOL],
                         ids=["waves", "waves-1w", "waves-mixed", "lanes", "lanes-fused", "lanes-general", "lanes-composed", "lanes-fused-pool"])
def test_sim_long_blocks_and_escapes(oracle, long_light, escapes, path):
    """Every selection of test_sim_parity.py.  The wave-per-frame selections (a wave per frame: the simulator's cost grows with every
    sample) take the 65 535- and 40 001-sample frames (waves) or the first alone (the other two); the lane selections the whole light
    workload.  Escapes: every frame reports
    what the reference reports, the first error in stream order."""
    if path & cx.PATH_LANES:
        w = long_light
    else:
        w = pc.subset(long_light, np.nonzero(long_light.block_sizes >= (40001 if path == cx.PATH_WAVES | cx.K2_LATENCY else 40002))[0])
    assert 40001 in w.block_sizes.tolist() or int(w.block_sizes.max()) == 65535
    st, _ = pc.check_against_oracle(oracle, SimBackend(path), w)
    assert np.all(st == cx.OK)
    pc.check_escape_kinds(escapes, *pc.check_against_oracle(oracle, SimBackend(path), escapes))


def test_sim_long_blocks_take_the_tiers(oracle):
    """The full workload (65 520-sample 16-bit and 32 768-sample 24-bit waves) on the fused lane build: the 16-bit tier and the split tier
    each take their long group, the general kernels the groups of 65 535 / 40 001 / 4 609 samples and the mixed ones."""
    w = pc.long_block_workload()
    stats = _stats()
    st, _ = pc.check_against_oracle(oracle, SimBackend(LANES), w)
    assert np.all(st == cx.OK)
    lean, split, left = int(stats[52]), int(stats[13]), int(stats[49])
    assert lean >= 1 and split >= 1 and left >= 2, (lean, split, left)      # groups: clx_k_lean | clx_k_lean24 | left to clx_k_lanes
    assert int(stats[50]) // 64 >= 2000, int(stats[50])                       # (lean turns: the 65 520-sample wave went through turn after turn)


def test_sim_escapes_take_the_tiers(oracle, escapes):
    """The escape families are the tiers' waves: the 16-bit tier and the split tier take groups that hold escapes, and an escape sends a
    lane to the slow turn (the tier counter "partition edge inside a four / escape")."""
    stats = _stats()
    pc.check_escape_kinds(escapes, *pc.check_against_oracle(oracle, SimBackend(LANES), escapes))
    assert int(stats[52]) >= 1 and int(stats[13]) >= 1 and int(stats[53]) > 0, (int(stats[52]), int(stats[13]), int(stats[53]))


@pytest.mark.parametrize("out", ["pcm16", "pcm24", "f32"])
def test_sim_long_blocks_and_escapes_narrow_outputs(oracle, long_light, escapes, out):
    """CLX_OUT_PCM16 / CLX_OUT_PCM24 / CLX_OUT_F32: the tiers' own stores for long rows, the general kernels' staging rows (as long as the
    batch's largest block: 65 535) for the rest; exact bytes of every OK frame, the reference's verdict for every broken one."""
    if out == "f32":
        import simlib_f32
        backend = simlib_f32.SimF32Backend()
    else:
        backend = SimBackend(LANES | (cx.OUT_PCM16 if out == "pcm16" else cx.OUT_PCM24))
    stats = _stats()
    st, _ = pc.check_against_oracle(oracle, backend, pc.for_output(long_light, out), out=out)
    assert np.all(st == cx.OK)
    if out != "f32":
        assert int(stats[49]) >= 2, int(stats[49])                  # groups the general kernels narrowed from their staging rows
    e = pc.for_output(escapes, out)
    pc.check_escape_kinds(e, *pc.check_against_oracle(oracle, backend, e, out=out))


def test_sim_long_blocks_and_escapes_runs_and_pool(oracle, long_light, escapes):
    """Consecutive runs of one planned batch on one scratch, and pool tickets of one merged launch: runs whose long frames are intact,
    damaged, or where the escapes sit."""
    import simlib
    simlib.build()
    w = pc.subset(long_light, list(range(32)) + list(np.nonzero(long_light.channels >= 3)[0]))
    w = pc.synth.concat("long + escapes", [w, escapes])
    descs, _ = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)
    rng = np.random.default_rng(64)
    bad = w.arena.copy()
    for i in range(0, 40, 3):
        lo, hi = int(w.offs[i]) + int(descs["header_bytes"][i]), int(w.offs[i] + w.lens[i])
        pos = int(rng.integers(8 * lo, 8 * hi))
        bad[pos >> 3] ^= 0x80 >> (pos & 7)
    arenas = [w.arena.copy(), bad, w.arena.copy()]
    refs = []
    for a in arenas:
        ref = np.full(w.pcm.size, 0x31313131, dtype=np.int32)
        refs.append((ref, oracle.decode_batch(a[:w.arena_len], w.offs, w.lens, out=ref, out_offs=w.out_offs, check_crc=True)))
    runs = simlib.decode_runs(arenas, w.arena_len, descs, w.out_offs, verify_crc=True, fill=0x31313131, path=LANES)
    pooled, _ = simlib.decode_pool(arenas, w.arena_len, descs, w.out_offs, verify_crc=True, fill=0x31313131, path=LANES | cx.NO_COMPOSE | cx.POOL)
    for name, got in (("runs", runs), ("pool", pooled)):
        for k, ((out, res), (ref, r)) in enumerate(zip(got, refs)):
            assert np.array_equal(res["status"], r["statuses"]) and np.array_equal(res["msg"], r["msgs"]), (name, k)
            ok = np.nonzero(res["status"] == cx.OK)[0]
            assert np.array_equal(res["end_bit"][ok], r["end_bits"][ok]), (name, k)
            for i in ok:
                lo, hi = int(w.out_offs[i]), int(w.out_offs[i]) + int(w.channels[i]) * int(w.block_sizes[i])
                assert np.array_equal(out[lo:hi], ref[lo:hi]), (name, k, int(i))
            assert int(np.sum(res["msg"] == pc.MSG["CLX_MSG_UNENCODED_BINARY"])) >= 40
        assert int(np.sum(got[1][1]["status"] != cx.OK)) > int(np.sum(got[0][1]["status"] != cx.OK))


def test_sim_long_and_escape_truncations_and_flips(oracle, long_light, escapes):
    """Every cut and flip of a few long frames (multichannel, 8 .. 24 bits) and of escape / bad-residual frames gives the reference's
    status, message, end bit and samples."""
    sim = SimBackend(LANES)
    long_idx = [i for i in range(long_light.n) if long_light.channels[i] > 2 and long_light.block_sizes[i] <= 8192][:2]
    esc_idx = [i for i, k in enumerate(escapes.kinds) if k != "ok"][:6]
    frames = pc.frames_of(long_light, long_idx) + pc.frames_of(escapes, esc_idx)
    seen = pc.check_truncations(oracle, sim, cuts_per_frame=4, seed=31, frames=frames)
    assert (cx.IO_ERROR, pc.MSG["CLX_MSG_UNEXPECTED_EOF"]) in seen and (cx.UNSUPPORTED, pc.MSG["CLX_MSG_UNENCODED_BINARY"]) in seen, seen
    seen = pc.check_bitflips(oracle, sim, trials=4, seed=32, frames=frames)
    assert len(seen) >= 3, seen
