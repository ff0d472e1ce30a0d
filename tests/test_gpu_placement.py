"""Where the decode writes, on the GPU: placement_cases' workloads and layouts (blocks reversed, shuffled, spread by gaps, shifted off
every alignment boundary, based on odd pointers) through Context.plan(...).run, pipelined submissions, the interleave stage and the
host-to-host stream decode -- every element of every sentinel-filled buffer against the oracle's (placement_cases.check_placed) --
and blocks more than 4 GiB apart.  The simulator runs the same matrix in test_sim_placement.py."""
import numpy as np
import pytest

import claxon_amd as cx
import f32_cases as fc
import parity_cases as pc
import placement_cases as pl

pytestmark = pytest.mark.gpu

FUSED = cx.PATH_LANES | cx.LANES_FUSED
SELECTIONS = {        # name -> (flags, output mode): test_gpu_parity's six planar selections, then the narrow outputs
    "waves": (cx.PATH_WAVES | cx.K2_LATENCY, "planar"),
    "waves-1w": (cx.PATH_WAVES | cx.K2_THROUGHPUT, "planar"),
    "lanes": (cx.PATH_LANES | cx.LANES_SPLIT, "planar"),
    "lanes-fused": (FUSED, "planar"),
    "lanes-general": (FUSED | cx.LANES_GENERAL, "planar"),
    "lanes-composed": (FUSED | cx.COMPOSE, "planar"),
    "pcm16": (cx.OUT_PCM16, "pcm16"),
    "pcm24": (cx.OUT_PCM24, "pcm24"),
    "f32": (cx.OUT_F32, "f32"),
    "pcm16-pool": (cx.OUT_PCM16 | cx.POOL, "pcm16"),
}
# (composing needs windows of stereo frames; `lean24` holds no frame of at most 16 bits for CLX_OUT_PCM16 to take)
CASES = [(wl, sel) for wl in pl.WORKLOADS for sel in SELECTIONS
         if (sel != "lanes-composed" or wl in pl.STEREO_WORKLOADS) and not (wl == "lean24" and SELECTIONS[sel][1] == "pcm16")]
SIGNED = {1: np.int8, 2: np.int16, 4: np.int32}


@pytest.fixture(scope="module")
def ctx():
    c = cx.Context(0, wait_s=120)
    yield c
    c.close()


def to_device(bits):
    """A numpy array of unsigned elements as a device tensor of the signed type of the same width (torch has no uint16 / uint32)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(SIGNED[bits.dtype.itemsize])).to("cuda:0")


def gpu_decode_into(ctx, flags):
    """placement_cases' adapter for the GPU: the sentinels go into a device tensor, d_out is its address plus `origin` elements."""
    import torch

    def decode_into(arena, arena_len, descs, out_offs, buf, origin, verify_crc):
        d_arena = torch.from_numpy(np.ascontiguousarray(arena)).to("cuda:0")
        d_buf = to_device(buf)
        assert d_buf.data_ptr() % 256 == 0
        batch = ctx.plan(descs, out_offs, verify_crc=verify_crc, path=flags)
        torch.cuda.synchronize()
        batch.run(d_arena.data_ptr(), int(arena_len), d_buf.data_ptr() + origin * buf.itemsize)
        res = batch.results()
        got = d_buf.cpu().numpy()
        batch.close()
        return got, res
    return decode_into


@pytest.mark.parametrize("workload,selection", CASES, ids=["%s-%s" % c for c in CASES])
def test_gpu_placed(oracle, ctx, workload, selection):
    """Every layout of one workload through one kernel selection; then once more, shuffled with gaps, with a third of the frames damaged."""
    flags, out_mode = SELECTIONS[selection]
    w = pl.for_mode(pl.WORKLOADS[workload](), out_mode)
    decode_into = gpu_decode_into(ctx, flags)
    for name, out_offs, length, base_shift in pl.layouts(w):
        pl.check_placed(oracle, decode_into, w, out_offs, length, out_mode, base_shift, ctx="%s %s %s" % (workload, selection, name))
    arena = pl.damaged_for(oracle, w)
    _, out_offs, length, _ = pl.layout(w, "shuffled_gaps")
    r = pl.check_placed(oracle, decode_into, w, out_offs, length, out_mode, 0, arena=arena, ctx="%s %s damaged" % (workload, selection))
    pl.assert_damage_share(r, w.n)


@pytest.mark.parametrize("lay", ["shuffled_aligned", "shifted(1)"])
@pytest.mark.parametrize("workload", ["lean16", "lean24"])
def test_gpu_placed_pipelined(oracle, ctx, workload, lay):
    """13 submissions into 13 sentinel-filled buffers (one merged launch of 12 and a remainder), then a flush: every buffer whole."""
    import torch
    w = pl.WORKLOADS[workload]()
    _, out_offs, length, base_shift = pl.layout(w, lay)
    before, after, masked, origin = pl.expected_buffer(oracle, w, out_offs, length, "planar", base_shift)
    _, r = pl.reference(oracle, w)
    descs = pc.workload_descs(w)
    d_arena = torch.from_numpy(w.arena).to("cuda:0")
    bufs = [to_device(before) for _ in range(13)]
    batch = ctx.plan(descs, out_offs, verify_crc=True)
    assert batch.submit_lanes and batch.submit_merge == 12
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for b in bufs:
        batch.submit(d_arena.data_ptr(), w.arena_len, b.data_ptr() + origin * 4, st)
    batch.flush(st)
    torch.cuda.synchronize()
    pl.check_results(w, r, batch.results(), "%s %s pipelined" % (workload, lay))
    for k, b in enumerate(bufs):
        pl.compare(w, out_offs, "planar", origin, b.cpu().numpy(), after, masked, "%s %s submission %d" % (workload, lay, k))
    batch.close()


def pcm_block(v, c, bs, bps, sample_bytes):
    """A frame's planar samples as the interleave stage's bytes."""
    if sample_bytes == cx.SAMPLE_F32:
        return fc.to_f32(v.reshape(c, bs).T.reshape(-1), bps).view(np.uint8)
    if sample_bytes == 4:
        return np.ascontiguousarray(v.reshape(c, bs).T.reshape(-1)).astype("<i4").view(np.uint8)
    return pc.block_in_mode(v, c, bs, bps, {2: "pcm16", 3: "pcm24"}[sample_bytes]).view(np.uint8)


@pytest.mark.parametrize("sample_bytes", [2, 3, 4, cx.SAMPLE_F32], ids=["2", "3", "4", "f32"])
@pytest.mark.parametrize("lay", ["shifted(1)", "odd_base(1)"])
def test_gpu_interleave_placed(oracle, ctx, lay, sample_bytes):
    """Batch.interleave and Context.interleave write the blocks of OK frames and nothing else: guards and gaps keep the sentinel, and so
    -- the failed frames are skipped, no mask here -- do the blocks of failed frames.  odd_base: the `pcm` pointer is one element
    (a sample; a byte for 3-byte samples) off the allocation."""
    import torch
    w = pl.WORKLOADS["general"]()
    arena = pl.damaged_for(oracle, w)
    ref, r = pl.reference(oracle, w, arena)
    _, out_offs, length, k = pl.layout(w, lay)
    sb = 4 if sample_bytes == cx.SAMPLE_F32 else sample_bytes
    elem = 1 if sb == 3 else sb
    origin = (pl.GUARD + k) * elem                                   # in bytes
    n = origin + sb * length + pl.GUARD * elem
    before = pl.sentinels(n, "pcm24")
    after = before.copy()
    planar = np.full(length, 0x6b6b6b6b, dtype=np.int32)            # the planar side: the oracle's samples at the same offsets
    for i in range(w.n):
        a, c, bs = int(w.out_offs[i]), int(w.channels[i]), int(w.block_sizes[i])
        if int(r["statuses"][i]) == cx.OK:
            planar[int(out_offs[i]):int(out_offs[i]) + c * bs] = ref[a:a + c * bs]
            after[origin + sb * int(out_offs[i]):origin + sb * (int(out_offs[i]) + c * bs)] = pcm_block(ref[a:a + c * bs], c, bs, w.bps[i], sample_bytes)

    def same(got, what):
        bad = np.nonzero(np.asarray(got).view(np.uint8) != after)[0]
        assert bad.size == 0, "%s: %d bytes differ, the first at byte %d (pcm%+d): %s" % (
            what, bad.size, int(bad[0]), int(bad[0]) - origin, pl.where(w, out_offs, "planar", 0, (int(bad[0]) - origin) // sb) if int(bad[0]) >= origin else "the front guard")

    descs = pc.workload_descs(w)
    # Batch.interleave behind a run of the damaged arena: the run's own results say which frames to skip
    d_arena = torch.from_numpy(arena).to("cuda:0")
    d_planar = torch.full((length,), 0x5c5c5c5c, dtype=torch.int32, device="cuda:0")
    d_pcm = to_device(before)
    batch = ctx.plan(descs, out_offs, verify_crc=True)
    torch.cuda.synchronize()
    batch.run(d_arena.data_ptr(), w.arena_len, d_planar.data_ptr())
    batch.interleave(d_planar.data_ptr(), d_pcm.data_ptr() + origin, sample_bytes)
    pl.check_results(w, r, batch.results(), "interleave")
    torch.cuda.synchronize()
    same(d_pcm.cpu().numpy(), "Batch.interleave %s" % lay)
    batch.close()
    # Context.interleave on host arrays with the oracle's statuses as `results`
    res = np.zeros(w.n, dtype=cx.FRAME_RESULT_DTYPE)
    res["status"] = r["statuses"]
    host = pl.aligned_array(n, np.uint8)
    host[:] = before
    view = host[origin:origin + sb * length]
    ctx.interleave(planar, descs, out_offs, sample_bytes, results=res, pcm=view.view(np.float32) if sample_bytes == cx.SAMPLE_F32 else view)
    same(host, "Context.interleave %s" % lay)


@pytest.mark.parametrize("sample_bytes", [0, 2])
def test_gpu_stream_decode_placed(oracle, ctx, sample_bytes):
    """clx_decode_frames_stream with gaps between the blocks (increasing order, as it demands), several chunks: OK frames' samples,
    zeros for failed frames -- exactly, no mask -- and zeros in every gap between the first block and the last (claxon_hip.h: the
    span is written whole); what lies in front of the first block and behind the last keeps the sentinel."""
    w = pl.WORKLOADS["general"]()
    arena = pl.damaged_for(oracle, w)
    ref, r = pl.reference(oracle, w, arena)
    out_offs, length = pl.shuffled_gaps(w, 5, increasing=True)
    mode = "planar" if sample_bytes == 0 else "pcm16"
    # (sample_bytes 2: the narrow stage keeps the low 16 bits of wider samples too -- block_in_mode's formula)
    origin = pl.GUARD
    before = pl.sentinels(origin + length + pl.GUARD, mode)
    after = before.copy()
    first, last = int(out_offs[0]), int(out_offs[-1]) + int(w.channels[-1]) * int(w.block_sizes[-1])
    after[origin + first:origin + last] = 0
    for i in range(w.n):
        a, c, bs = int(w.out_offs[i]), int(w.channels[i]), int(w.block_sizes[i])
        if int(r["statuses"][i]) == cx.OK:
            after[origin + int(out_offs[i]):origin + int(out_offs[i]) + c * bs] = pc.block_in_mode(ref[a:a + c * bs], c, bs, w.bps[i], mode).view(before.dtype)
    descs = pc.workload_descs(w)
    for chunk in (50, 0):
        ctx.set_stream_chunk(chunk)
        host = pl.aligned_array(before.size, before.dtype)
        host[:] = before
        view = host[origin:origin + length]
        _, res = ctx.decode_frames_stream(arena[:w.arena_len], descs, out_offs, out=view.view(np.int32) if sample_bytes == 0 else view.view(np.uint8),
                                          sample_bytes=sample_bytes, verify_crc=True)
        pl.check_results(w, r, res, "stream")
        pl.compare(w, out_offs, mode, origin, host, after, np.zeros(after.size, dtype=bool), "stream decode, sample_bytes %d, chunk %d" % (sample_bytes, chunk))
    ctx.set_stream_chunk(0)


def _count_not(t, fill, chunk=1 << 28):
    """How many elements of a device tensor differ from `fill`, counted on the device chunk by chunk."""
    n = 0
    for lo in range(0, t.numel(), chunk):
        n += int((t[lo:lo + chunk] != fill).sum())
    return n


def test_gpu_blocks_far_apart(oracle, ctx):
    """(a) planar, a buffer of 4 GiB + 64 MiB, through the fused lane kernels (asked for by flag: a batch this small would otherwise go to
    the wave kernels) and through the wave kernels: one wave's rows half in front of and half behind the 4 GiB mark (clx_k_lean's exit
    for rows more than 4 GiB from the wave's lowest: the general kernels take the group), one wave wholly behind it (the tier, on a
    64-bit base).  (b) CLX_OUT_PCM16 (always the fused lane kernels), a buffer of 8 GiB + 64 MiB: a wave at a sample offset beyond 2^32
    on 32 samples (the tier) and one a sample off (the general kernels' narrow rows) -- an offset cut to 32 bits lands in the first
    64 MiB.  Blocks against the oracle on the host; everything else must still hold the fill, counted on the device."""
    import torch
    MiB = 1 << 20
    big = (1 << 33) + 64 * MiB
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * big:             # (decided before any work: the test runs whole or not at all)
        pytest.skip("%.1f GiB free on the device, the test wants three times its largest buffer of %.1f GiB" % (free / 2.0 ** 30, big / 2.0 ** 30))
    w = pl._families(pc.lean_workload(), [(2, 1024, None, 64)])
    ref, r = pl.reference(oracle, w)
    assert np.all(r["statuses"] == cx.OK)
    descs = pc.workload_descs(w)
    d_arena = torch.from_numpy(w.arena).to("cuda:0")
    size = 2 * 1024
    offs_a = np.zeros(w.n, dtype=np.uint64)                    # (a): in int32 elements; the 4 GiB mark is element 2^30
    offs_a[0:16] = 64 + size * np.arange(16)
    offs_a[16:32] = (1 << 30) + 4096 + size * np.arange(16)
    offs_a[32:64] = (1 << 30) + 4 * MiB + size * np.arange(32)
    offs_b = np.zeros(w.n, dtype=np.uint64)                    # (b): in int16 elements, beyond element 2^32
    offs_b[0:32] = (1 << 32) + 2 * MiB + size * np.arange(32)
    offs_b[32:64] = (1 << 32) + 8 * MiB + 1 + size * np.arange(32)
    cases = [("planar", (1 << 32) + 64 * MiB, [("lanes-fused", FUSED), ("waves", cx.PATH_WAVES | cx.K2_LATENCY)], offs_a, 0x0badf00d),
             ("pcm16", big, [("pcm16", cx.OUT_PCM16)], offs_b, 0x5eed)]
    for mode, nbytes, selections, offs, fill in cases:
        raw = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        buf = raw.view(torch.int32 if mode == "planar" else torch.int16)
        assert int(offs.max()) + size <= buf.numel()
        for name, flags in selections:
            what = "far apart, %s %s" % (mode, name)
            buf.fill_(fill)
            batch = ctx.plan(descs, offs, verify_crc=True, path=flags)
            torch.cuda.synchronize()
            batch.run(d_arena.data_ptr(), w.arena_len, buf.data_ptr())
            pl.check_results(w, r, batch.results(), what)
            batch.close()
            for i in range(w.n):
                a, o = int(w.out_offs[i]), int(offs[i])
                got = buf[o:o + size].cpu().numpy()
                want = pc.block_in_mode(ref[a:a + size], 2, 1024, 16, mode)
                assert np.array_equal(got, want), "%s: frame %d at offset %d" % (what, i, o)
                buf[o:o + size] = fill
            stray = _count_not(buf, fill)
            assert stray == 0, "%s: %d elements outside the blocks were written" % (what, stray)
        del buf, raw
        torch.cuda.empty_cache()
