"""CLX_OUT_F32 / CLX_SAMPLE_F32 and the whole-stream loaders on the GPU: the simulator's families (test_f32_output.py) on the device,
pipelined submissions over distinct arenas (merged launches), the wave path and the host pipeline with CLX_SAMPLE_F32 against the
fused output, claxon_amd.load / load_batch against the STREAMINFO MD5, and the refused flag combinations."""
import hashlib
import os

import numpy as np
import pytest

import claxon_amd as cx
import f32_cases as fc
import parity_cases as pc
import synth
from parity_util import GpuBackend

pytestmark = pytest.mark.gpu
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")
MD5 = {"pop.flac": "68464288fa5e19835516972dcf47223c", "short.flac": "927598b89c89c1129a152eecfc14075e",
       "wasted_bits.flac": "4fbca4cf30f188453c0676e0cd700c71"}


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _descs(w):
    return cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)[0]


@pytest.mark.parametrize("extra", [cx.NO_COMPOSE, cx.COMPOSE], ids=["stream-order", "composed"])
def test_gpu_f32_families(oracle, ctx, extra):
    g = GpuBackend(ctx, cx.OUT_F32 | extra)
    for w in (pc.pcm16_workload(), fc.narrow_widths_workload(), fc.split_workload(), pc.ms_mover_workload(lone_tail=True), pc.ms_mover24_workload()):
        assert fc.check_f32(oracle, g, w) == w.n, w.name
    w = fc.narrow_widths_workload()
    assert fc.check_f32(oracle, g, w, damage=0.2, seed=4) < w.n


def test_gpu_f32_runaway_mid_side_fixtures_and_damage(oracle, ctx):
    g = GpuBackend(ctx, cx.OUT_F32)
    w, arena = pc.ms_wild_workload(bs=256)
    descs = _descs(w)
    out, res = g.decode(arena, w.arena_len, descs, w.out_offs, False)
    ref, r = fc.reference(oracle, arena, w, check_crc=False)
    assert np.array_equal(np.asarray(res["status"]), r["statuses"])
    want = fc.f32_of_frames(ref, descs, w.out_offs, w.pcm.size)
    assert np.array_equal(np.asarray(out).view(np.uint32), want.view(np.uint32))
    for name in ("non_subset.flac", "pop.flac", "wasted_bits.flac"):
        wf = fc.fixture_workload(os.path.join(FIXTURES, name))
        assert fc.check_f32(oracle, g, wf) == wf.n, name
    w = synth.concat("f32 damage", [synth.config3(64), synth.config4(16), synth.small_mixed(40)])
    assert fc.check_f32(oracle, g, w, truncate=0.3, seed=11) < w.n
    assert fc.check_f32(oracle, g, w, damage=0.3, seed=12) < w.n


def test_gpu_f32_pipelined_submissions(oracle, ctx):
    """submit_depth submissions over distinct arenas (every third one damaged) and distinct outputs: merged launches of the float tiers."""
    import torch
    w = synth.concat("f32 submit", [synth.config3(300), synth.config4(40)])
    descs = _descs(w)
    batch = ctx.plan(descs, w.out_offs, verify_crc=True, path=cx.OUT_F32)
    depth = batch.submit_depth
    assert batch.submit_lanes and depth > 1
    rng = np.random.default_rng(8)
    arenas = []
    for k in range(depth):
        a = w.arena.copy()
        if k % 3 == 1:
            for i in range(0, w.n, 7):
                pos = int(rng.integers(8 * (int(w.offs[i]) + 8), 8 * int(w.offs[i] + w.lens[i])))
                a[pos >> 3] ^= 0x80 >> (pos & 7)
        arenas.append(a)
    d_arenas = [torch.from_numpy(a).cuda() for a in arenas]
    outs = [torch.full((w.pcm.size,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(depth)]
    torch.cuda.synchronize()
    for k in range(depth):
        batch.submit(d_arenas[k].data_ptr(), w.arena_len, outs[k].data_ptr())
    batch.flush()
    torch.cuda.synchronize()
    for k in (0, 1, depth - 1):
        ref, r = fc.reference(oracle, arenas[k], w)
        want = fc.f32_of_frames(ref, descs, w.out_offs, w.pcm.size)
        got = outs[k].cpu().numpy()
        for i in np.nonzero(r["statuses"] == cx.OK)[0]:
            a, n = int(w.out_offs[i]), int(w.channels[i]) * int(w.block_sizes[i])
            assert np.array_equal(got[a:a + n].view(np.uint32), want[a:a + n].view(np.uint32)), (k, int(i))
    res = batch.results()
    assert np.array_equal(np.asarray(res["status"]), fc.reference(oracle, arenas[depth - 1], w)[1]["statuses"])
    batch.close()


def test_gpu_sample_f32_matches_the_fused_output(oracle, ctx):
    """The wave path + clx_batch_interleave(CLX_SAMPLE_F32), and clx_decode_frames_stream(CLX_SAMPLE_F32), give the fused output's floats."""
    import torch
    w = synth.concat("f32 forms", [synth.config3(40), synth.config4(8), synth.small_mixed(30)])
    descs = _descs(w)
    fused, res = GpuBackend(ctx, cx.OUT_F32).decode(w.arena, w.arena_len, descs, w.out_offs, True)
    assert np.all(res["status"] == cx.OK)
    fused = np.asarray(fused).view(np.float32)
    d_arena = torch.from_numpy(w.arena).cuda()
    d_out = torch.zeros(w.pcm.size, dtype=torch.int32, device="cuda")
    d_pcm = torch.zeros(w.pcm.size, dtype=torch.float32, device="cuda")
    batch = ctx.plan(descs, w.out_offs, verify_crc=True, path=cx.PATH_WAVES)
    torch.cuda.synchronize()
    batch.run(d_arena.data_ptr(), w.arena_len, d_out.data_ptr())
    batch.interleave(d_out.data_ptr(), d_pcm.data_ptr(), cx.SAMPLE_F32)
    assert np.all(batch.results()["status"] == cx.OK)
    assert np.array_equal(d_pcm.cpu().numpy().view(np.uint32), fused.view(np.uint32))
    batch.close()
    out, res = ctx.decode_frames_stream(w.arena[:w.arena_len], descs, w.out_offs, sample_bytes=cx.SAMPLE_F32, verify_crc=True)
    assert out.dtype == np.float32 and np.all(res["status"] == cx.OK)
    assert np.array_equal(out.view(np.uint32), fused.view(np.uint32))
    ref, _ = fc.reference(oracle, w.arena, w)
    host = ctx.interleave(ref, descs, w.out_offs, cx.SAMPLE_F32)
    assert host.dtype == np.float32 and np.array_equal(host.view(np.uint32), fused.view(np.uint32))


def test_gpu_load_md5(ctx):
    """load: scaled back to integers (exact), packed at ceil(bps / 8) bytes, the MD5 is STREAMINFO's."""
    for name, md5 in MD5.items():
        data = open(os.path.join(FIXTURES, name), "rb").read()
        x, rate = cx.load(ctx, data)
        st, _, si, _ = cx.read_stream_header(np.frombuffer(data, dtype=np.uint8))
        assert x.dtype.is_floating_point and x.is_cuda and tuple(x.shape) == (int(si.samples), int(si.channels)) and rate == si.sample_rate
        bps = int(si.bits_per_sample)
        v = (x.cpu().numpy().astype(np.float64) * 2.0 ** (bps - 1))
        assert np.all(v == np.round(v)) and np.all(np.abs(x.cpu().numpy()) <= 1.0)
        v = v.astype(np.int64).reshape(-1)
        sb = (bps + 7) // 8
        b = np.stack([(v >> (8 * k)) & 0xff for k in range(sb)], axis=1).astype(np.uint8)
        assert hashlib.md5(b.tobytes()).hexdigest() == md5, name


def test_gpu_load_batch(ctx):
    """Streams of different lengths: each slice is load() of that stream, the padding is zero, the lengths are right; a damaged frame
    raises ClaxonError."""
    import torch
    streams = [open(os.path.join(FIXTURES, n), "rb").read() for n in ("pop.flac", "short.flac", "wasted_bits.flac")]
    x, lengths, rates = cx.load_batch(ctx, streams)
    assert x.shape[0] == 3 and x.shape[1] % 8 == 0 and lengths.dtype == torch.int64
    for k, s in enumerate(streams):
        y, r = cx.load(ctx, s)
        assert int(lengths[k]) == y.shape[0] and rates[k] == r
        assert torch.equal(x[k, :y.shape[0]], y)
        assert not torch.any(x[k, y.shape[0]:] != 0)
    bad = bytearray(streams[0])
    bad[len(bad) // 2] ^= 0x10
    with pytest.raises(cx.ClaxonError):
        cx.load(ctx, bytes(bad))


def test_gpu_f32_refused_combinations(ctx):
    w = synth.config3(4)
    descs = _descs(w)
    for bad in (cx.OUT_F32 | cx.OUT_PCM16, cx.OUT_F32 | cx.OUT_PCM24, cx.OUT_F32 | cx.PATH_WAVES, cx.OUT_F32 | cx.PATH_LANES | cx.LANES_SPLIT,
                cx.OUT_F32 | cx.PATH_LANES | cx.LANES_FUSED | cx.LANES_GENERAL):
        with pytest.raises(cx.ClaxonError):
            ctx.plan(descs, w.out_offs, path=bad)
    ctx.plan(descs, w.out_offs, path=cx.OUT_F32 | cx.POOL).close()        # (CLX_POOL is ignored)
