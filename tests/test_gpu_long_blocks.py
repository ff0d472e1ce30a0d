"""FLAC's outer limits on the GPU: blocks of 4 609 .. 65 535 samples and escape-coded partitions (parity_cases.long_block_workload /
escape_workload) through every kernel selection, the narrow and float outputs, pipelined merged submissions, decode_frames_stream, the
FlacReader path, whole streams of 65 535-sample frames (indexers, load / load_batch / verify with the MD5), and batches at scale whose
staging memory is measured."""
import numpy as np
import pytest

import claxon_amd as cx
import md5_cases as mc
import parity_cases as pc
import synth
from parity_util import GpuBackend

pytestmark = pytest.mark.gpu
LANES = cx.PATH_LANES | cx.LANES_FUSED


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


@pytest.fixture(scope="module")
def long2():
    return pc.long_block_workload(scale=2)


@pytest.fixture(scope="module")
def escapes():
    return pc.escape_workload()


@pytest.mark.parametrize("path", [cx.PATH_WAVES | cx.K2_LATENCY, cx.PATH_WAVES | cx.K2_THROUGHPUT, cx.PATH_LANES | cx.LANES_SPLIT,
                                  LANES, LANES | cx.LANES_GENERAL, LANES | cx.COMPOSE],
                         ids=["waves", "waves-1w", "lanes", "lanes-fused", "lanes-general", "lanes-composed"])
def test_gpu_long_blocks_and_escapes(oracle, ctx, long2, escapes, path):
    st, _ = pc.check_against_oracle(oracle, GpuBackend(ctx, path), long2)
    assert np.all(st == cx.OK)
    pc.check_escape_kinds(escapes, *pc.check_against_oracle(oracle, GpuBackend(ctx, path), escapes))


@pytest.mark.parametrize("out", ["pcm16", "pcm24", "f32"])
def test_gpu_long_blocks_and_escapes_narrow_outputs(oracle, ctx, long2, escapes, out):
    flag = {"pcm16": cx.OUT_PCM16, "pcm24": cx.OUT_PCM24, "f32": cx.OUT_F32}[out]
    st, _ = pc.check_against_oracle(oracle, GpuBackend(ctx, LANES | flag), pc.for_output(long2, out), out=out)
    assert np.all(st == cx.OK)
    e = pc.for_output(escapes, out)
    pc.check_escape_kinds(e, *pc.check_against_oracle(oracle, GpuBackend(ctx, LANES | flag), e, out=out))


def _bytes_of(mode):
    return {0: 4, cx.OUT_PCM16: 2, cx.OUT_PCM24: 3, cx.OUT_F32: 4}[mode]


@pytest.mark.parametrize("mode", [0, cx.OUT_PCM16, cx.OUT_PCM24, cx.OUT_F32], ids=["planar", "pcm16", "pcm24", "f32"])
def test_gpu_long_blocks_pipelined_submissions(oracle, ctx, long2, escapes, mode):
    """submit_depth + 2 submissions (merged launches) over distinct arenas -- intact, long frames damaged -- into distinct outputs."""
    import torch
    name = {0: "planar", cx.OUT_PCM16: "pcm16", cx.OUT_PCM24: "pcm24", cx.OUT_F32: "f32"}[mode]
    long2 = pc.for_output(long2, name)
    w = synth.concat("long + escapes", [long2, pc.for_output(escapes, name)])
    descs = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)[0]
    batch = ctx.plan(descs, w.out_offs, verify_crc=True, path=mode)
    depth = batch.submit_depth
    rng = np.random.default_rng(17)
    arenas = []
    for k in range(depth + 2):
        a = w.arena.copy()
        if k % 2:
            for i in range(k, long2.n, 5):
                pos = int(rng.integers(8 * (int(w.offs[i]) + 16), 8 * int(w.offs[i] + w.lens[i])))
                a[pos >> 3] ^= 0x80 >> (pos & 7)
        arenas.append(a)
    d_arenas = [torch.from_numpy(a).cuda() for a in arenas]
    nb = _bytes_of(mode)
    outs = [torch.full((w.pcm.size * nb + 16,), 0x11, dtype=torch.uint8, device="cuda") for _ in arenas]
    torch.cuda.synchronize()
    for k in range(len(arenas)):
        batch.submit(d_arenas[k].data_ptr(), w.arena_len, outs[k].data_ptr())
    batch.flush()
    torch.cuda.synchronize()
    mode_name = {0: "planar", cx.OUT_PCM16: "pcm16", cx.OUT_PCM24: "pcm24", cx.OUT_F32: "f32"}[mode]
    for k in range(len(arenas)):
        got = outs[k].cpu().numpy()
        if mode == 0 or mode == cx.OUT_F32:
            got = got[:w.pcm.size * 4].view(np.int32)
        ref = np.zeros(w.pcm.size, dtype=np.int32)
        r = oracle.decode_batch(arenas[k][:w.arena_len], w.offs, w.lens, out=ref, out_offs=w.out_offs, check_crc=True)
        if k % 2 == 0:
            assert np.all(r["statuses"][:long2.n] == cx.OK)
        else:
            assert np.sum(r["statuses"][:long2.n] != cx.OK) >= 4
        for i in np.nonzero(r["statuses"] == cx.OK)[0]:
            a, c, bs = int(w.out_offs[i]), int(w.channels[i]), int(w.block_sizes[i])
            inter = ref[a:a + c * bs].reshape(c, bs).T.reshape(-1)
            if mode == 0:
                ok = np.array_equal(got[a:a + c * bs], ref[a:a + c * bs])
            elif mode == cx.OUT_PCM16:
                ok = np.array_equal(got[:w.pcm.size * 2].view(np.int16)[a:a + c * bs], inter.astype(np.int16))
            elif mode == cx.OUT_PCM24:
                u = inter.view(np.uint32)
                ok = np.array_equal(got[3 * a:3 * (a + c * bs)], np.stack([u & 0xff, (u >> 8) & 0xff, (u >> 16) & 0xff], axis=1).astype(np.uint8).reshape(-1))
            else:
                want = inter.astype(np.float32) * np.float32(2.0 ** (1 - int(w.bps[i])))
                ok = np.array_equal(got[a:a + c * bs].view(np.uint32), want.view(np.uint32))
            assert ok, (mode_name, k, int(i), bs, c)
    # (the batch exposes the verdicts of its last submission only: the earlier ones are checked above through the bytes of every frame
    #  the oracle decodes -- a frame the kernels failed would have left the fill there)
    res = batch.results()
    r = oracle.decode_batch(arenas[-1][:w.arena_len], w.offs, w.lens, out=np.zeros(w.pcm.size, dtype=np.int32), out_offs=w.out_offs, check_crc=True)
    assert np.array_equal(np.asarray(res["status"]), r["statuses"]) and np.array_equal(np.asarray(res["msg"]), r["msgs"])
    batch.close()


def test_gpu_long_blocks_decode_frames_stream(oracle, ctx, long2, escapes):
    """decode_frames_stream in chunks of a few frames (frames of up to 65 535 samples straddle nothing: every chunk is whole frames)."""
    w = synth.concat("long + escapes", [long2, escapes])
    descs = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)[0]
    ref = np.zeros(w.pcm.size, dtype=np.int32)
    r = oracle.decode_batch(w.arena[:w.arena_len], w.offs, w.lens, out=ref, out_offs=w.out_offs, check_crc=True)
    bad = r["statuses"] != 0
    for i in np.nonzero(bad)[0]:                                  # (samples of failed frames read as zeros)
        a = int(w.out_offs[i]); ref[a:a + int(w.channels[i]) * int(w.block_sizes[i])] = 0
    for chunk in (0, 7):
        ctx.set_stream_chunk(chunk)
        out, res = ctx.decode_frames_stream(w.arena[:w.arena_len], descs, w.out_offs, verify_crc=True)
        assert np.array_equal(res["status"], r["statuses"]) and np.array_equal(res["msg"], r["msgs"])
        assert np.array_equal(res["end_bit"][~bad], r["end_bits"][~bad])
        assert np.array_equal(out, ref)
    ctx.set_stream_chunk(0)


def _long_stream(rng, n, ch, bs, bps):
    """n frames of bs samples (numbered 0..n-1): (workload, interleaved samples)."""
    pcm = np.empty((n, ch, bs), dtype=np.int32)
    fps = []
    for i in range(n):
        for c in range(0, ch, 2):
            L, R, _ = pc._music(rng, 7 * i + c, bs, bps)
            pcm[i, c] = L
            if c + 1 < ch:
                pcm[i, c + 1] = R
        fp = synth.FrameParams(3 if ch == 2 else 0, 0, i)
        for c in range(ch):
            fp.sf[c] = synth.sf(synth.SF_LPC, 12, 14, 0 if bs % 2 else 4)
        fps.append(fp)
    w = synth.encode_frames("stream bs%d" % bs, pcm, ch, bs, bps, fps)
    return w, pcm.transpose(0, 2, 1).reshape(-1)


@pytest.fixture(scope="module")
def long_streams():
    rng = np.random.default_rng(6553)
    out = []
    for n, ch, bs, bps in ((5, 2, 65535, 16), (4, 2, 40001, 24), (3, 6, 65520, 20), (6, 1, 65535, 8)):
        w, vals = _long_stream(rng, n, ch, bs, bps)
        out.append(dict(w=w, vals=vals, ch=ch, bs=bs, bps=bps, data=mc.stream(w, bs, ch, bps, vals),
                        swapped=mc.stream(w, bs, ch, bps, vals, frames=[1, 0] + list(range(2, n))),
                        cut=mc.stream(w, bs, ch, bps, vals, frames=list(range(n - 1)))))
    return out


def test_gpu_long_streams_indexers_and_reader(oracle, ctx, long_streams):
    """STREAMINFO max block size 65 535: the host indexer and clx_k_find_headers give the oracle's frame offsets (header chains across
    frames of hundreds of KB), and the FlacReader path decodes every frame as the reference does."""
    for s in long_streams:
        data = s["data"]
        si, blocks, st, msg = oracle.decode_stream(data)
        assert len(blocks) == s["w"].n
        head = len(data) - s["w"].arena_len
        starts, pos = [], head
        for info, _ in blocks:
            starts.append(pos)
            pos += int(info.bytes_consumed)
        u8 = np.frombuffer(data, dtype=np.uint8)
        for name, (descs, hdrs, stop) in (("host", cx.index_frames(u8, start=head)), ("device", ctx.index_frames(u8, start=head))):
            assert descs["byte_off"].tolist() == starts, name
            assert stop == len(data), name
            assert hdrs["block_size"].tolist() == [s["bs"]] * len(starts), name
        end, got, _ = pc.stream_decode_both(oracle, GpuBackend(ctx, LANES), data, True)
        assert end == ("end", cx.END_OF_STREAM, 0) and len(got) == s["w"].n


def test_gpu_long_streams_md5(ctx, long_streams):
    """load / load_batch(verify_md5=True) and verify() pass the intact streams of 65 535-sample frames and fail a cut or swapped one."""
    for s in long_streams:
        x, _ = cx.load(ctx, s["data"], verify_md5=True)
        assert x.shape == (s["vals"].size // s["ch"], s["ch"])
        want = s["vals"].astype(np.float32) * np.float32(2.0 ** (1 - s["bps"]))
        assert np.array_equal(x.cpu().numpy().reshape(-1).view(np.uint32), want.view(np.uint32))
        for bad, why in ((s["swapped"], "MD5 signature mismatch"), (s["cut"], "length mismatch")):
            with pytest.raises(cx.ClaxonError) as e:
                cx.load(ctx, bad, verify_md5=True)
            assert why in e.value.message
    stereo = [s for s in long_streams if s["ch"] == 2]
    cx.load_batch(ctx, [s["data"] for s in stereo], verify_md5=True)
    with pytest.raises(cx.ClaxonError) as e:
        cx.load_batch(ctx, [stereo[0]["data"], stereo[1]["swapped"]], verify_md5=True)
    assert "(stream 1)" in e.value.message
    verdicts = cx.verify(ctx, [s[k] for s in long_streams for k in ("data", "swapped", "cut")])
    assert [v.ok for v in verdicts] == [True, False, False] * len(long_streams)


def _staging_bound():
    """What the plan and the merged submissions of a batch of 65 535-sample rows may hold: per internal stream (CLX_SUBMIT_STREAMS = 2)
    the general kernels' staging of one launch -- at most max(512 MiB, one group of 64 rows of 65 536 samples per CU) -- with a quarter
    on top for the batch's scratch and for what mem_get_info sees of the rest of the device."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return int(1.25 * 2 * max(512 << 20, cus * 64 * 65536 * 4))


def _mem_used():
    import torch
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(0)
    return -int(free)


def _scale_run(w_unique, total, mode):
    """`total` frames tiled from `w_unique` (re-stamped numbers), planned once and submitted submit_depth + 1 times (merged launches) into
    as many outputs; every output is compared on the device with the tiled source PCM.  Returns (device bytes that the plan and the
    submissions held, bytes of one output buffer)."""
    import torch
    ts = synth.TiledStream(w_unique, total)
    w = ts.slice(0, total)
    ctx = cx.Context(0, wait_s=300)
    descs = cx.descs_from_offsets(w.arena, w.offs, w.lens, check_crc=False)[0]
    n_samples = int(w.out_offs[-1]) + int(w.channels[-1]) * int(w.block_sizes[-1])
    nb = _bytes_of(mode)
    d_arena = torch.from_numpy(w.arena).cuda()
    used0 = _mem_used()
    batch = ctx.plan(descs, w.out_offs, verify_crc=True, path=mode)
    n_sub = batch.submit_depth + 1
    outs = [torch.full((n_samples * nb // 2 + 8,), 0x1111, dtype=torch.int16, device="cuda") for _ in range(n_sub)]
    for k in range(n_sub):
        batch.submit(d_arena.data_ptr(), int(w.arena_len), outs[k].data_ptr())
    batch.flush()
    used1 = _mem_used()
    res = batch.results()
    assert np.all(res["status"] == cx.OK)
    # the expected output: unique frame u's interleaved samples wherever frame i % U lands
    u = w_unique
    per = int(u.channels[0]) * int(u.block_sizes[0])
    assert np.all(u.channels == u.channels[0]) and np.all(u.block_sizes == u.block_sizes[0])
    uni = u.pcm.reshape(u.n, int(u.channels[0]), int(u.block_sizes[0])).transpose(0, 2, 1).reshape(u.n, per)
    if mode == cx.OUT_PCM16:
        d_uni = torch.from_numpy(uni.astype(np.int16)).cuda()
    else:
        d_uni = torch.from_numpy(uni.astype(np.float32) * np.float32(2.0 ** (1 - int(u.bps[0])))).cuda()
    idx = torch.from_numpy(np.arange(total) % u.n).cuda()
    for k, o in enumerate(outs):
        got = o[:n_samples * nb // 2]
        got = got.view(torch.float32) if mode == cx.OUT_F32 else got
        assert bool(torch.equal(got.view(total, per), d_uni[idx])), k
    batch.close(); ctx.close()
    held = used1 - used0 - sum(o.numel() * 2 for o in outs)
    return held, n_samples * nb


@pytest.mark.parametrize("mode", [cx.OUT_PCM16, cx.OUT_F32], ids=["pcm16", "f32"])
def test_gpu_scale_65535_sample_frames(mode):
    """2 048 stereo frames of 65 535 samples (64 unique, tiled) through merged submissions: every output exact.  Device memory that the
    plan and the submissions hold (staging rows of the general kernels -- every group of 65 535-sample frames is theirs -- scratch,
    descriptors), measured with torch.cuda.mem_get_info around them, stays within _staging_bound(): 10.7 GB on a 256-CU MI355X, where
    8.9 GB were measured -- and 25.8 GB before the general kernels' staging was bounded per launch (profiles/long_block_memory.txt)."""
    rng = np.random.default_rng(2048)
    bs, U = 65535, 64
    pcm = np.empty((U, 2, bs), dtype=np.int32)
    fps = []
    for i in range(U):
        L, R, _ = pc._music(rng, i, bs, 16)
        pcm[i, 0], pcm[i, 1] = L, R
        fp = synth.FrameParams(i % 4, 0, synth.TILE_NUMBER_BASE + i)
        for c in range(2):
            fp.sf[c] = synth.sf(synth.SF_FIXED, 2, 0, 0, rice_param=-1)
        fps.append(fp)
    u = synth.encode_frames("65535 x 64", pcm, 2, bs, 16, fps)
    held, out_bytes = _scale_run(u, 2048, mode)
    print("held %.3f GB, one output %.3f GB, ratio %.2f" % (held / 1e9, out_bytes / 1e9, held / out_bytes))
    assert held <= _staging_bound(), (held, out_bytes)


def test_gpu_scale_one_long_frame_among_short_ones(oracle):
    """2 000 stereo 4 096-sample frames with ONE 65 535-sample frame among them, CLX_OUT_PCM16 through merged submissions: exact output,
    and the plan and the submissions hold no more than _staging_bound() (the staging rows are as long as the batch's longest block;
    8.1 GB measured on an MI355X: profiles/long_block_memory.txt)."""
    import torch
    a, b = synth.config3(1000), synth.config3(1000)
    rng = np.random.default_rng(1)
    L, R, _ = pc._music(rng, 0, 65535, 16)
    fp = synth.FrameParams(3, 0, 1000)
    for c in range(2):
        fp.sf[c] = synth.sf(synth.SF_LPC, 8, 12, 0)
    lone = synth.encode_frames("65535", np.stack([L, R])[None], 2, 65535, 16, [fp])
    w = synth.concat("one long frame", [a, lone, b])
    descs = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)[0]
    ctx = cx.Context(0, wait_s=120)
    d_arena = torch.from_numpy(w.arena).cuda()
    used0 = _mem_used()
    batch = ctx.plan(descs, w.out_offs, verify_crc=True, path=cx.OUT_PCM16)
    n_sub = batch.submit_depth + 1
    outs = [torch.full((w.pcm.size + 8,), 0x1111, dtype=torch.int16, device="cuda") for _ in range(n_sub)]
    for k in range(n_sub):
        batch.submit(d_arena.data_ptr(), w.arena_len, outs[k].data_ptr())
    batch.flush()
    used1 = _mem_used()
    assert np.all(batch.results()["status"] == cx.OK)
    want = np.zeros(w.pcm.size, dtype=np.int16)
    for i in range(w.n):
        o, c, bs = int(w.out_offs[i]), int(w.channels[i]), int(w.block_sizes[i])
        want[o:o + c * bs] = w.pcm[o:o + c * bs].reshape(c, bs).T.reshape(-1).astype(np.int16)
    d_want = torch.from_numpy(want).cuda()
    for k, o in enumerate(outs):
        assert bool(torch.equal(o[:w.pcm.size], d_want)), k
    held = used1 - used0 - sum(o.numel() * 2 for o in outs)
    print("held %.3f GB, one output %.3f GB, ratio %.2f" % (held / 1e9, w.pcm.size * 2 / 1e9, held / (w.pcm.size * 2)))
    batch.close(); ctx.close()
    assert held <= _staging_bound(), (held, w.pcm.size * 2)
