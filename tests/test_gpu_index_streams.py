"""clx_index_streams_device on the GPU against the host indexer run on each stream alone (the shard of index_cases.py: a host arena, a
device arena, a shuffled shard), and the loaders that go through it: load_batch against load, verify against verify of each stream
alone, and one index_streams call per load_batch / verify."""
import numpy as np
import pytest

import claxon_amd as cx
import index_cases as ic
import md5_cases as mc
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


@pytest.fixture(scope="module")
def cases():
    c = ic.streams()
    a = ic.host_answers(c)
    ic.check_shape(c, a)
    return c, a


def _device_arena(arena):
    import torch
    host = np.zeros((arena.size + 15) // 16 * 16 + 32, dtype=np.uint8)
    host[:arena.size] = arena
    return torch.from_numpy(host).cuda()


def test_gpu_host_arena(ctx, cases):
    c, a = cases
    arena, offs, lens, starts, order = ic.shard(c)
    got = ctx.index_streams(arena, offs, lens, starts)
    ic.assert_equal(got, ic.expected(c, a, offs, order), "host arena")
    assert got[0].size >= 300


def test_gpu_device_arena(ctx, cases):
    c, a = cases
    arena, offs, lens, starts, order = ic.shard(c)
    got = ctx.index_streams(_device_arena(arena), offs, lens, starts)
    ic.assert_equal(got, ic.expected(c, a, offs, order), "device arena")


def test_gpu_shuffled_shard(ctx, cases):
    c, a = cases
    order = np.random.default_rng(4).permutation(len(c)).tolist()
    arena, offs, lens, starts, order = ic.shard(c, order)
    want = ic.expected(c, a, offs, order)
    ic.assert_equal(ctx.index_streams(arena, offs, lens, starts), want, "shuffled, host arena")
    ic.assert_equal(ctx.index_streams(_device_arena(arena), offs, lens, starts), want, "shuffled, device arena")


def test_gpu_capacity_and_refusals(ctx, cases):
    c, a = cases
    arena, offs, lens, starts, order = ic.shard(c)
    want = ic.expected(c, a, offs, order)
    ic.assert_equal(ctx.index_streams(arena, offs, lens, starts, cap=3), want, "grown from cap = 3")
    with pytest.raises(cx.ClaxonError) as e:
        ctx.index_streams(arena, offs + np.uint64(8), lens, starts)
    assert e.value.status == cx.API_ERROR and "stream 0" in e.value.message
    d, _, first, stops = ctx.index_streams(arena, [], [])
    assert d.size == 0 and first.tolist() == [0]


def test_gpu_loaders_split_an_arena_beyond_one_call(ctx, cases):
    """The loaders' indexing step with the per-call limit set below the shard's size: several calls on slices of the device arena,
    joined, give the one-call answer."""
    c, a = cases
    arena, offs, lens, starts, order = ic.shard(c)
    want = ic.expected(c, a, offs, order)
    calls = []
    real = ctx.index_streams
    ctx.index_streams = lambda *x, **kw: (calls.append(1), real(*x, **kw))[1]
    try:
        d, first, stops = cx._index_arena(ctx, _device_arena(arena), offs.tolist(), lens.tolist(), starts.tolist(), limit=1300000)
    finally:
        del ctx.index_streams
    assert len(calls) >= 5
    assert d.tobytes() == want[0].tobytes() and first.tobytes() == want[2].tobytes() and stops.tobytes() == want[3].tobytes()


def _stream(seed, n, ch, bs, bps):
    rng = np.random.default_rng(seed)
    lim = 1 << (bps - 1)
    t = np.arange(n * bs)
    pcm = np.empty((ch, n * bs), dtype=np.int64)
    for c in range(ch):
        pcm[c] = np.clip(np.round(0.5 * lim * np.sin(2 * np.pi * (60 + 17 * c + seed % 97) * t / 44100.0) + rng.normal(0, lim / 300, n * bs)), -lim, lim - 1)
    fp = [synth.FrameParams() for _ in range(n)]
    for i, f in enumerate(fp):
        f.number = i
        f.channel_assignment = (i % 4) if ch == 2 else 0
        for c in range(ch):
            f.sf[c] = synth.sf(synth.SF_LPC if (i + c) % 3 else synth.SF_FIXED, order=8 if (i + c) % 3 else 2, precision=12, partition_order=3)
    w = synth.encode_frames("loader", pcm.reshape(ch, n, bs).transpose(1, 0, 2).astype(np.int32), ch, bs, bps, fp)
    return mc.stream(w, bs, ch, bps, pcm.T.reshape(-1))


@pytest.fixture(scope="module")
def corpus():
    """64 stereo 16-bit streams of 1..12 frames of 1024 samples."""
    return [_stream(900 + k, 1 + (k * 7) % 12, 2, 1024, 16) for k in range(64)]


class _Count:
    def __init__(self, monkeypatch):
        self.streams = self.frames = 0
        real_s, real_f = cx.Context.index_streams, cx.Context.index_frames

        def index_streams(ctx, *a, **kw):
            self.streams += 1
            return real_s(ctx, *a, **kw)

        def index_frames(ctx, *a, **kw):
            self.frames += 1
            return real_f(ctx, *a, **kw)
        monkeypatch.setattr(cx.Context, "index_streams", index_streams)
        monkeypatch.setattr(cx.Context, "index_frames", index_frames)


def test_gpu_load_batch_of_64_streams(ctx, corpus, monkeypatch):
    import torch
    singles = [cx.load(ctx, s) for s in corpus]
    n = _Count(monkeypatch)
    x, lengths, rates = cx.load_batch(ctx, corpus)
    assert (n.streams, n.frames) == (1, 0)
    assert x.shape[0] == 64 and x.shape[1] % 8 == 0 and len({int(v) for v in lengths}) > 4
    for k, (y, r) in enumerate(singles):
        assert int(lengths[k]) == y.shape[0] == 1024 * (1 + (k * 7) % 12) and rates[k] == r
        assert torch.equal(x[k, :y.shape[0]], y), k
        assert not torch.any(x[k, y.shape[0]:] != 0), k
    cx.load_batch(ctx, corpus, verify_md5=True)
    bad = bytearray(corpus[37])
    bad[8 + 18 + 5] ^= 0x40                                        # a byte of STREAMINFO's MD5
    with pytest.raises(cx.ClaxonError) as e:
        cx.load_batch(ctx, corpus[:37] + [bytes(bad)] + corpus[38:], verify_md5=True)
    assert e.value.status == cx.FORMAT_ERROR and "MD5 signature mismatch" in e.value.message and "(stream 37)" in e.value.message


def test_gpu_verify_whole_shard_equals_each_stream_alone(ctx, cases, monkeypatch):
    c, _ = cases
    datas = [d.tobytes() for _, d, _ in c]
    alone = [cx.verify(ctx, [d])[0] for d in datas]
    n = _Count(monkeypatch)
    together = cx.verify(ctx, datas)
    assert (n.streams, n.frames) == (1, 0)
    assert len(together) == len(alone)
    for (name, _, _), t, s in zip(c, together, alone):
        assert (t.ok, t.md5_checked, t.status, t.message, t.samples) == (s.ok, s.md5_checked, s.status, s.message, s.samples), (name, t, s)
    assert sum(v.ok for v in together) >= 9 and sum(not v.ok for v in together) >= 9
