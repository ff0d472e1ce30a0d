"""Stream MD5 on the GPU: clx_md5_streams over every output mode's buffer, load / load_batch(verify_md5=True) and verify() on the
fixtures and on a few hundred synthetic streams, and the damage that every frame's CRC-16 passes -- frames swapped, a stream cut at
a frame boundary -- which only STREAMINFO's sample count and MD5 catch."""
import hashlib
import os

import numpy as np
import pytest

import claxon_amd as cx
import md5_cases as mc
import synth

pytestmark = pytest.mark.gpu
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _frames(rng, n, ch, bs, bps):
    """A workload of n frames (numbered 0..n-1) of a tone with noise; returns (workload, interleaved samples)."""
    lim = 1 << (bps - 1)
    t = np.arange(n * bs)
    pcm = np.empty((ch, n * bs), dtype=np.int64)
    for c in range(ch):
        pcm[c] = np.clip(np.round(0.6 * lim * np.sin(2 * np.pi * (50 + 31 * c + rng.integers(0, 200)) * t / 44100.0) +
                                  rng.normal(0, max(1.0, lim / 512), n * bs)), -lim, lim - 1)
    frames = pcm.reshape(ch, n, bs).transpose(1, 0, 2).astype(np.int32)
    fp = [synth.FrameParams() for _ in range(n)]
    for i, f in enumerate(fp):
        f.number = i
        f.channel_assignment = (i % 4) if ch == 2 and bps <= 16 else 0
        for c in range(ch):
            f.sf[c] = synth.sf(synth.SF_LPC if (i + c) % 3 else synth.SF_FIXED, order=8 if (i + c) % 3 else 2, precision=12,
                               partition_order=min(3, max(0, int(np.log2(bs)) - 5)))
    return synth.encode_frames("md5", frames, ch, bs, bps, fp), pcm.T.reshape(-1)


@pytest.fixture(scope="module")
def corpus():
    """A few hundred streams: 8..24 bits, mono / stereo / 6 channels, 1..5 frames of 256..4096 samples."""
    rng = np.random.default_rng(77)
    out = []
    for k in range(240):
        bps = (8, 12, 16, 20, 24)[k % 5]
        ch = (1, 2, 6)[(k // 5) % 3]
        bs = (256, 1024, 576, 4096)[(k // 15) % 4]
        n = 1 + int(rng.integers(0, 5))
        w, vals = _frames(rng, n, ch, bs, bps)
        out.append(dict(w=w, vals=vals, bps=bps, ch=ch, bs=bs, data=mc.stream(w, bs, ch, bps, vals)))
    return out


def test_gpu_fixtures_verify(ctx):
    names = ("pop.flac", "short.flac", "wasted_bits.flac")
    datas = [open(os.path.join(FIXTURES, n), "rb").read() for n in names]
    for name, data in zip(names, datas):
        x, _ = cx.load(ctx, data, verify_md5=True)
        st, _, si, _ = cx.read_stream_header(np.frombuffer(data, dtype=np.uint8))
        got = ctx.md5_streams(x, cx.SAMPLE_F32, [0], [x.numel()], [int(si.bits_per_sample)])
        assert bytes(got[0]) == bytes(si.md5sum), name
    cx.load_batch(ctx, datas, verify_md5=True)
    ns = open(os.path.join(FIXTURES, "non_subset.flac"), "rb").read()
    cx.load(ctx, ns, verify_md5=True)
    v = cx.verify(ctx, datas + [ns])
    assert [x.ok for x in v] == [True] * 4, v
    assert [x.md5_checked for x in v] == [True, True, True, False], v


def test_gpu_verify_synthetic_corpus(ctx, corpus):
    v = cx.verify(ctx, [c["data"] for c in corpus])
    bad = [(k, x) for k, x in enumerate(v) if not (x.ok and x.md5_checked)]
    assert not bad, bad[:4]
    assert [x.samples for x in v] == [c["vals"].size // c["ch"] for c in corpus]


def test_gpu_every_output_mode_hashes_the_same(ctx, corpus):
    """One arena of all streams' frames; each output mode decodes the streams it takes, then one md5_streams call over its buffer:
    PCM16 (<= 16 bits), PCM24 (<= 24), F32, and planar i32 followed by clx_batch_interleave at 4 and at ceil(bps / 8) bytes."""
    import torch
    w = synth.concat("md5 corpus", [c["w"] for c in corpus])
    descs = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)[0]
    frame_stream = np.concatenate([np.full(c["w"].n, k) for k, c in enumerate(corpus)])
    want = [mc.ref_md5(c["vals"], c["bps"]) for c in corpus]
    arena = torch.from_numpy(w.arena).cuda()
    modes = [("pcm16", cx.OUT_PCM16, 16, 2), ("pcm24", cx.OUT_PCM24, 24, 3), ("f32", cx.OUT_F32, 24, cx.SAMPLE_F32),
             ("planar+sb4", 0, 24, 4), ("planar+sb", 0, 24, None)]
    for name, flag, top, fmt in modes:
        ks = [k for k, c in enumerate(corpus) if c["bps"] <= top]
        base, at = {}, 0
        for k in ks:
            base[k] = at
            at += ((corpus[k]["vals"].size + 7) // 8) * 8
        sel = np.nonzero(np.isin(frame_stream, ks))[0]
        offs, local = np.zeros(sel.size, dtype=np.uint64), {}
        for j, i in enumerate(sel):
            k = int(frame_stream[i])
            offs[j] = base[k] + local.get(k, 0)
            local[k] = local.get(k, 0) + int(descs["n_channels"][i]) * int(descs["block_size"][i])
        d = descs[sel]
        b = ctx.plan(d, offs, verify_crc=True, path=flag)
        try:
            out = torch.zeros(at + 64, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            b.run(arena.data_ptr(), w.arena_len, out.data_ptr())
            assert np.all(b.results()["status"] == cx.OK), name
            bps = [corpus[k]["bps"] for k in ks]
            groups = [(fmt, ks, bps)] if fmt is not None else [(s, [k for k, x in zip(ks, bps) if mc.width(x) == s], [x for x in bps if mc.width(x) == s]) for s in (1, 2, 3)]
            for f, kk, bb in groups:
                src = out
                if flag == 0:
                    src = torch.zeros((at + 64) * mc.sample_size(f), dtype=torch.uint8, device="cuda")
                    b.interleave(out.data_ptr(), src.data_ptr(), f)
                    torch.cuda.synchronize()
                got = ctx.md5_streams(src, f, [base[k] for k in kk], [corpus[k]["vals"].size for k in kk], bb)
                for k, g in zip(kk, got):
                    assert bytes(g) == want[k], (name, f, k, corpus[k]["bps"], corpus[k]["ch"])
        finally:
            b.close()


def _damaged(rng):
    """(good stream, frames 2 and 3 swapped, cut after frame 3 of 6): every frame of each passes its CRC-16."""
    bs, ch, bps = 1024, 2, 16
    w, vals = _frames(rng, 6, ch, bs, bps)
    good = mc.stream(w, bs, ch, bps, vals)
    swapped = mc.stream(w, bs, ch, bps, vals, frames=[0, 1, 3, 2, 4, 5])
    cut = mc.stream(w, bs, ch, bps, vals, frames=[0, 1, 2, 3])
    return good, swapped, cut


def test_gpu_damage_the_crcs_cannot_see(ctx):
    rng = np.random.default_rng(5)
    good, swapped, cut = _damaged(rng)
    x, _ = cx.load(ctx, good, verify_md5=True)
    # without verification both load with no error: the gap this check closes
    y, _ = cx.load(ctx, swapped)
    assert y.shape == x.shape and not bool((y == x).all())
    z, _ = cx.load(ctx, cut)
    assert z.shape[0] == 4 * 1024
    with pytest.raises(cx.ClaxonError) as e:
        cx.load(ctx, swapped, verify_md5=True)
    assert e.value.status == cx.FORMAT_ERROR and "MD5 signature mismatch" in e.value.message
    with pytest.raises(cx.ClaxonError) as e:
        cx.load(ctx, cut, verify_md5=True)
    assert e.value.status == cx.FORMAT_ERROR and "length mismatch" in e.value.message
    with pytest.raises(cx.ClaxonError) as e:
        cx.load_batch(ctx, [good, swapped], verify_md5=True)
    assert "MD5 signature mismatch" in e.value.message and "(stream 1)" in e.value.message
    cx.load_batch(ctx, [good, swapped])                                  # (the default checks no more than before)


def test_gpu_verify_reports_each_stream(ctx):
    rng = np.random.default_rng(6)
    good, swapped, cut = _damaged(rng)
    good2, _, _ = _damaged(rng)
    junk = b"fLaC" + b"\x00" * 10
    v = cx.verify(ctx, [good, swapped, good2, cut, good, junk, b""])
    assert [x.ok for x in v] == [True, False, True, False, True, False, False], v
    assert v[1].md5_checked and v[1].message == "MD5 signature mismatch" and v[1].status == cx.FORMAT_ERROR
    assert "length mismatch" in v[3].message and v[3].samples == 4 * 1024
    assert v[5].status != cx.OK and v[6].status != cx.OK
    assert cx.verify(ctx, []) == []


def test_gpu_md5_streams_refusals_and_empty(ctx):
    import torch
    x = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for fmt, bps in ((0, 8), (2, 17), (cx.SAMPLE_F32, 25), (4, 33), (1, 0)):
        with pytest.raises(cx.ClaxonError):
            ctx.md5_streams(x, fmt, [0], [4], [bps])
    assert ctx.md5_streams(x, 2, [], [], []).shape == (0, 16)
    got = ctx.md5_streams(x, 2, [0, 3], [0, 5], [16, 16])
    assert bytes(got[0]) == hashlib.md5(b"").digest() and bytes(got[1]) == hashlib.md5(bytes(10)).digest()
