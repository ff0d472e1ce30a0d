"""Sample windows from resident streams on the GPU: open_streams / StreamSet.read and clx_gather_windows.  The oracle is
cx.load(ctx, stream) of the same bytes, sliced on the device and compared with torch.equal."""
import os

import numpy as np
import pytest
import torch

import claxon_amd as cx
import md5_cases as mc
import synth

pytestmark = pytest.mark.gpu
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _workload(rng, n, ch, bs, bps, number0=0):
    """n frames (numbered from number0) of a tone with noise: (workload, interleaved samples)."""
    lim = 1 << (bps - 1)
    t = np.arange(n * bs)
    pcm = np.empty((ch, n * bs), dtype=np.int64)
    for c in range(ch):
        pcm[c] = np.clip(np.round(0.6 * lim * np.sin(2 * np.pi * (50 + 31 * c + rng.integers(0, 200)) * t / 44100.0) +
                                  rng.normal(0, max(1.0, lim / 512), n * bs)), -lim, lim - 1)
    frames = pcm.reshape(ch, n, bs).transpose(1, 0, 2).astype(np.int32)
    fp = [synth.FrameParams() for _ in range(n)]
    po = max(p for p in range(4) if bs % (1 << p) == 0 and (bs >> p) >= 32 or p == 0)      # (partitions divide the block and hold the warm-up)
    for i, f in enumerate(fp):
        f.number = number0 + i
        f.channel_assignment = (i % 4) if ch == 2 and bps <= 16 else 0
        for c in range(ch):
            f.sf[c] = synth.sf(synth.SF_LPC if (i + c) % 3 else synth.SF_FIXED, order=8 if (i + c) % 3 else 2, precision=12,
                               partition_order=po)
    return synth.encode_frames("windows", frames, ch, bs, bps, fp), pcm.T.reshape(-1)


def _stream(rng, n, ch, bs, bps, last=0):
    """A FLAC stream of n frames of bs samples, then one of `last` samples when that is not 0: (bytes, frame boundaries)."""
    w, vals = _workload(rng, n, ch, bs, bps)
    if last:
        w2, v2 = _workload(rng, 1, ch, last, bps, number0=n)
        w, vals = synth.concat("windows", [w, w2]), np.concatenate([vals, v2])
    return mc.stream(w, bs, ch, bps, vals), [bs * i for i in range(n + 1)] + ([bs * n + last] if last else [])


class Case:
    """A stream, its whole decode by load() (the oracle, computed once) and its single-stream set."""

    def __init__(self, ctx, data, bounds=None):
        self.data, self.bounds = data, bounds
        self.ref, self.rate = cx.load(ctx, data)
        self.T, self.C = self.ref.shape
        self.set = cx.open_streams(ctx, [data])
        assert self.set.problems == [None] and int(self.set.lengths[0]) == self.T and self.set.channels == [self.C]
        assert self.set.sample_rates == [self.rate]
        if bounds is None:          # (a fixture: its frame boundaries from the host indexer)
            st, _, _, off = cx.read_stream_header(np.frombuffer(data, dtype=np.uint8))
            d, _, _ = cx.index_frames(data, off)
            self.bounds = np.concatenate([[0], np.cumsum(d["block_size"].astype(np.int64))]).tolist()


def _slices(ref, starts, length):
    """The oracle's windows [B, length, C] and valid counts: slices of load()'s tensor, zero-filled."""
    T, C = ref.shape
    want = torch.zeros((len(starts), length, C), dtype=torch.float32, device=ref.device)
    valid = []
    for k, s in enumerate(starts):
        v = min(max(T - s, 0), length)
        want[k, :v] = ref[s:s + v]
        valid.append(v)
    return want, valid


def _check_reads(case, starts, length, sid=0, sset=None):
    """One read() per layout of windows at `starts` of one stream against the slices: exact, "ct" the transpose of "tc"."""
    sset = sset or case.set
    want, valid = _slices(case.ref, starts, length)
    tc, v1 = sset.read([sid] * len(starts), starts, length)
    ct, v2 = sset.read([sid] * len(starts), starts, length, layout="ct")
    assert tc.shape == (len(starts), length, case.C) and ct.shape == (len(starts), case.C, length)
    assert tc.is_contiguous() and ct.is_contiguous() and tc.dtype == ct.dtype == torch.float32 and tc.is_cuda and ct.is_cuda
    assert v1.dtype == torch.int64 and v1.tolist() == valid and v2.tolist() == valid
    assert torch.equal(tc, want), [k for k in range(len(starts)) if not torch.equal(tc[k], want[k])][:5]
    assert torch.equal(ct, want.transpose(1, 2))


@pytest.fixture(scope="module")
def fixtures(ctx):
    return {n: Case(ctx, open(os.path.join(FIXTURES, n), "rb").read()) for n in ("pop.flac", "short.flac", "wasted_bits.flac")}


@pytest.fixture(scope="module")
def synthetic(ctx):
    rng = np.random.default_rng(2024)
    shapes = dict(stereo16=(32, 2, 256, 16, 0), mono24=(6, 1, 192, 24, 0), three=(5, 3, 128, 16, 0), short_last=(4, 2, 255, 16, 77))
    return {name: Case(ctx, *_stream(rng, *shape)) for name, shape in shapes.items()}


@pytest.mark.parametrize("name", ("pop.flac", "short.flac", "wasted_bits.flac"))
def test_gpu_fixture_windows(fixtures, name):
    """Start 0, a start inside the first frame, the first three frame boundaries straddled by one sample either side, the stream's
    end met exactly, overrun and started at -- each fixture as its own single-stream set (they differ in channel count)."""
    c = fixtures[name]
    inner = [b for b in c.bounds[1:4] if b < c.T]
    for length in (64, 2):
        starts = [0, min(5, c.T - 1)]
        for b in inner:
            starts += [b - 1, b - length + 1, max(b - length // 2, 0), b]      # (one sample before / after the boundary inside the window)
        starts += [max(c.T - length, 0), max(c.T - length + 3, 0), c.T - 1, c.T, c.T + 5]
        _check_reads(c, [max(s, 0) for s in starts], length)


@pytest.mark.parametrize("name,length", [(n, l) for n in ("stereo16", "mono24", "three", "short_last") for l in (100, 257)] + [("stereo16", 1)])
def test_gpu_synthetic_windows_round_every_frame_boundary(synthetic, name, length):
    """Every frame boundary minus 1, plus 0 and plus 1 as a window start, all windows of a stream in one call."""
    c = synthetic[name]
    assert c.bounds[-1] == c.T
    starts = sorted({max(b + d, 0) for b in c.bounds for d in (-1, 0, 1)})
    _check_reads(c, starts, length)


def test_gpu_only_the_covering_frames_are_decoded(synthetic):
    c = synthetic["stereo16"]
    s = c.set
    n0 = s.frames_decoded
    out, valid = s.read([0], [1000], 100)                   # samples 1000..1099: the frames of 768..1023 and 1024..1279
    assert s.frames_decoded - n0 == 2 and torch.equal(out[0], c.ref[1000:1100])
    n0 = s.frames_decoded
    out, valid = s.read([0], [0], c.T)
    assert s.frames_decoded - n0 == 32 and torch.equal(out[0], c.ref) and valid.tolist() == [c.T]
    n0 = s.frames_decoded
    out, _ = s.read([0, 0], [1000, 1000], 100)              # (shared frames are decoded once per window)
    assert s.frames_decoded - n0 == 4 and torch.equal(out[0], out[1]) and torch.equal(out[1], c.ref[1000:1100])
    n0 = s.frames_decoded
    out, valid = s.read([0, 0], [c.T, c.T + 100], 50)       # (at and behind the end: zeros, nothing decoded)
    assert s.frames_decoded == n0 and valid.tolist() == [0, 0] and not bool(out.any())


def test_gpu_one_call_many_streams(ctx):
    """Eight stereo streams of different lengths in one set, 64 windows at seeded random (stream, start)."""
    rng = np.random.default_rng(8)
    datas = [_stream(rng, 3 + 2 * k, 2, 256 if k % 2 else 192, 16, last=(0, 51, 0, 130)[k % 4])[0] for k in range(8)]
    refs = [cx.load(ctx, d)[0] for d in datas]
    s = cx.open_streams(ctx, datas)
    assert s.problems == [None] * 8 and s.lengths.tolist() == [r.shape[0] for r in refs] and s.channels == [2] * 8
    assert s.bits_per_sample == [16] * 8 and s.sample_rates == [44100] * 8
    sid = rng.integers(0, 8, size=64)
    starts = np.array([int(rng.integers(0, refs[k].shape[0] + 40)) for k in sid])
    length = 300
    for layout in ("tc", "ct"):
        out, valid = s.read(sid, starts, length, layout=layout)
        assert valid.tolist() == [min(max(refs[k].shape[0] - st, 0), length) for k, st in zip(sid.tolist(), starts.tolist())]
        for k, (i, st) in enumerate(zip(sid.tolist(), starts.tolist())):
            want, _ = _slices(refs[i], [st], length)
            got = out[k] if layout == "tc" else out[k].t()
            assert torch.equal(got, want[0]), (layout, k, i, st)
    s.close()


def test_gpu_damage(ctx):
    """Two streams in one set, one byte flipped in the middle of a middle frame of stream 1."""
    rng = np.random.default_rng(9)
    good, _ = _stream(rng, 6, 2, 256, 16)
    w, vals = _workload(rng, 8, 2, 256, 16)
    other = bytearray(mc.stream(w, 256, 2, 16, vals))
    head = len(other) - int(w.lens.sum())                             # (the metadata in front of the first frame)
    other[head + int(w.lens[:4].sum()) + int(w.lens[4]) // 2] ^= 0x10  # frame 4: samples 1024..1279
    s = cx.open_streams(ctx, [good, bytes(other)])
    ref0 = cx.load(ctx, good)[0]
    out, _ = s.read([0, 0], [0, 700], 400)
    assert torch.equal(out[0], ref0[:400]) and torch.equal(out[1], ref0[700:1100])
    with pytest.raises(cx.ClaxonError) as e:
        s.read([0, 1], [0, 1000], 100)
    assert e.value.status != cx.OK and e.value.message
    if s.problems[1] is None:
        assert "(window 1, stream 1)" in str(e.value)
        ref1 = cx.load(ctx, mc.stream(w, 256, 2, 16, vals))[0]
        out, _ = s.read([1], [300], 700)                               # samples 300..999: wholly before the damaged frame
        assert torch.equal(out[0], ref1[300:1000])
    else:
        assert e.value is s.problems[1]


def test_gpu_refusals(ctx, synthetic):
    two, three = synthetic["stereo16"], synthetic["three"]
    s = cx.open_streams(ctx, [two.data, three.data, b"not a FLAC stream at all"])
    assert s.problems[0] is None and s.problems[1] is None and isinstance(s.problems[2], cx.ClaxonError)
    assert s.channels == [2, 3, 0] and s.lengths.tolist() == [two.T, three.T, 0]
    with pytest.raises(ValueError):
        s.read([0, 1], [0, 0], 16)                          # mixed channel counts
    with pytest.raises(ValueError):
        s.read([0], [-1], 16)
    with pytest.raises(ValueError):
        s.read([0], [0], -1)
    with pytest.raises(ValueError):
        s.read([0], [0], 16, layout="lc")
    with pytest.raises(ValueError):
        s.read([3], [0], 16)
    with pytest.raises(cx.ClaxonError) as e:
        s.read([2], [0], 16)
    assert e.value is s.problems[2]
    out, valid = s.read([1], [10], 16)                      # (the good streams of the set read as ever)
    assert torch.equal(out[0], three.ref[10:26]) and valid.tolist() == [16]
    for layout, shape in (("tc", (0, 16, 2)), ("ct", (0, 2, 16))):
        out, valid = cx.open_streams(ctx, [two.data]).read([], [], 16, layout=layout)
        assert out.shape == shape and valid.shape == (0,)
    out, valid = s.read([0, 0], [0, 5], 0)
    assert out.shape == (2, 0, 2) and valid.tolist() == [0, 0]


def test_gpu_raw_gather(ctx):
    """clx_gather_windows itself on a random float tensor: B = 70, L = 1000, C = 2, both layouts, against torch indexing; then once
    more on a non-default torch stream."""
    g = torch.Generator(device="cpu").manual_seed(3)
    B, L, C = 70, 1000, 2
    src = torch.randn(40000, generator=g).to("cuda:0")
    rng = np.random.default_rng(3)
    first = rng.integers(0, 40000 - L * C, size=B)
    valid = rng.integers(0, L + 1, size=B)
    valid[0], valid[1] = L, 0
    want = torch.zeros((B, L, C), device="cuda:0")
    for k in range(B):
        want[k, :valid[k]] = src[first[k]:first[k] + valid[k] * C].view(-1, C)
    torch.cuda.synchronize()
    for layout, ref in ((cx.WINDOW_TC, want), (cx.WINDOW_CT, want.transpose(1, 2).contiguous())):
        out = torch.full(ref.shape, float("nan"), device="cuda:0")
        ctx.gather_windows(src, first, valid, L, C, layout, out)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), layout
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        out = torch.full((B, C, L), float("nan"), device="cuda:0")
        ctx.gather_windows(src, first, valid, L, C, cx.WINDOW_CT, out)      # (queued on `side`, the current stream here)
        again = out.clone()
    side.synchronize()
    assert torch.equal(again, want.transpose(1, 2))
    with pytest.raises(cx.ClaxonError) as e:
        ctx.gather_windows(src, first, valid, L, 9, cx.WINDOW_TC, out)
    assert e.value.status == cx.API_ERROR and "channels" in e.value.message
