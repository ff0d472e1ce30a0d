"""Where decoded frames land: layouts, workloads and ONE whole-buffer check, shared by the wave simulator's tests
(test_sim_placement.py) and the GPU's (test_gpu_placement.py).

The parity tests lay every output out in frame order, back to back, from offset 0 of a fresh allocation, and look at the blocks of OK
frames only.  Here the blocks are reversed, shuffled, spread by gaps, shifted off every documented alignment boundary or based on an
odd pointer, the buffer is pre-filled with a position-dependent sentinel, and EVERY element of it is compared with what the oracle
alone says it must hold afterwards: a frame's block in the output mode's format inside an OK frame's block, the sentinel everywhere
else (guards in front of the first block and behind the last, gaps) -- only the blocks of failed frames, whose content the contract
leaves open, are masked out."""
import zlib

import numpy as np

import claxon_amd as cx
import parity_cases as pc
import synth

MODES = ("planar", "pcm16", "pcm24", "f32")
ELEM_BYTES = {"planar": 4, "pcm16": 2, "pcm24": 1, "f32": 4}        # an element of `d_out`: int32, int16, a byte, a float
ELEMS_PER_SAMPLE = {"planar": 1, "pcm16": 1, "pcm24": 3, "f32": 1}
OUT_FLAG = {"planar": 0, "pcm16": cx.OUT_PCM16, "pcm24": cx.OUT_PCM24, "f32": cx.OUT_F32}
GUARD = 256                    # elements in front of the first block and behind the last (a multiple of 256 bytes in every mode)
SHIFTS = (1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 17)      # one below, on and one above 4 (a planar row), 8 (pcm16, f32) and 16 (pcm24) samples
ODD_BASES = (1, 2, 3)


# ------------------------------------------------------------------------------------------------ layouts

def _sizes(w):
    return w.channels.astype(np.uint64) * w.block_sizes.astype(np.uint64)


def _place(w, order, gaps):
    """Blocks in the order `order`, gaps[j] samples in front of the j-th placed block."""
    sizes = _sizes(w)
    offs = np.zeros(w.n, dtype=np.uint64)
    pos = 0
    for j, i in enumerate(order):
        pos += int(gaps[j])
        offs[int(i)] = pos
        pos += int(sizes[int(i)])
    return offs, pos


def reversed_order(w):
    """Frame n-1 first, back to back."""
    return _place(w, np.arange(w.n)[::-1], np.zeros(w.n, dtype=np.int64))


def shuffled_gaps(w, seed, increasing=False, min_frames=32):
    """A random permutation of the frames (`increasing`: frame order) with a gap of 0..67 samples in front of each block; the gaps of
    the first blocks are chosen so that every residue of an offset mod 32 occurs.  That takes 32 frames: `min_frames` (default 32)
    is asserted, and a caller that hands over fewer on purpose says so."""
    rng = np.random.default_rng(seed)
    order = np.arange(w.n) if increasing else rng.permutation(w.n)
    gaps = rng.integers(0, 68, w.n)
    sizes = _sizes(w)
    want = rng.permutation(32)
    pos = 0
    for j, i in enumerate(order):
        if j < 32:       # (two or three gaps in 0..67 give the wanted residue: take one of them)
            g = (int(want[j]) - pos) % 32
            gaps[j] = g + 32 * int(rng.integers(0, 2 if g + 32 <= 67 else 1))
        pos += int(gaps[j]) + int(sizes[int(i)])
    offs, length = _place(w, order, gaps)
    assert 0 <= gaps.min() and gaps.max() <= 67
    assert w.n >= min_frames, "%s has %d frames: too few for every residue mod 32" % (w.name, w.n)
    assert w.n < 32 or set((offs % np.uint64(32)).tolist()) == set(range(32)), "every residue mod 32 must occur"
    return offs, length


def shuffled_aligned(w, seed):
    """A random permutation with every gap a multiple of 32 samples (0 included): a block that started on 32 samples still does, so
    what qualified for the tiers still qualifies in every output mode -- but a wave's lowest row is no longer lane 0's, and the lanes'
    distances from it are not monotonic."""
    rng = np.random.default_rng(seed)
    gaps = 32 * rng.integers(0, 3, w.n)
    gaps[::5] = 0
    return _place(w, rng.permutation(w.n), gaps)


def shifted(w, d):
    """Back to back in frame order, every offset plus d."""
    return w.out_offs + np.uint64(d), int(w.pcm.size) + d


def layouts(w, seed=1):
    """Every layout of a workload: (name, out_offs, length in samples, base_shift in elements)."""
    out = [("reversed",) + reversed_order(w) + (0,), ("shuffled_gaps",) + shuffled_gaps(w, seed) + (0,),
           ("shuffled_aligned",) + shuffled_aligned(w, seed + 1) + (0,)]
    out += [("shifted(%d)" % d,) + shifted(w, d) + (0,) for d in SHIFTS]
    # odd_base(k): the offsets of the parity tests; the POINTER handed to the decode is the buffer's base plus k elements -- the only
    # layout in which the offsets look aligned and the addresses are not
    out += [("odd_base(%d)" % k, w.out_offs, int(w.pcm.size), k) for k in ODD_BASES]
    return out


def layout(w, name, seed=1):
    for lay in layouts(w, seed):
        if lay[0] == name:
            return lay
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ workloads

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _families(w, picks):
    """The frames of `w` by family: picks = [(channels, block size, bits or None, how many of the first such frames; negative: the last)]."""
    idx = []
    for ch, bs, bits, k in picks:
        f = np.nonzero((w.channels == ch) & (w.block_sizes == bs) & ((w.bps == bits) if bits else True))[0]
        idx.append(f[:k] if k >= 0 else f[k:])
    return pc.subset(w, np.concatenate(idx))


def lean16(small=False):
    """Reaches the 16-bit tier.  Of pc.lean_workload(): two full waves of stereo frames of one block size (64 frames of 1024 samples,
    at most 4 / at most 8 taps), its frames that end in a lone last tile (block sizes 16 mod 32: a wave of 144 samples, one of 48
    and the wave with idle lanes) and its wave of mono frames.  `small` (the simulator runs every lane one after the other): one wave
    of 512-sample stereo frames for the two, and a ragged wave of 16 mono frames, last."""
    def make():
        w = pc.lean_workload()
        if small:
            return _families(w, [(2, 512, None, 32), (2, 144, None, 32), (2, 48, None, 32), (1, 1024, None, 16)])
        return _families(w, [(2, 1024, None, 64), (1, 1024, None, 64), (2, 144, None, 32), (2, 48, None, 37)])
    return _cached(("lean16", small), make)


def lean24(small=False):
    """Reaches the split tier: synth.config4(64) plus the first 96 frames of pc.lean24_workload() (24-bit stereo, up to 32 taps).
    `small` (the simulator): a wave of config 4 at 256 samples and, of pc.lean24_workload(), its waves of 144, 64 and 80 samples
    (lone last tiles, blocks that end with the prologue) and a ragged wave of eight 16-bit frames of more than 12 taps, last."""
    def make():
        if small:
            return synth.concat("lean24", [synth.config4(32, bs=256), _families(pc.lean24_workload(), [(2, 144, 24, 32), (2, 64, 24, 32), (2, 80, 24, 32),
                                                                                                        (2, 1024, 16, 8)])])
        return synth.concat("lean24", [synth.config4(64), pc.head(pc.lean24_workload(), 96)])
    return _cached(("lean24", small), make)


def general(small=False):
    """Reaches the general and the wave kernels' ragged rows: synth.small_mixed(96) plus pc.edge_workload() -- 1..8 channels, block
    sizes 1, 2, 9, 12, 24, 40 ..., 8 to 24 bits.  `small` (the simulator): the frames of at most 256 samples of both, 48 of the mix."""
    def make():
        m, e = synth.small_mixed(96), pc.edge_workload()
        if small:
            m, e = pc.subset(m, np.nonzero(m.block_sizes <= 256)[0][:48]), pc.subset(e, np.nonzero(e.block_sizes <= 256)[0])
        return synth.concat("general", [m, e])
    return _cached(("general", small), make)


def ms(small=False):
    """Reaches the movers: waves of plain mid/side pairs, both rows of a pair in one lane (pc.ms_mover_workload(lone_tail=True)).
    `small` (the simulator): a wave of its 48-sample frames (a lone last tile), one of its 32-sample frames, and a ragged wave of
    eight frames of 1040 samples (a lone last tile again), last."""
    def make():
        w = pc.ms_mover_workload(lone_tail=True)
        return _families(w, [(2, 48, None, 32), (2, 32, None, 32), (2, 1040, None, 8)]) if small else w
    return _cached(("ms", small), make)


WORKLOADS = {"lean16": lean16, "lean24": lean24, "general": general, "ms": ms}
STEREO_WORKLOADS = ("lean16", "lean24", "ms")        # (what CLX_COMPOSE has windows of stereo frames to deal in)


def for_mode(w, out_mode):
    """The frames of `w` an output mode takes (CLX_OUT_PCM16: at most 16 bits; CLX_OUT_PCM24: at most 24); None: it takes none."""
    def make():
        lim = {"pcm16": 16, "pcm24": 24}.get(out_mode, 32)
        keep = np.nonzero(w.bps <= lim)[0]
        return w if keep.size == w.n else pc.subset(w, keep) if keep.size else None
    return _cached(("mode", id(w), out_mode), make)


def damaged(w, seed=1, frac=0.3):
    """One bit flipped behind the header in about `frac` of the frames (as parity_cases.check_pcm16 does): the arena."""
    rng = np.random.default_rng(seed)
    arena = w.arena.copy()
    descs, _ = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)
    for i in range(w.n):
        if rng.uniform() < frac:
            lo, hi = int(w.offs[i]) + int(descs["header_bytes"][i]), int(w.offs[i] + w.lens[i])
            pos = int(rng.integers(8 * lo, 8 * hi))
            arena[pos >> 3] ^= (0x80 >> (pos & 7))
    return arena


# ------------------------------------------------------------------------------------------------ the check

def aligned_array(n, dtype, align=256):
    """A numpy array of n elements whose first byte lies on `align` bytes (what a device allocation gives)."""
    dt = np.dtype(dtype)
    raw = np.zeros(n * dt.itemsize + align, dtype=np.uint8)
    k = (-raw.ctypes.data) % align
    a = raw[k:k + n * dt.itemsize].view(dt)
    assert a.ctypes.data % align == 0
    return a


def sentinels(n, out_mode, first=0):
    """Element i of a buffer before the decode: (i * 2654435761 + 0x9e3779b9) truncated to the element -- no constant, so a stray write
    of any constant (the fill value included) shows."""
    i = np.arange(first, first + n, dtype=np.uint64)
    return (i * np.uint64(2654435761) + np.uint64(0x9e3779b9)).astype(pc.OUT_BITS[out_mode])


def reference(oracle, w, arena=None, verify_crc=True):
    """The oracle's decode of the workload (planar samples back to back in frame order, statuses, messages, end bits) -- once per
    workload, arena and CRC setting."""
    key = ("ref", id(w), None if arena is None else zlib.crc32(arena.tobytes()), bool(verify_crc))

    def make():
        a = w.arena if arena is None else arena
        ref = np.zeros(w.pcm.size, dtype=np.int32)
        r = oracle.decode_batch(a[:w.arena_len], w.offs, w.lens, out=ref, out_offs=w.out_offs, check_crc=verify_crc)
        ref.setflags(write=False)
        return ref, r
    return _cached(key, make)


def expected_buffer(oracle, w, out_offs, length, out_mode, base_shift=0, arena=None, verify_crc=True):
    """(before, after, masked, origin): the whole buffer as bits -- GUARD elements, then base_shift, then `length` samples, then GUARD --
    before the decode (sentinels) and after it by the oracle alone; `masked`: elements of failed frames' blocks; origin: the element
    `d_out` points to."""
    ref, r = reference(oracle, w, arena, verify_crc)
    eps = ELEMS_PER_SAMPLE[out_mode]
    origin = GUARD + base_shift
    n = origin + eps * int(length) + GUARD
    before = sentinels(n, out_mode)
    after = before.copy()
    masked = np.zeros(n, dtype=bool)
    sizes = _sizes(w)
    for i in range(w.n):
        a, c, bs, sz = int(w.out_offs[i]), int(w.channels[i]), int(w.block_sizes[i]), int(sizes[i])
        lo = origin + eps * int(out_offs[i])
        if int(r["statuses"][i]) != cx.OK:
            masked[lo:lo + eps * sz] = True
            continue
        v = ref[a:a + sz]
        blk = pc.block_in_mode(v, c, bs, w.bps[i], out_mode)
        after[lo:lo + eps * sz] = blk.view(pc.OUT_BITS[out_mode])
    return before, after, masked, origin


def where(w, out_offs, out_mode, origin, idx):
    """Which frame's block, gap or guard element `idx` of the whole buffer lies in."""
    eps = ELEMS_PER_SAMPLE[out_mode]
    sizes = _sizes(w)
    lo = origin + eps * np.asarray(out_offs, dtype=np.int64)
    hi = lo + eps * sizes.astype(np.int64)
    inside = np.nonzero((lo <= idx) & (idx < hi))[0]
    if inside.size:
        i = int(inside[0])
        return "element %d of the block of frame %d (%d ch, bs %d, %d bits, offset %d)" % (idx - int(lo[i]), i, int(w.channels[i]), int(w.block_sizes[i]),
                                                                                           int(w.bps[i]), int(out_offs[i]))
    if idx < int(lo.min()):
        return "the front guard, %d elements in front of the first block" % (int(lo.min()) - idx)
    if idx >= int(hi.max()):
        return "the rear guard, %d elements behind the last block" % (idx - int(hi.max()))
    before = int(np.argmax(np.where(hi <= idx, hi, -1)))
    return "a gap, %d elements behind the block of frame %d (%d ch, bs %d)" % (idx - int(hi[before]), before, int(w.channels[before]), int(w.block_sizes[before]))


def compare(w, out_offs, out_mode, origin, got, after, masked, ctx=""):
    """The whole buffer against the expected one, masked elements aside; names the first element that differs and where it lies."""
    got = np.ascontiguousarray(got).view(pc.OUT_BITS[out_mode])
    assert got.size == after.size, (got.size, after.size)
    bad = np.nonzero((got != after) & ~masked)[0]
    if bad.size:
        idx = int(bad[0])
        raise AssertionError("%s: %d elements differ (%s); the first is element %d (d_out%+d) = 0x%x, expected 0x%x: %s" % (
            ctx, bad.size, out_mode, idx, idx - origin, int(got[idx]), int(after[idx]), where(w, out_offs, out_mode, origin, idx)))


def check_results(w, r, res, ctx=""):
    """Statuses and messages of every frame, end bits of every OK frame: the oracle's."""
    st, ms_ = np.asarray(res["status"]), np.asarray(res["msg"])
    bad = np.nonzero((st != r["statuses"]) | (ms_ != r["msgs"]))[0]
    assert bad.size == 0, (ctx, [(int(i), int(st[i]), int(ms_[i]), int(r["statuses"][i]), int(r["msgs"][i])) for i in bad[:6]])
    ok = np.nonzero(st == cx.OK)[0]
    assert np.array_equal(np.asarray(res["end_bit"])[ok], r["end_bits"][ok]), ctx


def check_placed(oracle, decode_into, w, out_offs, length, out_mode, base_shift=0, arena=None, verify_crc=True, ctx=""):
    """Decode `w` (or its damaged `arena`) with every frame's block at out_offs[i] (samples) of a sentinel-filled buffer of `length`
    samples between guards, `d_out` = the buffer's first element behind the front guard plus base_shift elements, and compare the
    WHOLE buffer with the oracle's.  decode_into(arena, arena_len, descs, out_offs, buffer, origin, verify_crc) -> (buffer, results):
    `buffer` arrives as the sentinels (an aligned numpy array of the mode's element type as bits), `origin` is the element d_out
    points to."""
    before, after, masked, origin = expected_buffer(oracle, w, out_offs, length, out_mode, base_shift, arena, verify_crc)
    _, r = reference(oracle, w, arena, verify_crc)
    descs = _cached(("descs", id(w)), lambda: cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)[0])
    buf = aligned_array(before.size, before.dtype)
    buf[:] = before
    got, res = decode_into(w.arena if arena is None else arena, w.arena_len, descs, np.asarray(out_offs, dtype=np.uint64), buf, origin, verify_crc)
    check_results(w, r, res, ctx)
    compare(w, out_offs, out_mode, origin, got, after, masked, ctx)
    return r


def damaged_for(oracle, w, verify_crc=True):
    """damaged(w, seed) with the first seed for which the ORACLE fails between 10 % and 60 % of the frames (the choice looks at the
    inputs and the oracle only)."""
    for seed in range(1, 33):
        arena = damaged(w, seed)
        failed = int(np.sum(reference(oracle, w, arena, verify_crc)[1]["statuses"] != cx.OK))
        if 0.1 * w.n <= failed <= 0.6 * w.n:
            return arena
    raise AssertionError("no seed damages between 10 % and 60 % of %s" % w.name)


def assert_damage_share(r, n):
    """The damaged runs' condition on their inputs: between 10 % and 60 % of the frames fail by the ORACLE, so the comparison is never
    mostly masked and never all-OK."""
    failed = int(np.sum(r["statuses"] != cx.OK))
    assert 0.1 * n <= failed <= 0.6 * n, (failed, n)
