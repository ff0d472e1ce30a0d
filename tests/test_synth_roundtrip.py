"""The synthetic generator is a miniature FLAC encoder written independently of the oracle:
oracle(decode(encode(pcm))) == pcm is therefore a two-sided check."""
import numpy as np
import pytest

import synth
from claxon_msgs import STATUS


def _decode(oracle, w, nthreads=1):
    out = np.full(w.pcm.size, 0x5a5a5a5a, dtype=np.int32)
    if w.bare_subframes:
        r = oracle.decode_subframes(w.arena[:w.arena_len], w.offs, w.block_sizes, w.bps, out=out, out_offs=w.out_offs)
    else:
        r = oracle.decode_batch(w.arena[:w.arena_len], w.offs, w.lens, out=out, out_offs=w.out_offs,
                                check_crc=True, nthreads=nthreads)
    return r, out


@pytest.mark.parametrize("make", [
    lambda: synth.config2(64), lambda: synth.config3(64), lambda: synth.config4(32),
    lambda: synth.config5_unique(96), lambda: synth.small_mixed(160),
], ids=["config2", "config3", "config4", "config5", "small_mixed"])
def test_roundtrip(oracle, make):
    w = make()
    r, out = _decode(oracle, w, nthreads=2)
    assert np.all(r["statuses"] == STATUS["CLX_OK"]), np.unique(r["msgs"])
    assert r["samples"] == w.total_samples
    assert np.array_equal(out, w.pcm)
    # every frame is consumed exactly: end_bit rounded up to a byte + 2 CRC bytes == frame length
    if not w.bare_subframes:
        assert np.array_equal((r["end_bits"] + 7) // 8 + 2, w.lens.astype(np.uint64))


def test_config_shapes():
    w = synth.config3(8)
    assert w.n == 8 and w.total_samples == 8 * 2 * 4096
    assert set(w.assignments.tolist()) == {synth.CH_MID_SIDE}
    assert w.arena.size % 16 == 0 and w.arena.size >= w.arena_len + 32
    assert w.algorithmic_bytes == w.compressed_bytes + 4 * w.total_samples
    # frame header: ff f8 | c9 (4096, 44.1k) | a8 (M/S, 16 bit)
    assert w.arena[:4].tolist() == [0xff, 0xf8, 0xc9, 0xa8]


def test_restamp(oracle):
    w = synth.config3(2)
    frame = w.arena[int(w.offs[1]):int(w.offs[1] + w.lens[1])].copy()
    info0, s0 = oracle.frame_decode(frame)
    assert synth.lib().synth_restamp_frame(frame.ctypes.data, frame.size, 77) == 1
    info1, s1 = oracle.frame_decode(frame)          # CRC-8 and CRC-16 still valid
    assert info1.status == STATUS["CLX_OK"] and info1.time == 77 * 4096
    assert np.array_equal(s0, s1)


def test_roundtrip_long_blocks_and_escapes(oracle):
    """Blocks of 4 609 .. 65 535 samples (the 16-bit block-size code above 4 608, 1 .. 8 channels, 8 .. 24 bits) decode back to their
    source; escape-coded partitions and the invalid residual headers come out as the reference's errors; a verbatim eight-channel
    24-bit frame of 65 535 samples fits the arena's estimate."""
    import parity_cases as pc
    w = pc.long_block_workload(light=True)
    r, out = _decode(oracle, w)
    assert np.all(r["statuses"] == STATUS["CLX_OK"]) and np.array_equal(out, w.pcm)
    assert np.array_equal((r["end_bits"] + 7) // 8 + 2, w.lens.astype(np.uint64))
    big = (w.block_sizes > 4608) & (w.block_sizes != 8192) & (w.block_sizes != 16384) & (w.block_sizes != 32768)
    for i in np.nonzero(big)[0]:                                  # header byte 2: block-size code 7 (16 bits of bs - 1 follow)
        assert w.arena[int(w.offs[i]) + 2] >> 4 == 7, int(w.block_sizes[i])
    e = pc.escape_workload()
    r, _ = _decode(oracle, e)
    for i, k in enumerate(e.kinds):
        s, m = pc.ESCAPE_KINDS[k]
        assert int(r["statuses"][i]) == STATUS[s] and (m is None or int(r["msgs"][i]) == pc.MSG[m]), (i, k)
    rng = np.random.default_rng(3)
    pcm = rng.integers(-(1 << 23), 1 << 23, size=(1, 8, 65535)).astype(np.int32)
    fp = synth.FrameParams(0, 0, 0)
    for c in range(8):
        fp.sf[c] = synth.sf(synth.SF_VERBATIM, 0, 0, 0)
    v = synth.encode_frames("verbatim 8 x 65535 x 24", pcm, 8, 65535, 24, [fp])
    assert v.lens[0] > 8 * 65535 * 3
    r, out = _decode(oracle, v)
    assert int(r["statuses"][0]) == STATUS["CLX_OK"] and np.array_equal(out, v.pcm)


def test_escape_partition_layout():
    """The escape code and what follows it, as the FLAC format lays them out: parameter 0b1111 (Rice) / 0b11111 (Rice2), a 5-bit width,
    then the partition's residuals as raw two's complement numbers of that width."""
    x = np.array([0, 3, -5, 7, 100, -100, 2, 1], dtype=np.int32)
    for rice2 in (0, 1):
        w = synth.encode_subframes("esc", x[None], 8, 16, [synth.sf(synth.SF_FIXED, 0, 0, 0, force_rice2=rice2, escape=0)])
        bits = "".join(format(int(b), "08b") for b in w.arena[:w.arena_len])
        pos = 8                                                   # subframe header: 0, type 001000 (FIXED 0), no wasted bits
        assert bits[pos:pos + 2] == ("01" if rice2 else "00") and bits[pos + 2:pos + 6] == "0000"
        pos += 6
        k = 5 if rice2 else 4
        assert bits[pos:pos + k] == "1" * k
        pos += k
        nb = int(bits[pos:pos + 5], 2)
        assert nb == 8                                            # -100 .. 100 take 8 bits
        pos += 5
        vals = [int(bits[pos + nb * i:pos + nb * (i + 1)], 2) for i in range(8)]
        assert [v - (1 << nb) if v >> (nb - 1) else v for v in vals] == x.tolist()

    # an escape in a Rice residual whose other partition wants a parameter above 14 (24-bit noise): the residual stays Rice, the escape
    # 0b1111, the other parameter 14
    y = np.concatenate([x, np.random.default_rng(5).integers(-(1 << 16), 1 << 16, 8)]).astype(np.int32)
    w = synth.encode_subframes("esc", y[None], 16, 24, [synth.sf(synth.SF_FIXED, 0, 0, 1, escape=0)])
    bits = "".join(format(int(b), "08b") for b in w.arena[:w.arena_len])
    assert bits[8:10] == "00" and bits[10:14] == "0001" and bits[14:18] == "1111"
    nb = int(bits[18:23], 2)
    assert nb == 8 and bits[23 + 8 * nb:23 + 8 * nb + 4] == format(14, "04b")
