"""clx_k_window on the GPU against numpy slicing of the same 32-bit words, over the case matrix that test_window_sim.py runs under the
wave simulator (window_cases.py): Context.gather_windows on raw tensors of arbitrary bit patterns, every L round the vector, wave and
tile sizes with 1..8 channels (each put_tile_ct<C>), both layouts, src_first mod 8 times valid in {0, 1, L-1, L}; outputs 1..3 words
off the 16-byte grid, where neighbouring rows share a vector that concurrent workgroups write (the simulator runs them in a fixed
order); B = 0, 1, 70; windows of several tiles, CT's fast path across tiles among them; overlapping and descending windows; and an
eight-channel stream through StreamSet.read().  The output is a slice of a buffer of NaN patterns with 64 guard words either side
(gpu_guarded.py), compared as uint32 on the host: the guards are intact, no word keeps the fill, every word is numpy's.  Left to the
simulator: the window next to an inaccessible page (a stray load there would be a fault) and the refused arguments."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import window_cases as wc
from gpu_guarded import DEV, device_out, written
from test_gpu_windows import Case, _check_reads, _stream

pytestmark = pytest.mark.gpu
assert (wc.TC, wc.CT) == (cx.WINDOW_TC, cx.WINDOW_CT)


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


@pytest.fixture(scope="module")
def run(ctx):
    """The runner of window_cases' checks.  written() raises for a guard word that changed, so the flag it returns is always True."""

    def go(src, src_first, valid, L, C, layout, out_offset_words=0):
        n = len(src_first) * L * C
        dev = torch.from_numpy(src.view(np.float32)).to(DEV)
        flat, out = device_out(n, out_offset_words)
        assert out.data_ptr() % 16 == 4 * out_offset_words
        torch.cuda.synchronize()
        ctx.gather_windows(dev, src_first, valid, L, C, layout, out)
        torch.cuda.synchronize()
        return written(flat, n, (len(src_first), L, C, layout, out_offset_words), out_offset_words), True

    return go


def _report(name, done):
    print("%s: %d calls, %d words compared with numpy, 0 differ" % ((name,) + done))


@pytest.mark.parametrize("layout", wc.LAYOUTS)
@pytest.mark.parametrize("C", wc.CHANNELS)
def test_lengths_alignments_and_valid_counts(run, C, layout):
    done = wc.check_lengths_alignments_and_valid_counts(run, C, layout)
    assert done == (11, 32 * C * sum(wc.LENGTHS))
    _report("lengths, alignments and valid counts, C = %d, layout %d" % (C, layout), done)


@pytest.mark.parametrize("layout", wc.LAYOUTS)
def test_output_on_a_4_byte_boundary_only(run, layout):
    done = wc.check_output_on_a_4_byte_boundary_only(run, layout)
    assert done[0] == 15
    _report("output 1..3 words off the 16-byte grid, layout %d" % layout, done)


@pytest.mark.parametrize("layout", wc.LAYOUTS)
@pytest.mark.parametrize("B", wc.BATCHES)
def test_batch_sizes(run, B, layout):
    done = wc.check_batch_sizes(run, B, layout)
    assert done == (3, B * (257 * 2 + 256 * 3 + 1000 * 2))
    _report("B = %d, layout %d" % (B, layout), done)


@pytest.mark.parametrize("layout", wc.LAYOUTS)
def test_a_window_of_several_tiles(run, layout):
    done = wc.check_a_window_of_several_tiles(run, layout)
    assert done[0] == 4 and (2 * 4096, 2) in wc.TILES
    _report("windows of several tiles, layout %d" % layout, done)


@pytest.mark.parametrize("layout", wc.LAYOUTS)
def test_overlapping_and_descending_windows(run, layout):
    done = wc.check_overlapping_and_descending_windows(run, layout)
    assert done == (1, 10 * 65 * 2)
    _report("overlapping and descending windows, layout %d" % layout, done)


@pytest.mark.parametrize("length", (100, 101))
def test_eight_channels_through_read(ctx, length):
    """A synthetic 8-channel 16-bit stream of 5 frames of 128 samples: windows round every frame boundary, both layouts, against
    slices of load().  L = 100 takes put_tile_ct<8> (rows on the 16-byte grid), L = 101 the generic rows."""
    c = Case(ctx, *_stream(np.random.default_rng(808), 5, 8, 128, 16))
    assert c.C == 8 and c.T == 5 * 128 and c.bounds[-1] == c.T
    starts = sorted({max(b + d, 0) for b in c.bounds for d in (-1, 0, 1)})
    _check_reads(c, starts, length)
    print("8 channels through read(), L = %d: 2 calls, %d words compared with load(), 0 differ" % (length, 2 * len(starts) * length * 8))
    c.set.close()
