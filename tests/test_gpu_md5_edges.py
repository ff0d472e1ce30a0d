"""clx_k_md5 on the GPU against hashlib, over the case matrix that test_md5_sim.py runs under the wave simulator (md5_cases.py): every
message length from 0 to 300 bytes at every width -- the two-block padding of 56..63 bytes left over among them --, every source
format with every width it can hold at lengths round the group sizes (the 13 instances of clx_md5::stream, their partial groups and
the F32 tail's conversion), the F32 extremes, streams that start at odd samples in a buffer at every byte offset from the 16-byte grid
(the unaligned 16-byte loads), and 150 streams of mixed width in one call.  Every digest of every call is compared; the expected
ones are hashlib's alone.  Left to the simulator: the stream next to an inaccessible page (a stray load there would be a fault) and
the refused arguments (test_gpu_md5.py has those of the device build)."""
import pytest
import torch

import claxon_amd as cx
import md5_cases as mc
from gpu_guarded import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    """The runner of md5_cases' checks: Context.md5_streams on a uint8 device tensor, sliced so that its first byte lies byte_offset
    bytes behind a 16-byte boundary."""
    ctx = cx.Context(0, wait_s=120)

    def go(buf, fmt, first, counts, bps, byte_offset=0):
        big = torch.zeros(buf.size + 64, dtype=torch.uint8, device=DEV)
        base = (-big.data_ptr()) % 16 + byte_offset
        dev = big[base:base + buf.size]
        dev.copy_(torch.from_numpy(buf))
        assert dev.data_ptr() % 16 == byte_offset and dev.is_contiguous()
        return ctx.md5_streams(dev, fmt, first, counts, bps)

    return go


def _report(name, done):
    print("%s: %d calls, %d digests compared with hashlib, 0 differ" % ((name,) + done))


def test_every_message_length_to_300_bytes(run):
    done = mc.check_every_message_length(run)
    assert done == (4, 301 + 151 + 101 + 76)
    _report("lengths 0..300 bytes at widths 1..4", done)


def test_every_format_with_every_width_it_holds(run):
    done = mc.check_every_format_and_width(run)
    assert done == (39, 39 * 13)
    _report("every format with every bps", done)


def test_f32_extremes_scale_back_exactly(run):
    done = mc.check_f32_extremes(run)
    assert done == (8, 24)
    _report("F32 extremes", done)


def test_any_alignment_of_a_stream_start(run):
    done = mc.check_any_alignment_of_a_stream_start(run)
    assert done == (80, 400)
    _report("odd sample starts and byte offsets 1..15", done)


def test_many_streams_of_very_different_lengths_in_one_call(run):
    done = mc.check_many_streams_of_mixed_width(run)
    assert done == (2, 300)
    _report("150 streams of mixed width, formats 4 and F32", done)
