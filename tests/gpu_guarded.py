"""The guarded output buffer of the GPU tests that compare words: the output is a slice of a device buffer filled with a NaN pattern,
GUARD words of the same pattern before it and GUARD behind.  After the call the guards still hold the pattern and no word of the
slice does (the kernels own their whole output)."""
import numpy as np
import torch

DEV = "cuda:0"
NAN_FILL = 0x7fc0dead            # a quiet NaN with a payload: what the output and its guards hold before the call
GUARD = 64                       # words before the output and behind it


def device_out(n, offset_words=0):
    """(the whole buffer, the n floats of it that the call may write), every word NAN_FILL.  The slice starts offset_words words
    behind a 16-byte boundary (GUARD words are a whole number of 16-byte vectors and torch's allocations start on one)."""
    flat = torch.from_numpy(np.full(n + 2 * GUARD + offset_words, NAN_FILL, dtype=np.uint32).view(np.float32)).to(DEV)
    assert flat.data_ptr() % 16 == 0
    return flat, flat[GUARD + offset_words:GUARD + offset_words + n]


def written(flat, n, what, offset_words=0):
    """The n output words on the host, after the checks that the guards are untouched and that every output word was written."""
    h = flat.cpu().numpy().view(np.uint32)
    at = GUARD + offset_words
    assert np.all(h[:at] == NAN_FILL), (what, "a guard word before the output was written")
    assert np.all(h[at + n:] == NAN_FILL), (what, "a guard word behind the output was written")
    body = h[at:at + n]
    left = int(np.count_nonzero(body == NAN_FILL))
    assert left == 0, (what, "%d of %d output words still hold the fill pattern" % (left, n))
    return body
