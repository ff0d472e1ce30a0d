"""The cases of the partitioned FFT reverberator (clx_reverb_windows_fft), shared by the simulator tests and the GPU tests: the edge
matrix of the blocks, the partitions of the response and the live ranges, in the kernel's own hop H and transform
length N.  Nothing here exceeds three blocks by eight rows, and nothing here touches a GPU."""
import numpy as np

import simlib_reverb_fft as sf
from norm_cases import GUARD, NAN_FILL, as_layout, from_layout, guarded, guards_intact, same_words

H, N = sf.HOP, sf.N
PAD_WORD = 0x7fc0beef                    # what data cells at t >= valid and taps at k >= ir_len hold: a NaN with a payload
LENS = [0, 1, 11, H, H + 1, 2 * H + 1]   # the responses' live taps, by response
K = 2 * H + 8                            # every row of d_ir is longer than its response
NAN_TAP = 5                              # where the response of the nan_tap case holds its NaN


def _case(name, rows, T, valid, index, keep, lens=LENS, offset=0, ir_offset=0, out_offset=0, kind="normal"):
    assert len(valid) == len(index) <= 6 and all(-1 <= j < len(lens) for j in index) and all(0 <= v <= T for v in valid)
    assert rows <= 8 and T <= 3 * H
    return dict(name=name, rows=rows, T=T, valid=list(valid), index=list(index), keep=keep, lens=list(lens), K=K, offset=offset,
                ir_offset=ir_offset, out_offset=out_offset, kind=kind)


def _mid(T):
    return min(H // 2 + 3, T - 2)


def _six(name, rows, T, variant, keep, offs):
    """Six windows.  a: the whole window and two more sharing the longest response (two partitions + 1 tap; one of them with a single
    live sample, one with T - 1: three different live tap counts of one response), an empty window, one cut mid-block under a
    partition + 1, one without a response.  b: the response without a live tap, eleven taps, one whole partition on a window cut
    mid-block, eleven taps on one sample, one tap on a window of H samples, a whole partition on three samples."""
    if variant == "a":
        valid, index = [T, 1, 0, _mid(T), T, T - 1], [5, 5, 1, 4, -1, 5]
    else:
        valid, index = [T, T, _mid(T), 1, H, 3], [0, 2, 3, 2, 1, 3]
    return _case(name, rows, T, valid, index, keep, offset=offs[0], ir_offset=offs[1], out_offset=offs[2])


def _matrix():
    cs = []
    # T of one block, one block + 1, two blocks + 3 and -- for a response longer than T -- a block + 5; rows 1, 2, 3, 8
    shapes = ((H, 1), (H, 3), (H + 1, 2), (H + 1, 8), (2 * H + 3, 3), (2 * H + 3, 1), (H + 5, 8), (H + 5, 2))
    for i, (T, rows) in enumerate(shapes):
        variant, keep = "ab"[i % 2], (i // 2 + i) % 2
        cs.append(_six("T%d_rows%d_%s%d" % (T, rows, variant, keep), rows, T, variant, keep, (i % 4, (i + 1) % 4, (3 * i + 1) % 4)))
    # the other keep_power on the shared response and on the long window
    cs.append(_six("T%d_rows2_a1" % (H + 5), 2, H + 5, "a", 1, (1, 3, 2)))
    cs.append(_six("T%d_rows1_b0" % (2 * H + 3), 1, 2 * H + 3, "b", 0, (3, 1, 1)))
    # a NaN tap in window 0's response, beside a finite window: window 0's live cells are unspecified, window 1's are what they are
    # without window 0
    cs.append(_case("nan_tap", 2, H + 5, [H + 5, H + 5], [0, 1], 1, lens=[11, H + 1], offset=1, ir_offset=1, out_offset=3, kind="nan_tap"))
    # energies of zero with keep_power: an all-zero signal (Ex == 0), a response of zeros (Ey == 0), and an ordinary window beside them
    cs.append(_case("zero_energy", 3, H + 5, [H + 5, H + 5, H + 5, 33], [1, 0, 1, 0], 1, lens=[H, 11], offset=2, ir_offset=3, out_offset=1,
                    kind="zeros"))
    return cs


MATRIX = _matrix()
NAMES = [c["name"] for c in MATRIX]


def case(name):
    return MATRIX[NAMES.index(name)]


def specified(c):
    """[B] bool: the windows whose live cells the definition fixes (every window but one with a non-finite live tap)."""
    return np.array([not (c["kind"] == "nan_tap" and k == 0) for k in range(len(c["valid"]))])


def data(c):
    """(x [B, rows, T], ir [N, K]) float32 (x in CT), seeded by the case's name.  Data cells at t >= valid[k] and taps at
    k >= ir_len[j] hold PAD_WORD: a NaN that must reach no cell and no sum, and words that must stay."""
    B, n_ir, rows, T = len(c["valid"]), len(c["lens"]), c["rows"], c["T"]
    rng = np.random.default_rng(sum(map(ord, c["name"])) + 4019)
    x = (rng.standard_normal((B, rows, T)) * rng.uniform(0.05, 2.0, (B, rows, 1))).astype(np.float32)
    ir = (rng.standard_normal((n_ir, c["K"])) * np.exp(-np.arange(c["K"]) / 400.0) * rng.uniform(0.2, 3.0, (n_ir, 1))).astype(np.float32)
    if c["kind"] == "nan_tap":
        ir[0, NAN_TAP] = np.float32("nan")
    if c["kind"] == "zeros":
        x[0] = np.float32(0.0)                               # window 0: Ex == 0
        x[0, 0, ::2] = np.float32(-0.0)
        ir[0] = np.float32(0.0)                              # windows 1 and 3: Ey == 0
        ir[0, 1::2] = np.float32(-0.0)
    for k, v in enumerate(c["valid"]):
        x[k, :, v:].view(np.uint32)[...] = PAD_WORD
    for j, n in enumerate(c["lens"]):
        ir[j, n:].view(np.uint32)[...] = PAD_WORD
    return x, ir


def masked(c, cells):
    """The cells with the unspecified ones (the live cells of a window with a non-finite tap) set to one word."""
    out = cells.copy()
    for k, ok in enumerate(specified(c)):
        if not ok:
            out[k, :, :c["valid"][k]] = np.float32(0.0)
    return out


_SIM, _WANT = {}, {}


def restated(name):
    """(cells, gains) of the case by simlib_reverb_fft.restate, computed once."""
    if name not in _WANT:
        c = case(name)
        x, ir = data(c)
        _WANT[name] = sf.restate(x, c["valid"], ir, c["lens"], c["index"], c["keep"])
    return _WANT[name]


def simulated(name, layout):
    """(cells [B, rows, T], gains [B]) of the case under the simulator in `layout`, computed once; the guard bands around the output
    and the gains, and every word of the data and of the responses, are checked here."""
    key = (name, layout)
    if key not in _SIM:
        c = case(name)
        x, ir = data(c)
        B, rows, T = x.shape
        flat, body = guarded(x.size, c["offset"])
        body[:] = as_layout(x, layout).reshape(-1)
        iflat, ibody = guarded(ir.size, c["ir_offset"])
        ibody[:] = ir.reshape(-1)
        oflat, obody = guarded(x.size, c["out_offset"])
        gflat, gbody = guarded(B, 1)
        before, ibefore = flat.view(np.uint32).copy(), iflat.view(np.uint32).copy()
        launched = sf.reverb_windows(body, c["valid"], ibody, c["lens"], c["index"], layout, obody, c["keep"], gbody, shape=(B, rows, T),
                                     n_ir=ir.shape[0], K=c["K"])
        assert launched, name
        assert np.array_equal(flat.view(np.uint32), before), (name, "the data was written")
        assert np.array_equal(iflat.view(np.uint32), ibefore), (name, "the responses were written")
        assert guards_intact(oflat, x.size, c["out_offset"]), (name, "a guard word around the output was written")
        assert guards_intact(gflat, B, 1), (name, "a guard word around the gains was written")
        assert not np.any(obody.view(np.uint32) == NAN_FILL), (name, "a cell of the output was not written")
        cells = from_layout(obody.reshape((B, T, rows) if layout == sf.TC else (B, rows, T)).copy(), layout)
        _SIM[key] = (cells, gbody.copy())
    return _SIM[key]
