"""The cases of the reverberator (clx_reverb_windows), shared by the simulator tests and the GPU tests: the edge matrix of the
tiling, the chunks of the response and the live ranges, in the kernel's own tile and chunk constants.  Nothing
here touches a GPU."""
import numpy as np

import simlib_reverb as sr
from norm_cases import GUARD, NAN_FILL, as_layout, from_layout, guarded, guards_intact, same_words

TILE, CHUNK, GROUP = sr.TILE, sr.CHUNK, sr.GROUP
PAD_WORD = 0x7fc0beef                    # what data cells at t >= valid and taps at k >= ir_len hold: a NaN with a payload
LENS = [0, 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, GROUP + 3]        # the responses' live taps, by response
K = 2 * CHUNK + 1 + 7                    # every row of d_ir is longer than its response


def _case(name, rows, T, valid, index, keep, lens=LENS, offset=0, ir_offset=0, out_offset=0, kind="normal"):
    assert len(valid) == len(index) <= 6 and all(-1 <= j < len(lens) for j in index) and all(0 <= v <= T for v in valid)
    return dict(name=name, rows=rows, T=T, valid=list(valid), index=list(index), keep=keep, lens=list(lens), K=K, offset=offset,
                ir_offset=ir_offset, out_offset=out_offset, kind=kind)


def _mid(T):
    return min(TILE // 2 + 3, T - 2)


def _six(name, rows, T, variant, keep, offs):
    """Six windows.  a: the whole window and two more sharing the longest response (two chunks + 1; one of them with a single live
    sample: a response longer than valid), an empty window, one cut mid-tile under a chunk + 1, one without a response.  b: the
    response without a live tap, one tap, a few taps (a ragged group), one chunk, on whole, mid-tile, one-sample and three-sample
    windows."""
    if variant == "a":
        valid, index = [T, 1, 0, _mid(T), T, T - 1], [4, 4, 1, 3, -1, 4]
    else:
        valid, index = [T, T, _mid(T), 1, T, 3], [0, 2, 5, 2, 1, 5]
    return _case(name, rows, T, valid, index, keep, offset=offs[0], ir_offset=offs[1], out_offset=offs[2])


def _matrix():
    cs = []
    # T of one tile, one tile + 1, two tiles + 3 and -- for a response longer than T -- a chunk + 5; rows 1, 2, 3, 8
    shapes = ((TILE, 1), (TILE, 3), (TILE + 1, 2), (TILE + 1, 8), (2 * TILE + 3, 1), (2 * TILE + 3, 3), (CHUNK + 5, 8), (CHUNK + 5, 2))
    for i, (T, rows) in enumerate(shapes):
        variant, keep = "ab"[i % 2], (i // 2 + i) % 2
        cs.append(_six("T%d_rows%d_%s%d" % (T, rows, variant, keep), rows, T, variant, keep, (i % 4, (i + 1) % 4, (3 * i + 1) % 4)))
    # the other variant and the other keep_power on the small shape and on one tile + 1
    cs.append(_six("T%d_rows2_a1" % (CHUNK + 5), 2, CHUNK + 5, "a", 1, (1, 3, 2)))
    cs.append(_six("T%d_rows3_b0" % (CHUNK + 5), 3, CHUNK + 5, "b", 0, (3, 1, 1)))
    cs.append(_six("T%d_rows1_b1" % (TILE + 1), 1, TILE + 1, "b", 1, (2, 2, 3)))
    # a NaN tap and an infinite tap: they reach the outputs t >= k and no other, which tells a skipped tap from one multiplied by
    # +0.0 (inf * 0 = NaN).  keep_power off, and the infinite tap over a positive signal: no invalid operation then makes a NaN
    # anew, whose sign and payload IEEE leaves to the machine -- the words are the same wherever the chain runs.
    cs.append(_case("nan_and_inf_taps", 2, CHUNK + 5, [CHUNK + 5, CHUNK + 5, 3, CHUNK + 5], [0, 1, 0, 1], 0, lens=[GROUP + 3, CHUNK + 1],
                    offset=1, ir_offset=1, out_offset=3, kind="special"))
    # energies of zero with keep_power: an all-zero signal (Ex == 0), a response of zeros (Ey == 0), and an ordinary window beside them
    cs.append(_case("zero_energy", 3, CHUNK + 5, [CHUNK + 5, CHUNK + 5, CHUNK + 5, 33], [1, 0, 1, 0], 1, lens=[CHUNK, GROUP + 3],
                    offset=2, ir_offset=3, out_offset=1, kind="zeros"))
    return cs


MATRIX = _matrix()
NAMES = [c["name"] for c in MATRIX]
NAN_TAP, INF_TAP = 5, CHUNK              # where the special responses hold their NaN and their +inf


def case(name):
    return MATRIX[NAMES.index(name)]


def data(c):
    """(x [B, rows, T], ir [N, K]) float32 (x in CT), seeded by the case's name.  Data cells at t >= valid[k] and taps at
    k >= ir_len[j] hold PAD_WORD: a NaN that must reach no cell and no sum, and words that must stay."""
    B, N, rows, T = len(c["valid"]), len(c["lens"]), c["rows"], c["T"]
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    x = (rng.standard_normal((B, rows, T)) * rng.uniform(0.05, 2.0, (B, rows, 1))).astype(np.float32)
    ir = (rng.standard_normal((N, c["K"])) * np.exp(-np.arange(c["K"]) / 60.0) * rng.uniform(0.2, 3.0, (N, 1))).astype(np.float32)
    if c["kind"] == "special":
        ir[0, NAN_TAP] = np.float32("nan")
        ir[1, INF_TAP] = np.float32("inf")
        ir[1, :INF_TAP] = np.abs(ir[1, :INF_TAP])
        x[1], x[3] = np.abs(x[1]) + np.float32(0.125), np.abs(x[3]) + np.float32(0.125)
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


_SIM, _WANT = {}, {}


def restated(name):
    """(cells, gains) of the case by simlib_reverb.restate, computed once."""
    if name not in _WANT:
        c = case(name)
        x, ir = data(c)
        _WANT[name] = sr.restate(x, c["valid"], ir, c["lens"], c["index"], c["keep"])
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
        launched = sr.reverb_windows(body, c["valid"], ibody, c["lens"], c["index"], layout, obody, c["keep"], gbody, shape=(B, rows, T),
                                     n_ir=ir.shape[0], K=c["K"])
        assert launched, name
        assert np.array_equal(flat.view(np.uint32), before), (name, "the data was written")
        assert np.array_equal(iflat.view(np.uint32), ibefore), (name, "the responses were written")
        assert guards_intact(oflat, x.size, c["out_offset"]), (name, "a guard word around the output was written")
        assert guards_intact(gflat, B, 1), (name, "a guard word around the gains was written")
        assert not np.any(obody.view(np.uint32) == NAN_FILL), (name, "a cell of the output was not written")
        cells = from_layout(obody.reshape((B, T, rows) if layout == sr.TC else (B, rows, T)).copy(), layout)
        _SIM[key] = (cells, gbody.copy())
    return _SIM[key]
