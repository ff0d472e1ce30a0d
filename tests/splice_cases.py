"""The cases of frame splicing (clx_splice_windows), shared by the simulator tests and the GPU tests: the edge matrix of the clamp,
the stride, the blocks and the tiling.  Every case is small: B <= 5, rows <= 256, at most a few tiles of 256 output
frames.  Nothing here touches a GPU."""
import numpy as np

import claxon_amd as cx
import simlib_splice as sp
from norm_cases import GUARD, NAN_FILL, as_layout, from_layout, guarded, guards_intact, same_words  # noqa: F401

TILE = sp.TILE
PAD_WORD = 0x7fc0beef                     # what the input's padding holds: a NaN that must never be read (one read poisons a FIR cell)
NAN_A, NAN_B, NEG_ZERO = 0x7fc12345, 0xffc00077, 0x80000000

_rng = np.random.default_rng(421)
PLANS = {
    "d1": cx.Splice.deltas(1, 2),
    "d2": cx.Splice.deltas(),                                # K = 3: a copy, m = 2, m = 4
    "d4w4": cx.Splice.deltas(4, 4),                          # m = 4, 8, 12, 16
    "lfr": cx.Splice.lfr(),                                  # K = 7 copies at -3 .. 3, stride 6
    "lfr_pad": cx.Splice.lfr(pad=7.25),
    "ctx": cx.Splice.context(2, 2),
    "ctx1": cx.Splice.context(1, 1),
    "sub3": cx.Splice.subsample(3),
    "sub64": cx.Splice.subsample(64),                        # a CT span of one row that does not fit the stage: shorter sub-tiles
    "k32": cx.Splice([(o, None) for o in range(-16, 16)]),
    "m16": cx.Splice([(0, _rng.uniform(-1, 1, 33))]),
    # copies and FIRs mixed, a zero coefficient, the widest offsets either way, an even stride, a pad that is not zero
    "mixed": cx.Splice([(-2, None), (1, [0.25, 0.5, 0.25]), (0, None), (5, [0.5, 0.0, -1.0, 0.0, 0.5]), (-64, None), (64, [1.0])], stride=2, pad=-1.5),
}


def _case(name, rows, T, valid, plan, offset=1, cells=()):
    """cells: ((window, row, frame, word), ..) planted into the live part of the batch."""
    return dict(name=name, rows=rows, T=T, valid=list(valid), plan=plan, offset=offset, cells=tuple(cells))


def _matrix():
    cs = []
    # V = 0, V = 1 (every tap clamps to the one frame), V below m = 4, V = T; B = 5 with mixed V
    cs.append(_case("short", 3, 9, [0, 1, 9, 2, 3], "d2"))
    # V below |o| = 64 and below m; B = 1
    cs.append(_case("v_below_offset", 2, 20, [5, 20, 1], "mixed", offset=3))
    cs.append(_case("b1", 4, 33, [33], "d4w4"))
    # T_out at the tile, one below and one above, at stride 1 and at stride 6; V ending mid-tile and a tile wholly in padding
    for T in (TILE - 1, TILE, TILE + 1):
        cs.append(_case("T%d" % T, 2, T, [T, T - 1, 130], "d1", offset=1 + 2 * (T % 2)))
    cs.append(_case("lfr_Tout256", 2, 6 * TILE - 5, [6 * TILE - 5, 6 * TILE - 6, 700], "lfr"))
    cs.append(_case("lfr_Tout257", 2, 6 * TILE + 1, [6 * TILE + 1, 6 * TILE, 13], "lfr_pad", offset=3))
    # a stride that does not divide V: s = 6 with V = 13 (three frames), V = 1 (one), V = 12, 7
    cs.append(_case("s6", 3, 13, [13, 1, 12, 7], "lfr", offset=3))
    cs.append(_case("sub3", 5, 100, [100, 98, 1], "sub3"))
    # rows 1, 13 (K * rows = 39: no multiple of 4), 80 (TC: three sub-tiles of 16 frames, the second half live, the third dead;
    # CT: chunks of 5 rows) and 256 (TC with m = 16: the rows do not fit the stage at once)
    cs.append(_case("rows1", 1, 300, [300, 257, 9], "d2"))
    cs.append(_case("rows13", 13, 70, [70, 33, 0], "d2", offset=3))
    cs.append(_case("rows80_lfr", 80, 200, [200, 100], "lfr"))
    cs.append(_case("rows256", 256, 20, [20, 7], "ctx1", offset=3))
    cs.append(_case("rows256_m16", 256, 40, [40, 9], "m16"))
    # K = 32 copies, and at 256 rows the 8192 output rows that are the most
    cs.append(_case("k32", 5, 40, [40, 17], "k32"))
    cs.append(_case("k32_rows256", 256, 5, [5, 2], "k32", offset=3))
    # m = 16 over two tiles, the second wholly padding for the last window
    cs.append(_case("m16", 3, 300, [300, 257, 16], "m16"))
    # mixed copy and FIR blocks at stride 2 with pad = -1.5; T_out = 265
    cs.append(_case("mixed", 7, 530, [530, 511, 100], "mixed", offset=3))
    # a copy block moves words: NaN payloads and -0.0 survive
    cs.append(_case("copy_words", 3, 30, [30, 25], "ctx",
                    cells=[(0, 1, 0, NAN_A), (0, 2, 29, NEG_ZERO), (0, 0, 10, NAN_B), (1, 0, 24, NAN_A), (1, 2, 0, NEG_ZERO), (1, 1, 12, NEG_ZERO)]))
    # stride 64: T_out = 300
    cs.append(_case("sub64", 2, 19200, [19200, 12345], "sub64"))
    return cs


MATRIX = _matrix()
NAMES = [c["name"] for c in MATRIX]


def case(name):
    return MATRIX[NAMES.index(name)]


def plan(c):
    return PLANS[c["plan"]]


def data(c):
    """The case's batch [B, rows, T] float32 (CT), seeded by its name: unit normals with a per-row offset; padding holds PAD_WORD."""
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    x = (rng.standard_normal((B, rows, T)) * rng.uniform(0.5, 3.0, (B, rows, 1)) + rng.uniform(-4, 4, (B, rows, 1))).astype(np.float32)
    for k, n in enumerate(c["valid"]):
        x[k, :, n:].view(np.uint32)[...] = PAD_WORD
    for k, r, t, word in c["cells"]:
        assert t < c["valid"][k]
        x.view(np.uint32)[k, r, t] = word
    return x


def out_shape(c):
    return len(c["valid"]), plan(c).n_out(c["rows"]), plan(c).frames_out(c["T"])


_SIM, _REST = {}, {}


def simulated(name, layout):
    """The cells [B, K * rows, T_out] of the case under the simulator in `layout`, computed once; the guard bands around the output
    are checked here, and so is that the input keeps its words and that every output word was written."""
    key = (name, layout)
    if key not in _SIM:
        c = case(name)
        x = data(c)
        B, R, To = out_shape(c)
        src = as_layout(x, layout)
        before = src.copy()
        flat, body = guarded(B * R * To, c["offset"])
        sp.splice_windows(src, body, c["valid"], layout, plan(c), shape=x.shape)
        Fs, Rc, H = sp.last_shape()
        assert ((Fs - 1) * plan(c).stride + 1 + 2 * H) * Rc <= sp.STAGE_WORDS, (name, "the sub-tile's span does not fit the stage")
        assert guards_intact(flat, B * R * To, c["offset"]), (name, "a guard word around the output was written")
        assert same_words(src, before), (name, "the input was written")
        assert not np.any(body.view(np.uint32) == NAN_FILL), (name, "an output word was not written")
        _SIM[key] = from_layout(body.reshape((B, To, R) if layout == sp.TC else (B, R, To)).copy(), layout)
    return _SIM[key]


def restated(name):
    """simlib_splice.restate of the case, computed once."""
    if name not in _REST:
        c = case(name)
        _REST[name] = sp.restate(data(c), c["valid"], plan(c))
    return _REST[name]
