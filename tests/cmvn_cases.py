"""The cases of global and sliding-window CMVN (clx_cmvn_global_windows, clx_cmvn_sliding_windows), shared by the simulator tests and
the GPU tests: the edge matrix of the statistics window, the groups of 32, the tiling and the row chunk.  Every
case is small: B <= 6, three tiles of 256 frames at the most.  Nothing here touches a GPU."""
import numpy as np

import simlib_cmvn as sc
from norm_cases import GUARD, NAN_FILL, as_layout, from_layout, guarded, guards_intact, same_words  # noqa: F401

TILE, RC = sc.TILE, sc.RC
T3 = 2 * TILE + 37                       # two whole tiles and a ragged one
PAD_WORD = 0x7fc0beef                    # what the input's padding holds: a NaN that must never be read (one read poisons a sum)
SNAN, NEG_ZERO = 0x7f800001, 0x80000000  # signalling patterns for the padding of the global cases
WINDOWS = (1, 2, 31, 32, 33, 300, 600, 1024)
ROWS = (1, 3, RC - 1, RC, RC + 1, 13, 3, 1)


def _clip(vs, T):
    out = []
    for v in vs:
        v = min(max(int(v), 0), T)
        if v not in out:
            out.append(v)
    return out[:6]


def _sliding(name, rows, T, valid, N, M, center, norm_vars, pad=0.0, offset=1, kind="logmel"):
    return dict(name=name, rows=rows, T=T, valid=list(valid), N=N, M=M, center=int(center), norm_vars=int(norm_vars), pad=pad, offset=offset,
                kind=kind)


def _sliding_matrix():
    cs = []
    i = 0
    for N in WINDOWS:
        ms = [m for m in (1, N, 100) if m <= N]
        for center in (0, 1):
            for nv in (0, 1):
                for half in "ab":
                    M = ms[i % len(ms)]
                    # a: V = 0, 1 and around the group of 32, and the whole T; b: around M, N and the tile
                    valid = _clip((0, 1, 31, 32, 33, T3), T3) if half == "a" else _clip((M - 1, M, N, N + 1, 256, 257), T3)
                    cs.append(_sliding("N%d_c%d_v%d_%s" % (N, center, nv, half), ROWS[i % len(ROWS)], T3, valid, N, M, center, nv,
                                       pad=(0.0, -1.5)[i % 2], offset=i % 4))
                    i += 1
    # 80 rows (ten whole chunks; TC rows of 320 bytes) and the 560 stacked rows of the low-frame-rate front end
    cs.append(_sliding("rows80", 80, T3, [T3, 300], 300, 100, 1, 0))
    cs.append(_sliding("rows80_v", 80, 300, [300, 257], 600, 100, 0, 1, offset=3))
    cs.append(_sliding("rows560", 560, 70, [70, 33, 0], 33, 10, 1, 1, offset=2))
    # cancelling pairs of magnitude 2^50 among the cells: the double sums round where it shows, so the ORDER is in the words
    for center in (0, 1):
        for nv in (0, 1):
            cs.append(_sliding("wide_c%d_v%d" % (center, nv), 3, T3, [T3, 257, 100, 33], 300, 100, center, nv, offset=1 + center, kind="wide"))
    # cells that are not finite: IEEE inside the windows that reach them, nothing elsewhere
    cs.append(_sliding("nonfinite", 2, 300, [300, 200], 32, 8, 1, 1, kind="nonfinite"))
    cs.append(_sliding("nonfinite_u", 2, 300, [300, 200], 64, 8, 0, 0, kind="nonfinite"))
    # the x-vector recipe and Kaldi's defaults
    cs.append(_sliding("xvector", 13, T3, [T3, 400, 299, 7], 300, 100, 1, 0))
    cs.append(_sliding("kaldi_default", 13, 700, [700, 601, 99], 600, 100, 0, 0, offset=3))
    return cs


SLIDING = _sliding_matrix()
SLIDING_NAMES = [c["name"] for c in SLIDING]
FINITE_NAMES = [c["name"] for c in SLIDING if c["kind"] != "nonfinite"]
# the cases the GPU runs: both layouts of each; both center values, norm_vars on and off, the three-tile T, every row count, 560 rows
GPU_SLIDING = ["N300_c0_v0_a", "N300_c0_v1_a", "N300_c1_v0_a", "N300_c1_v1_b", "N1024_c0_v0_a", "N1024_c1_v1_b", "N33_c0_v1_b", "N1_c0_v0_a",
               "N600_c1_v1_a", "rows80", "rows80_v", "rows560", "wide_c0_v1", "wide_c1_v0", "wide_c1_v1", "nonfinite", "xvector", "kaldi_default"]


def sliding_case(name):
    return SLIDING[SLIDING_NAMES.index(name)]


def _rng(name):
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def data(c):
    """The case's batch [B, rows, T] float32 (CT), seeded by its name: log-mel-like cells, about N(-5, 2^2) with a per-row offset;
    padding holds PAD_WORD."""
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    rng = _rng(c["name"])
    x = rng.standard_normal((B, rows, T)) * 2.0 - 5.0 + rng.uniform(-1, 1, (B, rows, 1))
    x = x.astype(np.float32)
    if c.get("kind") == "wide":
        # a third of a row's cells are neighbouring pairs (+v, -v) of magnitude 2^50 (some split by a group's edge): the exact sums
        # stay small, every addition of a v rounds at about 2^-3, and so the order of the additions shows in the float32 cell
        for k in range(B):
            for r in range(rows):
                at = 3 * rng.permutation((T - 2) // 3)[:T // 6] + 1
                v = (rng.uniform(0.5, 1.0, at.size) * 2.0 ** 50).astype(np.float32)
                x[k, r, at], x[k, r, at + 1] = v, -v
    if c.get("kind") == "nonfinite":
        for k, r, t, word in ((0, 0, 40, 0x7f800000), (0, 1, 150, 0x7fc00123), (1, 0, 199, 0xff800000), (1, 1, 0, 0x7fc00001)):
            x.view(np.uint32)[k, r, t] = word
    for k, n in enumerate(c["valid"]):
        x[k, :, n:].view(np.uint32)[...] = PAD_WORD
    return x


_SIM, _REST = {}, {}


def simulated_sliding(name, layout):
    """The cells [B, rows, T] of the case under the simulator in `layout`, computed once; the guard words around the output are
    checked here, and so is that the input keeps its words and that every output word was written."""
    key = (name, layout)
    if key not in _SIM:
        c = sliding_case(name)
        x = data(c)
        B, rows, T = x.shape
        src = as_layout(x, layout)
        before = src.copy()
        flat, body = guarded(B * rows * T, c["offset"])
        sc.sliding_windows(src, body, c["valid"], layout, c["N"], c["M"], c["center"], c["norm_vars"], c["pad"], shape=x.shape)
        assert sc.last_shape()[1] == min(rows, RC) and sc.last_shape()[2] <= sc.MAX_SPAN
        assert guards_intact(flat, B * rows * T, c["offset"]), (name, "a guard word around the output was written")
        assert same_words(src, before), (name, "the input was written")
        assert not np.any(body.view(np.uint32) == NAN_FILL), (name, "an output word was not written")
        _SIM[key] = from_layout(body.reshape((B, T, rows) if layout == sc.TC else (B, rows, T)).copy(), layout)
    return _SIM[key]


def restated_sliding(name):
    """simlib_cmvn.restate_sliding of the case, computed once."""
    if name not in _REST:
        c = sliding_case(name)
        _REST[name] = sc.restate_sliding(data(c), c["valid"], c["N"], c["M"], c["center"], c["norm_vars"], c["pad"])
    return _REST[name]


# ---- the global cases ---------------------------------------------------------------------------------------------------------------

def _global(name, rows, T, valid, pad=0.0, offset=0):
    return dict(name=name, rows=rows, T=T, valid=list(valid), pad=pad, offset=offset)


GLOBAL = [
    _global("g_rows3", 3, T3, [T3, 0, 1, 257, 256, 33]),                      # 1 647 cells a window
    _global("g_two_tiles", 5, 1031, [1031, 1030, 7], pad=-1.5, offset=1),      # 5 155 cells: two tiles of 4 096, T no multiple of 4
    _global("g_rows13", 13, 70, [70, 33, 0, 69], offset=3),                    # T = 2 mod 4: in CT the rows share vectors
    _global("g_rows80", 80, 37, [37, 36, 1], pad=7.25, offset=2),
    _global("g_rows560", 560, 70, [70, 12], offset=1),
    _global("g_rows8192", 8192, 3, [3, 2, 0], offset=3),
    _global("g_b1", 1, 9, [5]),
]
GLOBAL_NAMES = [c["name"] for c in GLOBAL]


def global_case(name):
    return GLOBAL[GLOBAL_NAMES.index(name)]


def global_data(c):
    """(x [B, rows, T] float32 with signalling NaNs and -0.0 in the padding, shift, scale)."""
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    rng = _rng(c["name"])
    x = (rng.standard_normal((B, rows, T)) * 2.0 - 5.0).astype(np.float32)
    for k, n in enumerate(c["valid"]):
        w = x[k, :, n:].view(np.uint32)
        w[...] = SNAN
        w[:, 1::2] = NEG_ZERO
    shift = rng.uniform(3.0, 7.0, rows).astype(np.float32)
    scale = rng.uniform(0.3, 0.9, rows).astype(np.float32)
    return x, shift, scale


_GSIM = {}


def simulated_global(name, layout):
    """The cells [B, rows, T] of the global case under the simulator in `layout`, computed once, in place inside guard words."""
    key = (name, layout)
    if key not in _GSIM:
        c = global_case(name)
        x, shift, scale = global_data(c)
        B, rows, T = x.shape
        flat, body = guarded(B * rows * T, c["offset"])
        body[...] = as_layout(x, layout).reshape(-1)
        sc.global_windows(body, c["valid"], layout, shift, scale, c["pad"], shape=x.shape)
        assert guards_intact(flat, B * rows * T, c["offset"]), (name, "a guard word around the batch was written")
        _GSIM[key] = from_layout(body.reshape((B, T, rows) if layout == sc.TC else (B, rows, T)).copy(), layout)
    return _GSIM[key]
