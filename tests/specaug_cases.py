"""The cases of SpecAugment (clx_specaug_windows), shared by the simulator tests and the GPU tests: the edge matrix of the warp, the
masks, the fill and the tiling.  Every case is small: B <= 6, rows <= 256, T a few tiles of 256 frames (one case
spans two 4096-frame chunks of the mean's sum, at one row).  Nothing here touches a GPU."""
import numpy as np

import simlib_specaug as ss
from norm_cases import GUARD, NAN_FILL, as_layout, from_layout, guarded, guards_intact, same_words  # noqa: F401

TILE = ss.TILE
PAD_WORD = 0x7fc0beef                     # what padding holds: a NaN with a payload that must come back as it is (not gpu_guarded's fill)
NAN_A, NAN_B, INF = 0x7fc12345, 0xffc00077, 0x7f800000


def _case(name, rows, T, valid, warp=None, fm=None, tm=None, fill="mean", offset=1, cells=(), finite=True):
    """cells: ((window, row, frame, word), ..) planted into the batch; finite: every live cell is finite (the reference applies)."""
    B = len(valid)
    return dict(name=name, rows=rows, T=T, valid=list(valid), warp=None if warp is None else np.array(warp, dtype=np.int64).reshape(B, 2),
                fm=None if fm is None else np.array(fm, dtype=np.int64).reshape(B, -1, 2),
                tm=None if tm is None else np.array(tm, dtype=np.int64).reshape(B, -1, 2), fill=fill, offset=offset, cells=tuple(cells), finite=finite)


def _spread(B, n, limit, width, seed):
    """[B, n, 2] masks with firsts in [0, limit) and widths in [0, width], seeded."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, limit, (B, n)), rng.integers(0, width + 1, (B, n))], axis=-1)


def _matrix():
    cs = []
    # the shortest windows: V = 0, 1, 2 (the only warp is (1, 1)), V = 3 with segments of one frame (all four taps clamp to it)
    cs.append(_case("short", 3, 40, [0, 1, 2, 3, 3, 40], warp=[(0, 0), (0, 0), (1, 1), (1, 2), (2, 1), (1, 39)],
                    fm=[[(1, 1)], [(0, 0)], [(2, 5)], [(0, 0)], [(1, 1)], [(0, 0)]], tm=[[(0, 3)], [(0, 1)], [(1, 1)], [(0, 0)], [(2, 1)], [(38, 9)]], fill=0.5))
    # the warp's ends, and a stretch and a squeeze by one frame
    cs.append(_case("ends", 3, 40, [40, 40, 40, 40, 37], warp=[(1, 39), (39, 1), (20, 21), (20, 19), (36, 1)], offset=3))
    # c == w: a copy, with NaN and Inf cells inside that come through as words, alone and beside a mask (the compute path's copy)
    cs.append(_case("copy_words", 3, 70, [70, 70, 66], warp=[(30, 30), (30, 30), (0, 0)], tm=[[(0, 0)], [(5, 3)], [(60, 3)]], fill=-2.0,
                    cells=[(0, 1, 10, NAN_A), (0, 2, 29, INF), (1, 0, 30, NAN_B), (1, 1, 40, INF | 0x80000000), (2, 2, 7, NAN_A), (2, 0, 59, NAN_B)],
                    finite=False))
    # T at the tile, one below and one above; V ending mid-tile
    for T in (TILE - 1, TILE, TILE + 1):
        cs.append(_case("T%d" % T, 3, T, [T, T - 1, 130], warp=[(128, 100), (T - 2, 17), (64, 65)], tm=[[(250, 9)], [(0, 0)], [(129, 4)]],
                        fm=[[(2, 1)], [(0, 0)], [(0, 0)]], offset=1 + 2 * (T % 2)))
    # a warp point on a tile boundary, from either side; V ending mid-tile; tiles that are plain copies beside tiles that are not
    cs.append(_case("warp_on_tile", 2, 600, [600, 515, 300, 600], warp=[(256, 300), (256, 200), (100, 256), (0, 0)],
                    tm=[[(0, 0)], [(510, 20)], [(0, 0)], [(300, 10)]], fill=1.25, offset=3))
    # masks: width 0, overlapping, past V and past rows, every row, every frame
    cs.append(_case("masks", 80, 70, [70, 50, 70, 70, 33], fm=[[(5, 0), (79, 0)], [(10, 20), (25, 20)], [(70, 30), (79, 1 << 31)], [(0, 80), (3, 3)], [(0, 0), (0, 0)]],
                    tm=[[(9, 0), (0, 0)], [(40, 20), (45, 100)], [(0, 0), (69, 5)], [(1, 1), (0, 0)], [(0, 33), (10, 5)]], fill=0.0))
    # F = M = 32 on warped windows, the mean as the fill
    cs.append(_case("masks32", 80, 300, [300, 280], warp=[(100, 140), (270, 200)], fm=_spread(2, 32, 80, 4, 1), tm=_spread(2, 32, 300, 5, 2), offset=3))
    # a NaN under masked cells does not leak: its whole row is masked; beside it the same NaN with no mask leaks where the taps say
    cs.append(_case("nan_masked", 3, 60, [60, 60], warp=[(20, 30), (20, 30)], fm=[[(1, 1)], [(0, 0)]], fill=0.25,
                    cells=[(0, 1, 25, NAN_A), (1, 1, 25, NAN_A)], finite=False))
    # the mean over two 4096-frame chunks at one row, and the mean of a window that is then fully masked
    cs.append(_case("mean_chunks", 1, 4200, [4200, 4097, 100], warp=[(0, 0), (4000, 4090), (0, 0)], tm=[[(4090, 30)], [(0, 7)], [(0, 100)]]))
    cs.append(_case("mean_all_masked", 3, 50, [50, 41, 0], fm=[[(0, 3)], [(0, 0)], [(0, 3)]], tm=[[(0, 0)], [(0, 41)], [(0, 9)]], offset=3))
    # rows 1 and 256 (3 and 80 are above), warped and masked past the rows
    cs.append(_case("rows1", 1, 300, [300, 257, 9], warp=[(200, 100), (3, 250), (4, 5)], fm=[[(0, 0)], [(0, 0)], [(0, 1)]], tm=[[(255, 2)], [(0, 0)], [(0, 0)]]))
    cs.append(_case("rows256", 256, 67, [67, 30], warp=[(30, 40), (0, 0)], fm=[[(250, 27)], [(31, 2)]], tm=[[(60, 3)], [(0, 0)]], offset=3))
    # no warp, no masks: a word copy of everything
    cs.append(_case("identity", 5, 300, [300, 120, 0], fill=3.0, cells=[(0, 2, 3, NAN_A), (1, 4, 119, INF)], finite=False))
    return cs


MATRIX = _matrix()
NAMES = [c["name"] for c in MATRIX]


def case(name):
    return MATRIX[NAMES.index(name)]


def data(c):
    """The case's batch [B, rows, T] float32 (CT), seeded by its name: unit normals with a per-row offset; padding holds PAD_WORD."""
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    x = (rng.standard_normal((B, rows, T)) * rng.uniform(0.5, 3.0, (B, rows, 1)) + rng.uniform(-4, 4, (B, rows, 1))).astype(np.float32)
    for k, n in enumerate(c["valid"]):
        x[k, :, n:].view(np.uint32)[...] = PAD_WORD
    for k, r, t, word in c["cells"]:
        x.view(np.uint32)[k, r, t] = word
    return x


_SIM = {}


def simulated(name, layout):
    """(cells [B, rows, T], fills [B]) of the case under the simulator in `layout`, computed once; the guard bands around the output
    and around the fills are checked here, and so is that the input keeps its words."""
    key = (name, layout)
    if key not in _SIM:
        c = case(name)
        x = data(c)
        B, rows, T = x.shape
        src = as_layout(x, layout)
        before = src.copy()
        flat, body = guarded(x.size, c["offset"])
        fflat, fbody = guarded(B, 1)
        ss.specaug_windows(src, body, c["valid"], layout, c["warp"], c["fm"], c["tm"], c["fill"], fbody, shape=(B, rows, T))
        assert guards_intact(flat, x.size, c["offset"]), (name, "a guard word around the output was written")
        assert guards_intact(fflat, B, 1), (name, "a guard word around the fills was written")
        assert same_words(src, before), (name, "the input was written")
        assert not np.any(body.view(np.uint32) == NAN_FILL), (name, "an output word was not written")
        cells = from_layout(body.reshape((B, T, rows) if layout == ss.TC else (B, rows, T)).copy(), layout)
        _SIM[key] = (cells, fbody.copy())
    return _SIM[key]
