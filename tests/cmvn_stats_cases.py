"""The cases of the CMVN accumulator and the grouped normalisation (clx_cmvn_stats_windows, clx_cmvn_grouped_windows), shared by the
simulator tests and the GPU tests: the edges of the strands (64) and the chunks (4096), of the TC row group (16 / 17 rows), of the
16-byte grid of the in-place apply, and of the group lists.  Every case is small: B <= 6.  Nothing here touches a
GPU."""
import numpy as np

import simlib_cmvn_stats as ss
from norm_cases import GUARD, NAN_FILL, as_layout, from_layout, guarded, guards_intact, same_words  # noqa: F401

PAD_WORD = 0x7fc0beef                    # what the input's padding holds: a NaN that must never be read (one read poisons a sum)
NAN64 = 0x7ff8dead0000beef               # what the accumulator and its guards hold before a reset
LAYOUTS = (ss.CT, ss.TC)


def _case(name, rows, T, valid, groups=None, n_groups=1, offset=1, pad=0.0, norm_vars=1, kind="mixed"):
    assert len(valid) <= 6 and (groups is None or len(groups) == len(valid))
    return dict(name=name, rows=rows, T=T, valid=list(valid), groups=None if groups is None else list(groups), n_groups=n_groups, offset=offset,
                pad=pad, norm_vars=norm_vars, kind=kind)


CASES = [
    # T and valid around the strands and the chunks
    _case("T1", 3, 1, [1, 0, 1]),
    _case("T63", 1, 63, [63, 62, 0, 1], groups=[0, 0, 0, 0], offset=2),
    _case("T64", 17, 64, [64, 63, 1, 0], groups=[0, 1, 2, 3], n_groups=4, offset=3, pad=-1.5),
    _case("T65", 16, 65, [65, 64, 1, 0, 65], norm_vars=0),
    _case("T4095", 3, 4095, [4095, 4094, 1], groups=[0, 1, 2], n_groups=3, offset=2),
    _case("T4096", 1, 4096, [4096, 4095, 0], offset=3),
    # unsorted ids; group 1 has one window without a live frame, group 3 has no window, one window takes no part
    _case("T4097", 13, 4097, [4097, 4096, 1, 4097, 4097, 0], groups=[2, 0, 2, -1, 0, 1], n_groups=4, pad=7.25),
    _case("T8193", 2, 8193, [8193, 8192, 4097], groups=[1, 1, 0], n_groups=2, offset=2),
    _case("unsorted", 5, 131, [131, 130, 1, 131, 64, 0], groups=[2, 0, 2, -1, 0, 1], n_groups=4, offset=3, norm_vars=0),
    # the rows: 80 bands, 560 stacked rows, the limit
    _case("rows80", 80, 70, [70, 69, 0, 1], groups=[1, 0, 1, 0], n_groups=2, offset=2),
    _case("rows560", 560, 37, [37, 12, 36], offset=1),
    _case("rows8192", 8192, 65, [65], groups=[1], n_groups=2, offset=3),
    _case("many_groups", 2, 67, [67, 66], groups=[65535, 0], n_groups=65536, offset=1),
    # a NaN and an Inf in window 0 alone: group 0 is affected, group 1 is not, group 2 has no window
    _case("nonfinite", 2, 130, [130, 130, 100], groups=[0, 1, 1], n_groups=3, kind="nonfinite"),
]
NAMES = [c["name"] for c in CASES]
FINITE = [n for n in NAMES if n != "nonfinite"]
# the cases the GPU runs, both layouts of each
GPU = ["T1", "T64", "T65", "T4096", "T4097", "T8193", "unsorted", "rows80", "rows560", "rows8192", "many_groups", "nonfinite"]


def case(name):
    return CASES[NAMES.index(name)]


def _rng(name, salt=0):
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) + 7919 * salt)


def data(c, salt=0):
    """The case's batch [B, rows, T] float32 (CT), seeded by its name (and `salt`: a later call's batch): cells of either sign and of
    magnitudes 1e-3 .. 1e4, so that the order of the additions is in the words; padding holds PAD_WORD."""
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    rng = _rng(c["name"], salt)
    x = (rng.choice([-1.0, 1.0], (B, rows, T)) * 10.0 ** rng.uniform(-3, 4, (B, rows, T))).astype(np.float32)
    if c["kind"] == "nonfinite" and salt == 0:
        x.view(np.uint32)[0, 0, 40] = 0x7f800000
        x.view(np.uint32)[0, 1, 99] = 0x7fc00123
    for k, n in enumerate(c["valid"]):
        x[k, :, n:].view(np.uint32)[...] = PAD_WORD
    return x


def guarded64(words):
    """(the whole float64 buffer, the `words` doubles of it a call may write), every word NAN64, GUARD words on either side."""
    flat = np.full(words + 2 * GUARD, NAN64, dtype=np.uint64).view(np.float64)
    return flat, flat[GUARD:GUARD + words]


def guards_intact64(flat, words):
    h = flat.view(np.uint64)
    return bool(np.all(h[:GUARD] == NAN64) and np.all(h[GUARD + words:] == NAN64))


def same_words64(a, b):
    return a.shape == b.shape and bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def stats_shape(c):
    return (c["n_groups"], 2, c["rows"] + 1)


_STATS, _CELLS, _REST = {}, {}, {}


def simulated_stats(name, layout, calls=1):
    """The accumulator [G, 2, rows + 1] of the case under the simulator in `layout` after a reset call over data(c) and calls - 1
    accumulating calls over data(c, 1), data(c, 2), ..; computed once.  The accumulator starts as NAN64 words inside guard words."""
    key = (name, layout, calls)
    if key not in _STATS:
        c = case(name)
        words = int(np.prod(stats_shape(c)))
        flat, body = guarded64(words)
        for i in range(calls):
            x = data(c, i)
            ss.stats_windows(as_layout(x, layout), c["valid"], layout, c["groups"], c["n_groups"], body, accumulate=i > 0, shape=x.shape)
        assert guards_intact64(flat, words), (name, "a guard word around the accumulator was written")
        assert not np.any(body.view(np.uint64) == NAN64), (name, "a word of the accumulator was not written by the reset")
        _STATS[key] = body.reshape(stats_shape(c)).copy()
    return _STATS[key]


def restated_stats(name, calls=1):
    key = (name, calls)
    if key not in _REST:
        c = case(name)
        acc = None
        for i in range(calls):
            acc = ss.restate_stats(data(c, i), c["valid"], c["groups"], c["n_groups"], acc, accumulate=i > 0)
        _REST[key] = acc
    return _REST[key]


def simulated_grouped(name, layout):
    """(cells [B, rows, T], shift_scale [G, 2, rows]) of the case's batch normalised in place under the simulator in `layout` by the
    accumulator simulated_stats(name, CT) leaves, inside guard words; computed once."""
    key = (name, layout)
    if key not in _CELLS:
        c = case(name)
        x = data(c)
        B, rows, T = x.shape
        st = simulated_stats(name, ss.CT)
        before = st.copy()
        flat, body = guarded(B * rows * T, c["offset"])
        body[...] = as_layout(x, layout).reshape(-1)
        sflat, sbody = guarded(c["n_groups"] * 2 * rows, 1)
        ss.grouped_windows(body, c["valid"], layout, c["groups"], c["n_groups"], st, sbody, c["norm_vars"], c["pad"], shape=x.shape)
        assert guards_intact(flat, B * rows * T, c["offset"]), (name, "a guard word around the batch was written")
        assert guards_intact(sflat, c["n_groups"] * 2 * rows, 1), (name, "a guard word around shift_scale was written")
        assert same_words64(st, before), (name, "the accumulator was written")
        cells = from_layout(body.reshape((B, T, rows) if layout == ss.TC else (B, rows, T)).copy(), layout)
        _CELLS[key] = (cells, sbody.reshape(c["n_groups"], 2, rows).copy())
    return _CELLS[key]
