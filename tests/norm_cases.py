"""The cases of the per-window normalisation (clx_norm_windows), shared by the simulator tests and the GPU tests: the edge matrix
of the sums' order and the tiling, and the outside cases recorded by tools/make_norm_goldens.py (tests/golden/features/norm_*.npz)
with their intervals.  Nothing here touches a GPU."""
import math
import os

import numpy as np

import simlib_norm as sn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features")
CHUNK, STRANDS = sn.CHUNK, sn.STRANDS
NAN_FILL = 0x7fc0dead
GUARD = 64

ALL = sn.opts()
OPTS = {                                  # the four legal combinations of mean, var and ddof-with-var, eps 0 and 1e-7, pad 0 and -1
    "mv": sn.opts(1, 1, 0, 0.0, 0.0),
    "m": sn.opts(1, 0, 0, 0.0, -1.0),
    "v": sn.opts(0, 1, 0, 1e-7, 0.0),
    "mv1": sn.opts(1, 1, 1, 1e-7, -1.0),
}


def _valids(T):
    """0, 1, 2, T - 1, T and one in between, for six windows (clipped to 0..T)."""
    return [min(max(v, 0), T) for v in (T, 0, 1, 2, T - 1, T // 2 + 1)]


def _case(name, rows, T, valid, opt, offset=0, stats=True, kind="normal"):
    return dict(name=name, rows=rows, T=T, valid=list(valid), o=OPTS[opt] if isinstance(opt, str) else opt, offset=offset, stats=stats, kind=kind)


def _matrix():
    cs = []
    # T across the chunk and the strands, one row and a few, every option combination in turn
    keys = list(OPTS)
    for i, T in enumerate((1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 3 * STRANDS - 1, 3 * STRANDS + 1)):
        cs.append(_case("T%d_rows1" % T, 1, T, _valids(T), keys[i % 4], offset=i % 4))
        cs.append(_case("T%d_rows3" % T, 3, T, _valids(T)[:4] if T > CHUNK else _valids(T), keys[(i + 1) % 4], offset=(i + 2) % 4, stats=bool(i % 2)))
    # rows up to the limit, at a T that is no multiple of 4 (rows share vectors) and more than one apply tile
    for i, rows in enumerate((2, 8, 23, 80, sn.MAX_ROWS)):
        T = 3 * STRANDS + 1 if rows < 80 else 67
        cs.append(_case("rows%d" % rows, rows, T, _valids(T)[:3 if rows >= 80 else 6], keys[i % 4], offset=(i + 1) % 4))
    # every option combination on one shape, with and without stats, at every offset within 16 bytes
    for i, k in enumerate(keys):
        cs.append(_case("opts_%s" % k, 3, 131, _valids(131), k, offset=i, stats=True))
        cs.append(_case("opts_%s_nostats" % k, 3, 131, _valids(131), k, offset=(i + 1) % 4, stats=False))
    cs.append(_case("constant_row", 2, 70, [70, 70, 33], "mv", kind="constant"))
    cs.append(_case("one_live_ddof1", 2, 9, [1, 1, 9], sn.opts(1, 1, 1, 0.0, 0.0)))
    return cs


MATRIX = _matrix()
NAMES = [c["name"] for c in MATRIX]


def case(name):
    return MATRIX[NAMES.index(name)]


def data(c):
    """The case's batch [B, rows, T] float32 (CT), seeded by its name; padding cells hold values that must not reach a sum."""
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    x = (rng.standard_normal((B, rows, T)) * rng.uniform(0.1, 4.0, (B, rows, 1)) + rng.uniform(-3, 3, (B, rows, 1))).astype(np.float32)
    if c["kind"] == "constant":
        x[0, 0, :] = np.float32(1.25)                        # d = 0 throughout: 0 / 0 with eps = 0
        x[1, 1, :] = np.float32(0.0)
    for k, n in enumerate(c["valid"]):
        x[k, :, n:] = np.float32(1e30)                       # (what a sum must not see)
    return x


def as_layout(x, layout):
    """[B, rows, T] as the layout's own contiguous array."""
    return np.ascontiguousarray(x.transpose(0, 2, 1)).copy() if layout == sn.TC else x.copy()


def from_layout(a, layout):
    return np.ascontiguousarray(a.transpose(0, 2, 1)) if layout == sn.TC else a


def guarded(words, offset):
    """(the whole buffer, the `words` floats of it a call may write): GUARD + offset words of NAN_FILL in front, GUARD behind; the
    slice starts `offset` floats behind a 16-byte boundary."""
    raw = np.full(words + 2 * GUARD + offset + 4, NAN_FILL, dtype=np.uint32)
    skew = (-(raw.ctypes.data // 4)) % 4                     # floats up to the next 16-byte boundary
    flat = raw[skew:skew + words + 2 * GUARD + offset].view(np.float32)
    assert flat.ctypes.data % 16 == 0
    return flat, flat[GUARD + offset:GUARD + offset + words]


def guards_intact(flat, words, offset):
    h = flat.view(np.uint32)
    at = GUARD + offset
    return bool(np.all(h[:at] == NAN_FILL) and np.all(h[at + words:] == NAN_FILL))


_SIM = {}


def simulated(name, layout):
    """(cells [B, rows, T], stats [B, rows, 2] or None) of the case under the simulator in `layout`, computed once; the guard bands
    around the batch and around stats are checked here."""
    key = (name, layout)
    if key not in _SIM:
        c = case(name)
        x = data(c)
        B, rows, T = x.shape
        flat, body = guarded(x.size, c["offset"])
        body[:] = as_layout(x, layout).reshape(-1)
        sflat, sbody = guarded(B * rows * 2, 1)
        sn.norm_windows(body, c["valid"], layout, c["o"], sbody if c["stats"] else None, shape=(B, rows, T))
        assert guards_intact(flat, x.size, c["offset"]), (name, "a guard word around the batch was written")
        if c["stats"]:
            assert guards_intact(sflat, B * rows * 2, 1), (name, "a guard word around stats was written")
        else:
            assert np.all(sflat.view(np.uint32) == NAN_FILL), (name, "stats was written though it was not given")
        cells = from_layout(body.reshape((B, T, rows) if layout == sn.TC else (B, rows, T)).copy(), layout)
        _SIM[key] = (cells, sbody.reshape(B, rows, 2).copy() if c["stats"] else None)
    return _SIM[key]


def same_words(a, b):
    return a.shape == b.shape and bool(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)))


# ---- the outside cases ------------------------------------------------------------------------------------------------------------

def pairwise_rel(n):
    """The relative error bound of numpy's float32 sum of n contiguous terms: blocks of at most 128 terms in 8 accumulators (16 additions
    each, 3 to combine them), then a binary tree over the blocks."""
    return min(n, 19 + max(0, math.ceil(math.log2(max(n / 128.0, 1.0))))) * sn.U32


class Outside:
    """One recorded outside answer: x [1, rows, T] (the outside's own input, float64), x32 (what this library is given), valid, the
    Norm options, `want` [1, rows, T] (the outside's answer) and `allow` [1, rows, T]: the interval's half width around `want` --
    this library's bound around the float64 reference plus the outside's own."""

    def __init__(self, name, x, valid, o, want, outside_bound, dx=None):
        self.name, self.o, self.valid = name, o, [int(valid)]
        self.x = np.asarray(x, dtype=np.float64)[None]
        self.x32 = self.x.astype(np.float32)
        self.want = np.asarray(want, dtype=np.float64)[None]
        if dx is None:                                       # (how far this library's input lies from the outside's: one rounding)
            dx = np.abs(self.x32.astype(np.float64) - self.x)
        self.ours = sn.bound(self.x, self.valid, o, dx=dx)
        self.allow = self.ours + outside_bound(self.x, self.valid, o)
        self.rows, self.T = self.x.shape[1], self.x.shape[2]

    def check(self, got, what):
        """got [1, rows, T]: every live cell inside the interval, every padding cell exactly pad (the widths are printed)."""
        n = self.valid[0]
        got = np.asarray(got, dtype=np.float64)
        err = np.abs(got - self.want)
        print("%s %s: worst error %.3g, worst error / allowance %.3g, widest allowance %.3g" % (
            self.name, what, err[..., :n].max(), (err[..., :n] / self.allow[..., :n]).max(), self.allow[..., :n].max()))
        assert np.all(got[..., n:] == np.float32(self.o["pad"])), (self.name, what, "padding")
        assert np.all(err[..., :n] <= self.allow[..., :n]), (self.name, what, float((err[..., :n] / self.allow[..., :n]).max()))


_OUT = {}
OUTSIDE = ("wav2vec2", "cmvn_means", "cmvn_vars", "cmvn_both", "seamless")


def outside(name):
    if name in _OUT:
        return _OUT[name]
    if name == "wav2vec2":
        d = np.load(os.path.join(GOLDEN, "norm_wav2vec2.npz"))
        n = int(d["valid"])
        # the outside works in float32 on the contiguous signal: numpy's pairwise sums, rounded squares
        c = Outside(name, d["input"][None, :], n, sn.opts(1, 1, 0, 1e-7, 0.0), d["output"][None, :],
                    lambda x, v, o: sn.bound(x, v, o, sum_rel=pairwise_rel(n), sq_rounded=True))
        c.pcm = d["pcm"]
    elif name.startswith("cmvn_"):
        d = np.load(os.path.join(GOLDEN, "norm_cmvn.npz"))
        which = name[5:]
        o = sn.opts(int(which != "vars"), int(which != "means"), 0, 0.0, 0.0)
        n = int(d["valid"])
        # the outside works in float64 (sums of n terms along the frames) and rounds its answer to float32 once
        c = Outside(name, d["input"].T, n, o, d["output_" + which].T,
                    lambda x, v, o: sn.bound(x, v, o, sum_rel=n * sn.U64, u=sn.U64, sq_rounded=True) + sn.U32 * np.abs(sn.reference(x, v, o)[0]) + 2.0 ** -149)
    elif name == "seamless":
        d = np.load(os.path.join(GOLDEN, "norm_seamless.npz"))
        n = int(d["valid"])
        # the outside works in float32 and adds the frames one after the other (a reduction along the first axis of [T, 80])
        c = Outside(name, d["input"].T, n, sn.opts(1, 1, 1, 1e-7, 0.0), d["output"].T,
                    lambda x, v, o: sn.bound(x, v, o, sum_rel=n * sn.U32, sq_rounded=True))
    else:
        raise KeyError(name)
    _OUT[name] = c
    return c


CMVN_SAMPLES = 400 + 40 * 160            # the first samples of kaldi16's stream that hold exactly 41 whole frames: norm_cmvn's input_length


def outside_via_fbank(name):
    """A cmvn_* case for the whole path from FLAC bytes: the input is then not the outside fbank rounded once but this library's own
    fbank of kaldi16's first CMVN_SAMPLES samples, which outside_cases.intervals holds to the outside fbank cell
    by cell; that distance takes the place of the rounding in the interval (dx of simlib_norm.bound)."""
    key = "fbank_" + name
    if key not in _OUT:
        import outside_cases as oc
        c = oc.case("kaldi16")
        frames, O, lo, hi, cap = oc.intervals(c, 0)
        d = np.load(os.path.join(GOLDEN, "norm_cmvn.npz"))
        assert np.array_equal(O, d["input"]) and list(frames) == list(range(O.shape[0]))
        which = name[5:]
        n = int(d["valid"])
        o = sn.opts(int(which != "vars"), int(which != "means"), 0, 0.0, 0.0)
        _OUT[key] = Outside(key, O.T, n, o, d["output_" + which].T,
                            lambda x, v, o: sn.bound(x, v, o, sum_rel=n * sn.U64, u=sn.U64, sq_rounded=True) + sn.U32 * np.abs(sn.reference(x, v, o)[0]) + 2.0 ** -149,
                            dx=np.maximum(O - lo, hi - O).T[None])
        _OUT[key].stream = c.streams[0][:CMVN_SAMPLES]
    return _OUT[key]
