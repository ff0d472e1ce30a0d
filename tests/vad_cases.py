"""The cases of the energy VAD and the frame selection (clx_vad_windows, clx_select_windows), shared by the simulator tests and the
GPU tests: the edge matrix of the live length, the context, the proportion, the tiles of 256 frames and the waves of 64 inside
them.  Every case is small: B <= 10, three tiles of 256 frames at the most.  Nothing here touches a GPU."""
import numpy as np

import simlib_vad as sv
from norm_cases import GUARD, NAN_FILL, as_layout, from_layout, guarded, guards_intact, same_words  # noqa: F401

TILE = sv.TILE
T3 = 2 * TILE + 37                       # two whole tiles and a ragged one
PAD_WORD = 0x7fc0beef                    # what the padding and the rows that are not the energy row hold: never read by the decision
BYTE_FILL, BYTE_GUARD = 0xa5, 64         # what a mask buffer and the guard bytes around it hold before a call
CONTEXTS = (0, 1, 2, 5, 128)
PROPORTIONS = (0.12, 0.5, 0.6, 0.999)    # 0.5: num == den * p ties at the edges, where den is even
SCALES = (0.0, 0.5)
ROWS = (1, 3, 13, 30, 80)
KINDS = ("normal", "all", "none", "alternating", "runs")
RUNS = ((60, 68), (250, 262), (505, 520), (63, 64), (255, 257), (511, 513), (300, 301))   # across the waves' and the tiles' edges


def valids(c, T):
    """V in 0, 1, 2, c, c + 1, 2c + 1, 255, 256, 257 and T (clipped to 0..T, each once)."""
    out = []
    for v in (T, 0, 1, 2, c, c + 1, 2 * c + 1, 255, 256, 257):
        v = min(max(int(v), 0), T)
        if v not in out:
            out.append(v)
    return out


def _vad(name, rows, T, valid, E, s, c, p, row, kind="normal", offset=0):
    return dict(name=name, rows=rows, T=T, valid=list(valid), E=E, s=s, c=c, p=p, row=row, kind=kind, offset=offset)


def _vad_matrix():
    cs = []
    i = 0
    for c in CONTEXTS:
        for p in PROPORTIONS:
            for s in SCALES:
                rows = ROWS[i % len(ROWS)]
                cs.append(_vad("c%d_p%s_s%s" % (c, p, s), rows, T3, valids(c, T3), (5.0, 5.5)[i % 2], s, c, p, (0, rows - 1)[(i // 2) % 2],
                               kind=KINDS[i % len(KINDS)], offset=i % 4))
                i += 1
    # the recipes' options and Kaldi's defaults over 30 MFCC rows
    cs.append(_vad("voxceleb", 30, T3, valids(2, T3), 5.5, 0.5, 2, 0.12, 0))
    cs.append(_vad("kaldi_default", 30, T3, valids(0, T3), 5.0, 0.5, 0, 0.6, 0, offset=1))
    # the 560 stacked rows of the low-frame-rate front end, first and last row
    cs.append(_vad("rows560", 560, 70, [70, 33, 0, 1], 5.0, 0.5, 2, 0.5, 0, offset=2))
    cs.append(_vad("rows560_last", 560, 70, [70, 69, 11], 5.5, 0.5, 5, 0.12, 559, offset=3))
    # cells planted exactly at the threshold: not above.  s == 0: thr = E; s != 0: whole numbers whose mean is 6, thr = 5 + 3 = 8
    cs.append(_vad("planted", 3, T3, valids(2, T3), 5.5, 0.0, 2, 0.5, 1, kind="planted"))
    cs.append(_vad("planted_s", 3, T3, valids(1, T3), 5.0, 0.5, 1, 0.6, 2, kind="planted_s", offset=1))
    # a NaN and both infinities in the energy row (s == 0: the threshold stays a number; s != 0: IEEE in the sum)
    cs.append(_vad("nonfinite", 2, 300, [300, 200, 257], 5.0, 0.0, 2, 0.5, 0, kind="nonfinite"))
    cs.append(_vad("nonfinite_s", 2, 300, [300, 200, 257], 5.0, 0.5, 1, 0.6, 1, kind="nonfinite"))
    # neighbouring pairs (+2^50, -2^50) in the energy row: the order of the sum moves thr by many ulps
    cs.append(_vad("wide_c0", 3, T3, [T3, 257, 100, 33], 5.0, 0.5, 0, 0.6, 1, kind="wide", offset=1))
    cs.append(_vad("wide_c5", 1, T3, [T3, 300, 129, 64], 5.5, 0.5, 5, 0.12, 0, kind="wide", offset=2))
    return cs


VAD = _vad_matrix()
VAD_NAMES = [c["name"] for c in VAD]
ORDINARY_NAMES = [c["name"] for c in VAD if c["kind"] in KINDS]            # finite, no planted cells, no wide pairs
FINITE_NAMES = [c["name"] for c in VAD if c["kind"] != "nonfinite"]
WIDE_NAMES = [c["name"] for c in VAD if c["kind"] == "wide"]
# the cases the GPU runs, both layouts of each: every context, every proportion, both scales, every row count, both planted kinds,
# the cells that are not finite and the wide sums
GPU_VAD = ["c0_p0.12_s0.0", "c0_p0.5_s0.5", "c1_p0.6_s0.5", "c2_p0.999_s0.0", "c2_p0.12_s0.5", "c5_p0.5_s0.5", "c5_p0.6_s0.0", "c128_p0.12_s0.5",
           "c128_p0.5_s0.0", "c128_p0.999_s0.5", "voxceleb", "kaldi_default", "rows560", "rows560_last", "planted", "planted_s", "nonfinite",
           "wide_c0", "wide_c5"]


def vad_case(name):
    return VAD[VAD_NAMES.index(name)]


def _rng(name):
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def vad_data(c):
    """The case's batch [B, rows, T] float32 (CT), seeded by its name.  The energy row: float32 N(5, 2^2) cells (`normal`), or cells
    around 20 (`all`: above any threshold here), around 0 (`none`), the two in turn (`alternating`) or runs of the first among the
    second that straddle the waves' and the tiles' edges (`runs`).  Every other row and the padding hold PAD_WORD."""
    B, rows, T, kind = len(c["valid"]), c["rows"], c["T"], c["kind"]
    rng = _rng(c["name"])
    e = (rng.standard_normal((B, T)) * 2.0 + 5.0).astype(np.float32)
    noise = rng.uniform(-1, 1, (B, T)).astype(np.float32)
    t = np.arange(T)
    if kind == "all":
        e = 20 + noise
    elif kind == "none":
        e = noise
    elif kind == "alternating":
        e = np.where(t % 2 == 0, 20 + noise, noise)
    elif kind == "runs":
        on = np.zeros(T, dtype=bool)
        for a, b in RUNS:
            on[a:b] = True
        e = np.where(on, 20 + noise, noise)
    elif kind == "planted":
        e[:, ::3] = np.float32(c["E"])                       # equal to thr: not above
        e[:, 1::7] = np.nextafter(np.float32(c["E"]), np.float32(np.inf))      # one ulp over: above
    elif kind == "planted_s":
        # 6 everywhere, then pairs (8, 4) and (10, 2) inside every live length (the pairs start at even frames below V - 1):
        # every sum is exact, the mean is 6, thr = E + 0.5 * 6 = 8 exactly, the 8s are not above and the 10s are
        e = np.full((B, T), 6.0, dtype=np.float32)
        for k, V in enumerate(c["valid"]):
            for a in range(0, V - 1, 2):
                hi, lo = ((8.0, 4.0), (10.0, 2.0), (6.0, 6.0))[(a // 2 + k) % 3]
                e[k, a], e[k, a + 1] = hi, lo
    elif kind == "wide":
        for k in range(B):
            at = 3 * rng.permutation((T - 2) // 3)[:T // 6] + 1
            v = (rng.uniform(0.5, 1.0, at.size) * 2.0 ** 50).astype(np.float32)
            e[k, at], e[k, at + 1] = v, -v
        for k, V in enumerate(c["valid"]):                   # (a pair cut by the live length would leave 2^50 in the mean)
            if V and V < T and e[k, V - 1] > 2.0 ** 40:
                e[k, V - 1] = 5.0
    elif kind == "nonfinite":
        for k, at, word in ((0, 40, 0x7f800000), (0, 150, 0x7fc00123), (1, 199, 0xff800000), (1, 0, 0x7fc00001), (2, 255, 0x7f800000), (2, 256, 0xff800000)):
            e.view(np.uint32)[k, at] = word
    x = np.zeros((B, rows, T), dtype=np.float32)
    x.view(np.uint32)[...] = PAD_WORD
    x[:, c["row"], :] = e.astype(np.float32)
    for k, n in enumerate(c["valid"]):
        x[k, :, n:].view(np.uint32)[...] = PAD_WORD
    return x


def guarded_bytes(n):
    """(the whole buffer, the n bytes of it a call may write): BYTE_GUARD bytes of BYTE_FILL on both sides."""
    raw = np.full(n + 2 * BYTE_GUARD, BYTE_FILL, dtype=np.uint8)
    return raw, raw[BYTE_GUARD:BYTE_GUARD + n]


def byte_guards_intact(raw, n):
    return bool(np.all(raw[:BYTE_GUARD] == BYTE_FILL) and np.all(raw[BYTE_GUARD + n:] == BYTE_FILL))


_SIM, _REST, _REF = {}, {}, {}


def simulated_vad(name, layout):
    """(mask uint8 [B, T], thresholds float32 [B]) of the case under the simulator in `layout`, computed once; the guards around both
    outputs are checked here, and so is that the input keeps its words and that every output byte and word was written."""
    key = (name, layout)
    if key not in _SIM:
        c = vad_case(name)
        x = vad_data(c)
        B, rows, T = x.shape
        src = as_layout(x, layout)
        before = src.copy()
        raw, mask = guarded_bytes(B * T)
        flat, thr = guarded(B, c["offset"])
        sv.vad_windows(src, c["valid"], layout, c["E"], c["s"], c["c"], c["p"], c["row"], mask=mask, thresholds=thr, shape=x.shape)
        assert byte_guards_intact(raw, B * T), (name, "a guard byte around the mask was written")
        assert guards_intact(flat, B, c["offset"]), (name, "a guard word around the thresholds was written")
        assert same_words(src, before), (name, "the input was written")
        assert np.all(mask <= 1), (name, "a mask byte was not written, or is neither 0 nor 1")
        assert not np.any(thr.view(np.uint32) == NAN_FILL), (name, "a threshold was not written")
        _SIM[key] = (mask.reshape(B, T).copy(), thr.copy())
    return _SIM[key]


def restated_vad(name):
    """simlib_vad.restate_vad of the case, computed once."""
    if name not in _REST:
        c = vad_case(name)
        _REST[name] = sv.restate_vad(vad_data(c), c["valid"], c["E"], c["s"], c["c"], c["p"], c["row"])
    return _REST[name]


def reference_vad(name):
    """simlib_vad.reference_vad of the case, computed once."""
    if name not in _REF:
        c = vad_case(name)
        _REF[name] = sv.reference_vad(vad_data(c), c["valid"], c["E"], c["s"], c["c"], c["p"], c["row"])
    return _REF[name]


# ---- the selection ------------------------------------------------------------------------------------------------------------------

MASKS = ("ones", "zeros", "first", "last_live", "second", "bytes", "random")


def _select(name, rows, T, valid, mask, pad=0.0, offset=0):
    return dict(name=name, rows=rows, T=T, valid=list(valid), mask=mask, pad=pad, offset=offset)


def _select_matrix():
    cs = []
    for i, m in enumerate(MASKS):
        rows = ROWS[i % len(ROWS)]
        cs.append(_select("%s_rows%d" % (m, rows), rows, T3, valids((0, 5, 128)[i % 3], T3), m, pad=(0.0, -1.5)[i % 2], offset=i % 4))
    cs.append(_select("random_rows30", 30, T3, valids(2, T3), "random", offset=1))
    cs.append(_select("random_rows80", 80, T3, [T3, 300, 257, 0], "random", pad=7.25, offset=3))
    cs.append(_select("second_rows560", 560, 70, [70, 33, 0, 1], "second", offset=2))
    cs.append(_select("padding_counts_nothing", 3, T3, [100, 0, 256, 511], "ones", pad=-1.5, offset=1))
    return cs


SELECT = _select_matrix()
SELECT_NAMES = [c["name"] for c in SELECT]
GPU_SELECT = SELECT_NAMES                 # all of them: eleven small cases, both layouts


def select_case(name):
    return SELECT[SELECT_NAMES.index(name)]


def select_data(c):
    """(x [B, rows, T] float32, mask uint8 [B, T]) of the case.  The cells are any words -- numbers, NaNs with payloads, -0.0 -- and
    PAD_WORD from V on; the mask's bytes from V on are 0xff (they must not count)."""
    B, rows, T, kind = len(c["valid"]), c["rows"], c["T"], c["mask"]
    rng = _rng(c["name"])
    x = rng.standard_normal((B, rows, T)).astype(np.float32)
    w = x.view(np.uint32)
    odd = rng.random((B, rows, T)) < 0.02
    w[odd] = rng.choice(np.array([0x7fc01234, 0xffc00001, 0x7f800001, 0x80000000, 0x7f800000], dtype=np.uint32), int(odd.sum()))
    mask = np.zeros((B, T), dtype=np.uint8)
    for k, V in enumerate(c["valid"]):
        if kind == "ones":
            mask[k, :V] = 1
        elif kind == "first" and V:
            mask[k, 0] = 1
        elif kind == "last_live" and V:
            mask[k, V - 1] = 1
        elif kind == "second":
            mask[k, k % 2:V:2] = 1
        elif kind == "bytes":
            mask[k, :V] = rng.choice(np.array([0, 0, 2, 128, 255, 1], dtype=np.uint8), V)
        elif kind == "random":
            mask[k, :V] = rng.random(V) < (0.1, 0.5, 0.9)[k % 3]
        mask[k, V:] = 0xff
        w[k, :, V:] = PAD_WORD
    return x, mask


_SSIM, _SREST = {}, {}


def simulated_select(name, layout):
    """(cells [B, rows, T], counts uint32 [B]) of the case under the simulator in `layout`, computed once; the guard words around the
    output are checked here, and so is that the source and the mask keep their words and that every output word was written."""
    key = (name, layout)
    if key not in _SSIM:
        c = select_case(name)
        x, mask = select_data(c)
        B, rows, T = x.shape
        src = as_layout(x, layout)
        before, mask_before = src.copy(), mask.copy()
        flat, body = guarded(B * rows * T, c["offset"])
        _, counts = sv.select_windows(src, body, c["valid"], mask, layout, c["pad"], shape=x.shape)
        assert guards_intact(flat, B * rows * T, c["offset"]), (name, "a guard word around the output was written")
        assert same_words(src, before) and np.array_equal(mask, mask_before), (name, "an input was written")
        assert not np.any(body.view(np.uint32) == NAN_FILL), (name, "an output word was not written")
        _SSIM[key] = (from_layout(body.reshape((B, T, rows) if layout == sv.TC else (B, rows, T)).copy(), layout), counts)
    return _SSIM[key]


def restated_select(name):
    """simlib_vad.restate_select of the case, computed once."""
    if name not in _SREST:
        c = select_case(name)
        x, mask = select_data(c)
        _SREST[name] = sv.restate_select(x, c["valid"], mask, c["pad"])
    return _SREST[name]
