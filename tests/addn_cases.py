"""The cases of the several-noise mixer (clx_addn_windows), shared by the simulator tests and the GPU tests: the edge matrix of the
sums' order, the covers, the periods, the offsets and the tiling.  Nothing here touches a GPU.

A case: rows, T, valid [B], noise_valid (a list per noise batch), terms (a list per window of (batch, index, offset, loop, snr_db)),
offset (the data's word offset within 16 bytes), noise_offsets (one per batch) and kind."""
import numpy as np

import simlib_addn as sd
from add_cases import PAD_WORD
from norm_cases import as_layout, from_layout, guarded, guards_intact, same_words

CHUNK, STRANDS = sd.CHUNK, sd.STRANDS
INF = float("inf")
PERIODS = (1, 3, 63, 64, 65, 4096, 4097)


def _case(name, rows, T, valid, noise_valid, terms, offset=0, noise_offsets=None, kind="normal"):
    assert len(valid) == len(terms) and all(len(w) <= sd.MAX_TERMS for w in terms)
    assert all(j < 0 or (0 <= b < len(noise_valid) and j < len(noise_valid[b])) for w in terms for b, j, _, _, _ in w)
    return dict(name=name, rows=rows, T=T, valid=list(valid), noise_valid=[list(v) for v in noise_valid], terms=[list(w) for w in terms],
                offset=offset, noise_offsets=list(noise_offsets or [0] * len(noise_valid)), kind=kind)


def _shape(name, rows, T, offset, noise_offsets):
    """Seven windows over two noise batches.  Batch 0: the periods 1, 3, 63, 64, 65, 4096, 4097 (clipped to T), then T, T // 2 and 0
    live samples.  Batch 1: T and min(T, 5).  Windows: Vs = T with a looped and an unlooped term that overlap; Vs = 0; Vs = 1
    with P > Vs, looped; Vs = T with 16 terms (noise windows of both batches, looped and not, at the offsets 0, 1, 3, 4095, 4096,
    Vs - 1, Vs and above, among them an index of -1, +inf and a noise without live samples between live terms); no term; Vs = T - 1 with two terms on one
    noise window at different offsets and a disjoint third; Vs in between with the offsets again, unlooped.  (The periods as loops
    that go round more than once are _loops' cases.)"""
    nv0 = [min(p, T) for p in PERIODS] + [T, T // 2, 0]
    nv1 = [T, min(T, 5)]
    full, half, none = 7, 8, 9
    offs = [0, 1, 3, CHUNK - 1, CHUNK, T - 1, T, T + 5]
    many = []
    for i in range(16):
        if i == 5:
            many.append((0, -1, 0, 0, 0.0))
        elif i == 9:
            many.append((0, 2, 1, 1, INF))
        elif i == 12:
            many.append((0, none, 0, 1, 3.0))
        else:
            many.append((i % 2 if i % 7 else 1, (i % 7) if i % 2 == 0 else i % 2, offs[i % 8], int(i % 3 != 0), float(3 * (i % 5) - 4)))
    v5, v6 = max(T - 1, 0), T // 2 + 1
    valid = [T, 0, min(1, T), T, T // 2 + 1, v5, min(v6, T)]
    terms = [
        [(0, 1, 0, 1, 0.0), (0, full, 0, 0, 5.0)],
        [(0, full, 0, 1, 3.0)],
        [(0, full, 0, 1, -3.0)],
        many,
        [],
        [(1, 1, 1, 1, 6.0), (1, 1, 3, 0, -2.0), (0, half, max(v5 - 1, 0), 0, 10.5)],
        [(0, 4, o, 0, 2.0 + i) for i, o in enumerate([0, 1, 3, CHUNK - 1, CHUNK, max(v6 - 1, 0), v6, v6 + 9])],
    ]
    return _case(name, rows, T, valid, [nv0, nv1], terms, offset, noise_offsets)


def _loops(name, rows, T, offset, noise_offset):
    """The periods as loops that go round at least twice: one noise window per period 1, 3, 63, 64, 65, 4096, 4097.  Window 0 (Vs = T)
    loops every one of them from offset 0, window 1 from offset 3 (off the 16-byte grid), window 2 (Vs = T - 1) loops 1, 4096 and
    4097 from the offsets 1, 4095 and 4096: the sum pass starts lanes at (c * 4096 + l) mod P in every chunk, a wrap falls inside
    a later chunk, the step 64 mod P is 0 (P = 1, 64) and the apply pass meets wrap points inside vectors."""
    assert T >= 3 * max(PERIODS) + 3
    every = list(range(len(PERIODS)))
    big = [PERIODS.index(p) for p in (1, 4096, 4097)]
    terms = [[(0, j, 0, 1, float(j) - 2.0) for j in every], [(0, j, 3, 1, 1.5 * j) for j in every],
             [(0, j, o, 1, 4.0 + i) for i, (j, o) in enumerate((j, o) for j in big for o in (1, CHUNK - 1, CHUNK))]]
    return _case(name, rows, T, [T, T, T - 1], [list(PERIODS)], terms, offset, (noise_offset,))


def _matrix():
    cs = []
    shapes = ((1, 1), (1, 3), (63, 2), (63, 8), (64, 8), (64, 1), (65, 3), (65, 2), (CHUNK - 1, 2), (CHUNK, 3), (CHUNK, 1), (CHUNK + 1, 1),
              (CHUNK + 1, 2), (2 * CHUNK + 3, 3), (2 * CHUNK + 3, 1))
    for i, (T, rows) in enumerate(shapes):
        cs.append(_shape("T%d_rows%d" % (T, rows), rows, T, i % 4, ((i // 4 + i) % 4, (i + 2) % 4)))
    # every pair of word offsets within 16 bytes, data against noise, on a shape whose rows share vectors, more than one apply tile
    for off in range(4):
        for noff in range(4):
            T = 3 * STRANDS + 1 + 512
            cs.append(_case("offsets_%d_%d" % (off, noff), 3, T, [T, T - 2], [[T, 100], [T]],
                            [[(0, 0, 0, 0, 0.0), (0, 1, 2, 1, 4.0), (1, 0, 0, 1, 8.0)], [(0, 1, 4, 1, 1.0), (1, 0, 5, 0, -1.0)]], off, (noff, (noff + off + 1) % 4)))
    # every period looped at least twice, one row (CT and TC are one kernel), two and three rows (TC's own sum kernel)
    T = 3 * max(PERIODS) + 5
    for i, rows in enumerate((1, 2, 3)):
        cs.append(_loops("loops_T%d_rows%d" % (T, rows), rows, T, (i + 1) % 4, (2 * i + 3) % 4))
    # dead terms between live ones: an all-zero noise, +inf, an index of -1; and an all-zero signal beside them
    cs.append(_case("dead_between", 2, 70, [70, 70, 70, 33], [[70, 70, 20]],
                    [[(0, 1, 0, 0, 0.0), (0, 0, 3, 1, 0.0), (0, 2, 5, 1, 2.0)], [(0, 1, 0, 0, 0.0), (0, 1, 3, 1, INF), (0, 2, 5, 1, 2.0)],
                     [(0, 1, 0, 0, 0.0), (0, -1, 3, 1, 1.0), (0, 2, 5, 1, 2.0)], [(0, 1, 0, 0, 0.0), (0, 2, 1, 1, -3.0)]], 1, (3,), kind="zeros"))
    # disjoint covers (foreground noises along the utterance) and the snr's range
    cs.append(_case("disjoint", 2, 300, [300, 257], [[10, 17, 40]],
                    [[(0, 0, 0, 0, 0.0), (0, 1, 20, 0, -200.0), (0, 2, 100, 0, 200.0), (0, 0, 295, 0, 5.0)], [(0, 2, 250, 0, 3.0), (0, 1, 7, 0, 3.0)]], 2, (1,)))
    return cs


MATRIX = _matrix()
NAMES = [c["name"] for c in MATRIX]


def case(name):
    return MATRIX[NAMES.index(name)]


def data(c):
    """(x [B, rows, T], [noise [N_b, rows, T] per batch]) float32 (CT), seeded by the case's name.  Data cells at t >= valid[k] and
    noise cells at t >= noise_valid hold PAD_WORD: a NaN that must reach neither a sum nor a cell, and words that must stay."""
    B, rows, T = len(c["valid"]), c["rows"], c["T"]
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    x = (rng.standard_normal((B, rows, T)) * rng.uniform(0.05, 2.0, (B, rows, 1))).astype(np.float32)
    noises = [(rng.standard_normal((len(nv), rows, T)) * rng.uniform(0.01, 8.0, (len(nv), rows, 1))).astype(np.float32) for nv in c["noise_valid"]]
    if c["kind"] == "zeros":
        noises[0][0] = np.float32(0.0)                       # En == 0
        x[3] = np.float32(0.0)                               # Es == 0
        x[3, 0, ::2] = np.float32(-0.0)
    for k, v in enumerate(c["valid"]):
        x[k, :, v:].view(np.uint32)[...] = PAD_WORD
    for n, nv in zip(noises, c["noise_valid"]):
        for j, v in enumerate(nv):
            n[j, :, v:].view(np.uint32)[...] = PAD_WORD
    return x, noises


def run(c, x, noises, layout, call):
    """The case's batches laid out in guarded buffers at the case's offsets and handed to call(body, shape, noise bodies, n_noise,
    noise_valid, term_first, terms, gains body) -> launched; returns (cells [B, rows, T], gains [M], launched) and checks the
    guard bands around the batch and the gains and every word of the noises."""
    B, rows, T = x.shape
    flat, body = guarded(x.size, c["offset"])
    body[:] = as_layout(x, layout).reshape(-1)
    nbufs = []
    for n, off in zip(noises, c["noise_offsets"]):
        nflat, nbody = guarded(n.size, off)
        nbody[:] = as_layout(n, layout).reshape(-1)
        nbufs.append((nflat, nbody, nflat.view(np.uint32).copy()))
    first, terms = sd.flatten(c["terms"])
    M = max(int(first[-1]), 1)
    gflat, gbody = guarded(M, 1)
    launched = call(body, (B, rows, T), [b for _, b, _ in nbufs], [n.shape[0] for n in noises], np.concatenate([np.asarray(v, dtype=np.uint32) for v in c["noise_valid"]]),
                    first, terms, gbody)
    assert guards_intact(flat, x.size, c["offset"]), (c["name"], "a guard word around the batch was written")
    for nflat, _, before in nbufs:
        assert np.array_equal(nflat.view(np.uint32), before), (c["name"], "a noise batch was written")
    assert guards_intact(gflat, M, 1), (c["name"], "a guard word around the gains was written")
    cells = from_layout(body.reshape((B, T, rows) if layout == sd.TC else (B, rows, T)).copy(), layout)
    return cells, gbody[:int(first[-1])].copy(), launched


def _sim_call(valid, layout):
    def call(body, shape, nbodies, n_noise, noise_valid, first, terms, gbody):
        return sd.addn_windows(body, valid, nbodies, noise_valid, first, terms, layout, gbody, shape=shape, n_noise=n_noise)
    return call


_SIM = {}


def simulated(name, layout):
    """(cells [B, rows, T], gains [M]) of the case under the simulator in `layout`, computed once."""
    key = (name, layout)
    if key not in _SIM:
        c = case(name)
        x, noises = data(c)
        cells, gains, launched = run(c, x, noises, layout, _sim_call(c["valid"], layout))
        assert launched, name
        _SIM[key] = (cells, gains)
    return _SIM[key]
