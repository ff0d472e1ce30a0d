"""The cases of the noise mixer (clx_add_windows), shared by the simulator tests and the GPU tests: the edge matrix of the sums'
order, the live ranges and the tiling.  Nothing here touches a GPU."""
import numpy as np

import simlib_add as sa
from norm_cases import GUARD, NAN_FILL, as_layout, from_layout, guarded, guards_intact, same_words

CHUNK, STRANDS = sa.CHUNK, sa.STRANDS
PAD_WORD = 0x7fc0beef                    # what data cells at t >= Vs and noise cells at t >= noise_valid hold: a NaN with a payload
INF = float("inf")


def _case(name, rows, T, valid, noise_valid, index, snr, offset=0, noise_offset=0, kind="normal"):
    assert len(valid) == len(index) == len(snr) and all(-1 <= j < len(noise_valid) for j in index)
    return dict(name=name, rows=rows, T=T, valid=list(valid), noise_valid=list(noise_valid), index=list(index), snr=list(snr), offset=offset,
                noise_offset=noise_offset, kind=kind)


def _six(name, rows, T, offset, noise_offset):
    """Six windows over five noise windows: the whole window; an empty signal; one live sample, sharing noise 0 with window 0
    (noise_valid > Vs); a noise that ends inside the window (Vn < Vs; Vn == 0 at T == 1); no noise; noise_valid > Vs, in between."""
    valid = [T, 0, min(1, T), T, T // 2 + 1, max(T - 1, 0)]
    return _case(name, rows, T, valid, [T, T, T // 2, T, 0], [0, 1, 0, 2, -1, 3], [0.0, 5.0, 200.0, -200.0, 3.0, 10.5], offset, noise_offset)


def _matrix():
    cs = []
    shapes = ((1, 1), (1, 3), (63, 2), (63, 8), (64, 8), (64, 1), (65, 3), (65, 2), (CHUNK - 1, 2), (CHUNK, 3), (CHUNK, 1), (CHUNK + 1, 1),
              (CHUNK + 1, 2), (2 * CHUNK + 3, 3), (2 * CHUNK + 3, 1))
    for i, (T, rows) in enumerate(shapes):
        cs.append(_six("T%d_rows%d" % (T, rows), rows, T, i % 4, (i // 4 + i) % 4))
    # every pair of offsets within 16 bytes on one shape whose rows share vectors (T no multiple of 4), more than one apply tile
    for off in range(4):
        cs.append(_six("offset%d_rows8" % off, 8, 3 * STRANDS + 1 + 512, off, (off + 1 + off // 2) % 4))
    # the ratio's range: -200, 0, 200 and +inf on whole windows, one noise window for all four
    cs.append(_case("snr_range", 2, 70, [70, 70, 70, 70], [70], [0, 0, 0, 0], [-200.0, 0.0, 200.0, INF]))
    # energies of zero: an all-zero noise, an all-zero signal, a noise with no live sample, and one ordinary window beside them
    cs.append(_case("zero_energy", 3, 70, [70, 70, 70, 33], [70, 70, 0], [0, 1, 2, 1], [0.0, 0.0, 0.0, -3.0], 1, 3, kind="zeros"))
    return cs


MATRIX = _matrix()
NAMES = [c["name"] for c in MATRIX]


def case(name):
    return MATRIX[NAMES.index(name)]


def data(c):
    """(x [B, rows, T], noise [N, rows, T]) float32 (CT), seeded by the case's name.  Data cells at t >= valid[k] and noise cells at
    t >= noise_valid[j] hold PAD_WORD: a NaN that must reach neither a sum nor a cell, and words that must stay."""
    B, N, rows, T = len(c["valid"]), len(c["noise_valid"]), c["rows"], c["T"]
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    x = (rng.standard_normal((B, rows, T)) * rng.uniform(0.05, 2.0, (B, rows, 1))).astype(np.float32)
    n = (rng.standard_normal((N, rows, T)) * rng.uniform(0.01, 8.0, (N, rows, 1))).astype(np.float32)
    if c["kind"] == "zeros":
        n[0] = np.float32(0.0)                               # window 0: En == 0
        x[1] = np.float32(0.0)                               # window 1: Es == 0
        x[1, 0, ::2] = np.float32(-0.0)
    for k, v in enumerate(c["valid"]):
        x[k, :, v:].view(np.uint32)[...] = PAD_WORD
    for j, v in enumerate(c["noise_valid"]):
        n[j, :, v:].view(np.uint32)[...] = PAD_WORD
    return x, n


_SIM = {}


def simulated(name, layout):
    """(cells [B, rows, T], gains [B]) of the case under the simulator in `layout`, computed once; the guard bands around the batch
    and the gains, and every word of the noise, are checked here."""
    key = (name, layout)
    if key not in _SIM:
        c = case(name)
        x, n = data(c)
        B, rows, T = x.shape
        flat, body = guarded(x.size, c["offset"])
        body[:] = as_layout(x, layout).reshape(-1)
        nflat, nbody = guarded(n.size, c["noise_offset"])
        nbody[:] = as_layout(n, layout).reshape(-1)
        before = nflat.view(np.uint32).copy()
        gflat, gbody = guarded(B, 1)
        launched = sa.add_windows(body, c["valid"], nbody, c["noise_valid"], c["index"], c["snr"], layout, gbody, shape=(B, rows, T),
                                  n_noise=n.shape[0])
        assert launched, name
        assert guards_intact(flat, x.size, c["offset"]), (name, "a guard word around the batch was written")
        assert np.array_equal(nflat.view(np.uint32), before), (name, "the noise was written")
        assert guards_intact(gflat, B, 1), (name, "a guard word around the gains was written")
        cells = from_layout(body.reshape((B, T, rows) if layout == sa.TC else (B, rows, T)).copy(), layout)
        _SIM[key] = (cells, gbody.copy())
    return _SIM[key]
