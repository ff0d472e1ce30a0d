"""The resampling window reader (clx_resample.hip: clx_resample_plan, clx_resample_fill, the table builder and clx_k_resample) under the
wave simulator, against the resampler's definition evaluated in float64 with numpy (simlib_resample.reference: from the float32
source samples, without the library's table).  Per output |y - y64| <= gamma * sum_k |h_k x_k| with gamma = N u / (1 - N u),
u = 2^-24, N = 2W + 2 -- the bound of an N-term float32 dot product in any order, one term more for the table's single rounding and
one for libm's double -- and an output without a tap inside the stream is exactly 0.  The source is 700 random samples per channel;
every window's span sits in the source between NaNs, so a tap taken from outside the span shows in the result.  One test moves
the windows to where out_t0 + L is just below 2^43, the largest the call accepts (far_windows, shared with the GPU tests)."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_resample as sr

T = 700
NAN_FILL = 0x7fc0dead            # a quiet NaN with a payload: what the output holds before the call
GUARD = 0xffc0beef               # the word behind the output
PAIRS = ((44100, 16000), (48000, 16000), (16000, 44100), (8000, 16000))
LAYOUTS = (sr.TC, sr.CT)
TILE = 1024                      # clx_rs::kTile


def _signal(seed, C, T=T):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(T, C)).astype(np.float32)


def _starts(T_R, L):
    """Output 0 (zeros to the left of the stream), inside, across the end (valid < L), the last output, at the end and behind it."""
    return sorted({0, 1, T_R // 3, max(T_R - L, 0), max(T_R - L // 2, 0), T_R - 1, T_R, T_R + 7})


class Win:
    """A window of x [T, C] at fs: outputs st .. of the stream resampled to R, with the source span [lo, hi) the formula gives
    (trim = (a, b) cuts a samples off its front and b off its back: those count as zero)."""

    def __init__(self, x, fs, R, st, L, trim=(0, 0), whole=False):
        self.x, self.fs, self.st = x, fs, st
        Tx = x.shape[0]
        self.T_R = Tx if fs == R else sr.length_at(Tx, fs, R)
        self.valid = int(np.clip(self.T_R - st, 0, L))
        if self.valid == 0:
            self.lo = self.hi = 0
        elif fs == R:
            self.lo, self.hi = st, st + self.valid
        else:
            self.lo, self.hi = sr.span(st, st + self.valid - 1, Tx, fs, R)
        if whole:
            self.lo, self.hi = 0, Tx
        self.lo, self.hi = self.lo + trim[0], max(self.hi - trim[1], self.lo + trim[0])
        self.seen = x.copy()                                 # what the window's span lets the resampler see
        self.seen[:self.lo] = 0
        self.seen[self.hi:] = 0


def _run(wins, R, L, C, layout):
    """One call over `wins`; returns the output as [B, L, C] float32."""
    parts, first, at = [], [], 1
    for w in wins:                                           # spans back to back with NaNs between, each at its own 4-byte alignment
        parts.append(np.full(at - sum(p.size for p in parts), np.nan, dtype=np.float32))
        first.append(at)
        parts.append(w.x[w.lo:w.hi].reshape(-1))
        at += (w.hi - w.lo) * C + 3
    parts.append(np.full(8, np.nan, dtype=np.float32))
    src = np.ascontiguousarray(np.concatenate(parts))
    n = len(wins) * L * C
    buf = np.full(n + 1, NAN_FILL, dtype=np.uint32)
    buf[n] = GUARD
    sr.resample_windows(src, first, [w.lo for w in wins], [w.hi - w.lo for w in wins], [w.st for w in wins], [w.valid for w in wins],
                        [w.fs for w in wins], R, L, C, layout, buf)
    assert buf[n] == GUARD, "the word behind the output was written"
    out = buf[:n].view(np.float32)
    return out.reshape(len(wins), C, L).transpose(0, 2, 1) if layout == sr.CT else out.reshape(len(wins), L, C)


def _check(wins, R, L, C, layout):
    got = _run(wins, R, L, C, layout)
    worst = 0.0
    for k, w in enumerate(wins):
        what = (w.fs, R, L, C, layout, "window %d at %d" % (k, w.st))
        assert np.all(got[k, w.valid:].view(np.uint32) == 0), (what, "the window's tail is not zeros")
        if w.fs == R:
            assert np.array_equal(got[k, :w.valid].view(np.uint32), w.seen[w.st:w.st + w.valid].view(np.uint32)), (what, "not a copy")
        elif w.valid:
            worst = max(worst, sr.assert_close(got[k, :w.valid], w.seen, w.fs, R, np.arange(w.st, w.st + w.valid), what))
    return worst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", (1, 2, 3))
@pytest.mark.parametrize("fs,R", PAIRS)
def test_rate_pairs_and_window_positions(fs, R, C, layout):
    """L = 257 for every pair; L = one tile and one output where the resampled stream is longer than that.  Each window's span is
    cut exactly to the formula's, so src_t0 > 0 for all but the first."""
    x = _signal(fs + 10 * C + layout, C)
    T_R = sr.length_at(T, fs, R)
    for L in (257, TILE + 1):
        if L > 257 and T_R <= L:
            continue
        wins = [Win(x, fs, R, st, L) for st in _starts(T_R, L)]
        assert wins[0].lo == 0 and any(w.lo > 0 for w in wins) and any(0 < w.valid < L for w in wins) and wins[-1].valid == 0
        worst = _check(wins, R, L, C, layout)
        print("%d -> %d, L %d, C %d, layout %d: worst |error| / bound %.3f" % (fs, R, L, C, layout, worst))


def test_the_sizes_of_the_pairs():
    assert [sr.pair(*p) for p in PAIRS[:3]] + [sr.pair(44100, 48000)] == [(441, 160, 17), (3, 1, 19), (160, 441, 7), (147, 160, 7)]
    assert [cx.resample_pair(*p) for p in PAIRS] == [sr.pair(*p) for p in PAIRS] and cx.resample_pair(16000, 16000) == (1, 1, 0)
    assert sr.length_at(T, 44100, 16000) == 254 and sr.length_at(T, 8000, 16000) == 1400


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", (1, 2, 3))
def test_an_equal_pair_is_a_copy(C, layout):
    """Any bit pattern (NaNs and denormals too) moves unchanged; a span shorter than the window's samples leaves zeros."""
    rng = np.random.default_rng(5 + C)
    x = rng.integers(0, 1 << 32, size=(T, C), dtype=np.uint64).astype(np.uint32).view(np.float32)
    for L in (257, TILE + 1):
        wins = [Win(x, 22050, 22050, st, L) for st in (0, 3, T - L // 2, T - 1, T, T + 9) if st >= 0]
        wins.append(Win(x, 22050, 22050, 100, L, trim=(5, 2)))
        _check(wins, 22050, L, C, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_call_mixes_rate_pairs_and_a_copy(layout):
    C, L, R = 2, 257, 16000
    xs = {fs: _signal(fs, C, T=T + 13 * i) for i, fs in enumerate((44100, 48000, 8000, 16000))}
    wins = []
    for rnd in range(3):
        for fs, x in xs.items():
            T_R = x.shape[0] if fs == R else sr.length_at(x.shape[0], fs, R)
            wins.append(Win(x, fs, R, (0, T_R // 2, T_R - 40)[rnd], L))
    assert {w.fs for w in wins[:4]} == set(xs)
    pairs0 = sr.lib().sim_resample_cached_pairs()
    _check(wins, R, L, C, layout)
    pairs1, floats1 = sr.lib().sim_resample_cached_pairs(), sr.lib().sim_resample_cached_floats()
    assert pairs0 <= pairs1
    _check(wins[::-1], R, L, C, layout)                      # (the tables are built once per pair and kept)
    assert (sr.lib().sim_resample_cached_pairs(), sr.lib().sim_resample_cached_floats()) == (pairs1, floats1)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_span_wider_or_narrower_than_the_formula(layout):
    """The whole stream as every window's span gives the same outputs; a span cut short counts the missing samples as zero."""
    C, L = 2, 257
    for fs, R in PAIRS:
        x = _signal(3 * fs + 1, C)
        T_R = sr.length_at(T, fs, R)
        wins = [Win(x, fs, R, st, L, whole=True) for st in _starts(T_R, L)]
        wins += [Win(x, fs, R, st, L, trim=trim) for st in (0, T_R // 3) for trim in ((3, 0), (0, 2), (1, 5), (10 ** 6, 0))]
        assert wins[-1].hi == wins[-1].lo                    # (a live window without a single source sample: zeros)
        _check(wins, R, L, C, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", (1, 2, 3))
def test_loads_stay_inside_the_span(C, layout):
    """The span ends on the last float before an inaccessible page, or begins on the first float behind one: a stray load would
    fault.  The window that starts at the stream's end has no span at all and points at the inaccessible page itself."""
    L = 257
    for fs, R in PAIRS + ((11025, 11025),):
        x = _signal(fs + C, C)
        T_R = T if fs == R else sr.length_at(T, fs, R)
        for st in (0, T_R // 3, max(T_R - L // 2, 0), T_R):
            w = Win(x, fs, R, st, L)
            for at_end in (True, False):
                out = np.full(L * C, NAN_FILL, dtype=np.uint32)
                sr.resample_guarded(x[w.lo:w.hi], w.lo, w.hi - w.lo, st, w.valid, fs, R, L, C, layout, at_end, out)
                got = out.view(np.float32)
                got = got.reshape(C, L).T if layout == sr.CT else got.reshape(L, C)
                assert np.all(got[w.valid:].view(np.uint32) == 0)
                if fs == R:
                    assert np.array_equal(got[:w.valid], x[st:st + w.valid])
                elif w.valid:
                    sr.assert_close(got[:w.valid], x, fs, R, np.arange(st, st + w.valid), (fs, R, C, layout, st, at_end))
                else:
                    assert w.hi == w.lo


FAR = 1 << 43                    # clx_rs::kMaxOut: out_t0 + L stays below it


def far_windows(seed, C, L, fs=44100, R=16000):
    """Three windows whose last output is one of the last below 2^43, at three phases (out_t0 mod n), of a stream taken as endless.
    Only the positions are large: a window's source is its span by the formula, noise, and nothing else.  Returns (the source buffer
    with the spans between NaNs from an odd float on, the per-window arguments of resample_windows in its order, the spans)."""
    o, n, _ = sr.pair(fs, R)
    rng = np.random.default_rng(seed)
    out_t0 = [FAR - L - back for back in (1, 2, 79)]
    assert len({m0 % n for m0 in out_t0}) == 3 and min(out_t0) > 1 << 42
    spans = [sr.span(m0, m0 + L - 1, 1 << 62, fs, R) for m0 in out_t0]
    xs = [rng.uniform(-1.0, 1.0, size=(hi - lo, C)).astype(np.float32) for lo, hi in spans]
    parts, first = [np.full(1, np.nan, dtype=np.float32)], []
    for x in xs:
        first.append(sum(p.size for p in parts))
        parts += [x.reshape(-1), np.full(3, np.nan, dtype=np.float32)]
    assert any(f % 2 for f in first)
    args = (first, [lo for lo, _ in spans], [hi - lo for lo, hi in spans], out_t0, [L] * 3, [fs] * 3)
    return np.ascontiguousarray(np.concatenate(parts)), args, xs


@pytest.mark.parametrize("layout", LAYOUTS)
def test_windows_that_end_just_below_two_to_the_43(layout):
    """The block's one 64-bit product and quotient, m0 * o / n, at the largest m0 the call accepts (m0 * o is about 2^51.8), in the
    window's first tile and in its second; the reference takes the same positions as int64."""
    C, L, fs, R = 2, TILE + 6, 44100, 16000
    src, args, xs = far_windows(43, C, L, fs, R)
    n = 3 * L * C
    buf = np.full(n + 1, NAN_FILL, dtype=np.uint32)
    buf[n] = GUARD
    sr.resample_windows(src, *args, R, L, C, layout, buf)
    assert buf[n] == GUARD, "the word behind the output was written"
    out = buf[:n].view(np.float32)
    got = out.reshape(3, C, L).transpose(0, 2, 1) if layout == sr.CT else out.reshape(3, L, C)
    for k, x in enumerate(xs):
        worst = sr.assert_close(got[k], x, fs, R, args[3][k] + np.arange(L, dtype=np.int64), (layout, k), t0=args[1][k])
        print("out_t0 2^43 - %d, layout %d: worst |error| / bound %.3f" % (FAR - args[3][k], layout, worst))


def test_refused_arguments_and_empty_calls():
    src = np.zeros(64, dtype=np.float32)
    out = np.zeros(64, dtype=np.float32)
    ok = dict(src=src, src_first=[0], src_t0=[0], src_n=[4], out_t0=[0], valid=[4], src_rate=[44100], out_rate=16000, window_len=4,
              channels=2, layout=sr.TC, out=out)
    sr.resample_windows(**ok)
    for change, why in ((dict(channels=0), "channels"), (dict(channels=9), "channels"), (dict(layout=2), "layout"), (dict(layout=7), "layout"),
                        (dict(valid=[5]), "valid"), (dict(src=None), "null"), (dict(out=None), "null"), (dict(src_first=None), "null"),
                        (dict(src_t0=None), "null"), (dict(src_n=None), "null"), (dict(out_t0=None), "null"), (dict(valid=None), "null"),
                        (dict(src_rate=None), "null"), (dict(src_rate=[0]), "rate"), (dict(src_rate=[1 << 20]), "rate"),
                        (dict(out_rate=0), "rate"), (dict(out_rate=1 << 20), "rate"), (dict(out_rate=16001), "table"),
                        (dict(src_rate=[(1 << 20) - 1], out_rate=(1 << 20) - 3), "table"), (dict(out_t0=[1 << 43]), "out_t0")):
        with pytest.raises(cx.ClaxonError) as e:
            sr.resample_windows(**dict(ok, **change))
        assert e.value.status == cx.API_ERROR and e.value.message and why in e.value.message, (change, e.value.message)
    # two windows, the second one refused
    with pytest.raises(cx.ClaxonError) as e:
        sr.resample_windows(**dict(ok, src_first=[0, 0], src_t0=[0, 0], src_n=[4, 4], out_t0=[0, 0], valid=[4, 5], src_rate=[44100, 44100]))
    assert "valid" in e.value.message
    # more blocks than a grid has: 512 windows of 2^22 tiles each (refused before anything is looked at on the device side)
    z = [0] * 512
    with pytest.raises(cx.ClaxonError) as e:
        sr.resample_windows(**dict(ok, src_first=z, src_t0=z, src_n=z, out_t0=z, valid=z, src_rate=[44100] * 512, window_len=(1 << 32) - 1))
    assert "too many" in e.value.message
    # the empty calls succeed, touch nothing and need no pointer
    out[:] = 7.0
    none = dict(src_first=[], src_t0=[], src_n=[], out_t0=[], valid=[], src_rate=[])
    sr.resample_windows(**dict(ok, **none))
    sr.resample_windows(**dict(ok, src=None, out=None, **none))
    sr.resample_windows(**dict(ok, valid=[0], window_len=0))
    sr.resample_windows(**dict(ok, src=None, out=None, valid=[0], window_len=0))
    assert np.all(out == 7.0)
    with pytest.raises(cx.ClaxonError):
        sr.resample_windows(**dict(ok, src=None, out=None, channels=0, **none))          # (channels, layout and out_rate are checked first)
