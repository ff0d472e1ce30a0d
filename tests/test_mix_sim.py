"""The channel-mixing window reader (clx_mix.hip: clx_mix_plan, clx_mix_fill and clx_k_mix) under the wave simulator.  At the native
rate a window is compared as uint32 words with the mix's definition evaluated with numpy float32 scalars in the stated order
(simlib_mix.mix).  Under resampling the mixed float32 values are exact by definition, so the resampler's own bound holds unchanged:
per output |y - y64| <= gamma * sum_k |h_k x_k| against simlib_resample.reference on the mixed signal, gamma = N u / (1 - N u),
u = 2^-24, N = 2W + 2; an identity is bit-equal to clx_k_resample on the same inputs and replicated channels are bit-equal to each
other.  The source is 700 random samples per channel (more only where a window of one tile and one output has to be all valid);
every window's span sits between NaNs at its own 4-byte alignment, the output starts as a NaN pattern with a guard word behind it."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_mix as sm
import simlib_resample as sr
from test_resample_sim import GUARD, LAYOUTS, NAN_FILL, PAIRS, TILE, T, Win, _signal, _starts

NATIVE = 22050                   # the rate of the windows that are cut at their own rate


class Cut:
    """A window of x [T, Cs] at its own rate with a chosen valid: samples st .. st + valid - 1 (Win's fields)."""

    def __init__(self, x, st, valid, fs=NATIVE):
        self.x, self.seen, self.fs, self.st, self.valid = x, x, fs, st, valid
        self.lo, self.hi = (st, st + valid) if valid else (0, 0)


def _source(wins):
    """The spans back to back with NaNs between, each at its own 4-byte alignment: (floats, each span's first float)."""
    parts, first, at = [], [], 1
    for w in wins:
        parts.append(np.full(at - sum(p.size for p in parts), np.nan, dtype=np.float32))
        first.append(at)
        parts.append(w.x[w.lo:w.hi].reshape(-1))
        at += (w.hi - w.lo) * w.x.shape[1] + 3
    parts.append(np.full(8, np.nan, dtype=np.float32))
    return np.ascontiguousarray(np.concatenate(parts)), first


def _shaped(buf, B, L, K, layout):
    n = B * L * K
    assert buf[n] == GUARD, "the word behind the output was written"
    out = buf[:n].view(np.float32)
    return out.reshape(B, K, L).transpose(0, 2, 1) if layout == sr.CT else out.reshape(B, L, K)


def _run(wins, R, L, K, layout, shift=0, t_shift=0):
    """One clx_mix_windows call over `wins`; the output as [B, L, K] float32.  shift / t_shift move every window's outputs and
    source samples along their streams (the large offsets)."""
    src, first = _source(wins)
    buf = np.full(len(wins) * L * K + 1, NAN_FILL, dtype=np.uint32)
    buf[-1] = GUARD
    sm.mix_windows(src, first, [w.lo + t_shift for w in wins], [w.hi - w.lo for w in wins], [w.st + shift for w in wins],
                   [w.valid for w in wins], [w.fs for w in wins], [w.x.shape[1] for w in wins], R, L, K, layout, buf)
    return _shaped(buf, len(wins), L, K, layout)


def _run_resample(wins, R, L, C, layout):
    """The same call shape through clx_resample_windows (every window has C channels)."""
    src, first = _source(wins)
    buf = np.full(len(wins) * L * C + 1, NAN_FILL, dtype=np.uint32)
    buf[-1] = GUARD
    sr.resample_windows(src, first, [w.lo for w in wins], [w.hi - w.lo for w in wins], [w.st for w in wins], [w.valid for w in wins],
                        [w.fs for w in wins], R, L, C, layout, buf)
    return _shaped(buf, len(wins), L, C, layout)


def _compare(got, wins, R, L, K, layout):
    """got [B, L, K] against the definition, window by window; returns the worst |error| / bound of the resampled ones."""
    worst = 0.0
    for k, w in enumerate(wins):
        Cs = w.x.shape[1]
        what = (w.fs, R, L, Cs, K, layout, "window %d at %d" % (k, w.st))
        assert np.all(got[k, w.valid:].view(np.uint32) == 0), (what, "the window's tail is not zeros")
        want = sm.mix(w.seen, K)
        if w.fs == R:
            assert np.array_equal(got[k, :w.valid].view(np.uint32), want[w.st:w.st + w.valid].view(np.uint32)), (what, "not the mix")
        elif w.valid:
            worst = max(worst, sr.assert_close(got[k, :w.valid], want, w.fs, R, np.arange(w.st, w.st + w.valid), what))
        if Cs == 1:
            for c in range(1, K):
                assert np.array_equal(got[k, :, c].view(np.uint32), got[k, :, 0].view(np.uint32)), (what, "replicated channels differ")
    same = [k for k, w in enumerate(wins) if w.x.shape[1] == K]
    if same:                                                 # identities: what clx_k_resample gives, bit for bit
        ref = _run_resample([wins[k] for k in same], R, L, K, layout)
        assert np.array_equal(got[same].view(np.uint32), ref.view(np.uint32)), (R, L, K, layout, "an identity differs from clx_k_resample")
    return worst


def _check(wins, R, L, K, layout):
    return _compare(_run(wins, R, L, K, layout), wins, R, L, K, layout)


def _valids(L):
    return sorted({0, 1, L - 1, L})


@pytest.mark.parametrize("Cs", (2, 3, 5, 8))
def test_native_rate_reduce(Cs):
    """The mean of Cs channels, bit for bit, for window lengths around the 16-byte and the tile's edges and valid = 0, 1, L - 1, L;
    K = 1 is the same bytes in both layouts."""
    for L in (1, 3, 4, 5, 257, TILE + 1):
        x = _signal(100 * Cs + L, Cs, T=max(T, L + 40))
        wins = [Cut(x, 3 + 7 * i, v) for i, v in enumerate(_valids(L))]
        got = [_run(wins, NATIVE, L, 1, layout) for layout in LAYOUTS]
        assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
        _compare(got[0], wins, NATIVE, L, 1, sr.TC)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_native_rate_replicate_and_identity(layout):
    """Any bit pattern (NaNs and denormals too) moves unchanged: a mono source to each of K channels, C channels to C."""
    rng = np.random.default_rng(77 + layout)
    for L in (5, 257, TILE + 1):
        for Cs, K in ((1, 2), (1, 3), (1, 8), (1, 1), (2, 2), (3, 3)):
            x = rng.integers(0, 1 << 32, size=(max(T, L + 40), Cs), dtype=np.uint64).astype(np.uint32).view(np.float32)
            _check([Cut(x, 2 + 5 * i, v) for i, v in enumerate(_valids(L))], NATIVE, L, K, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fs,R", PAIRS)
def test_resampled_reduce_replicate_identity(fs, R, layout):
    """tests/test_resample_sim.py's rate pairs and window positions: 2 -> 1 and 3 -> 1 within the bound on the mix of what the span
    shows, 1 -> 2 within it with equal channels, 2 -> 2 equal to clx_k_resample."""
    T_R = sr.length_at(T, fs, R)
    for Cs, K in ((2, 1), (3, 1), (1, 2), (2, 2)):
        x = _signal(fs + 10 * Cs + K + layout, Cs)
        for L in (257, TILE + 1):
            if L > 257 and T_R <= L:
                continue
            wins = [Win(x, fs, R, st, L) for st in _starts(T_R, L)]
            assert wins[0].lo == 0 and any(w.lo > 0 for w in wins) and any(0 < w.valid < L for w in wins) and wins[-1].valid == 0
            worst = _check(wins, R, L, K, layout)
            print("%d -> %d, L %d, %d -> %d channels, layout %d: worst |error| / bound %.3f" % (fs, R, L, Cs, K, layout, worst))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_call_mixes_rules_rates_and_copies(layout):
    """Every kind of window in one call.  A reduce needs K == 1 and a replicate K > 1, so it takes two calls to meet all of them:
    K = 1 with an identity (mono) copy and resample, a reduce copy, reduces resampled at two pairs and a dead window; K = 2 with an
    identity copy and resample, a replicate copy and resample and a dead window.  The tables are clx_resample_windows' own."""
    L, R = 257, 16000
    x = {(fs, C): _signal(fs + C, C, T=T + 13 * C) for fs in (44100, 48000, 16000) for C in (1, 2, 3)}
    win = lambda fs, C, st: Win(x[fs, C], fs, R, st, L)
    k1 = [win(16000, 1, 5), win(44100, 1, 40), win(16000, 3, 0), win(44100, 2, 100), win(48000, 3, 7), win(44100, 2, 10 ** 6),
          win(16000, 2, T - 100)]
    k2 = [win(16000, 2, 5), win(48000, 2, 40), win(16000, 1, 700), win(44100, 1, 100), win(48000, 1, 10 ** 6), win(44100, 2, 0)]
    assert k1[5].valid == 0 and k2[4].valid == 0 and 0 < k1[6].valid < L and 0 < k2[2].valid < L
    _check(k1, R, L, 1, layout)
    pairs, floats = sm.lib().sim_mix_cached_pairs(), sm.lib().sim_mix_cached_floats()
    assert pairs >= 2
    _check(k2, R, L, 2, layout)
    _check(k1[::-1], R, L, 1, layout)
    # a pair built by clx_mix_windows serves clx_resample_windows on the same cache, and the other way round
    src, first = _source(k2[:2])
    buf = np.full(2 * L * 2 + 1, NAN_FILL, dtype=np.uint32)
    buf[-1] = GUARD
    sm.resample_windows(src, first, [w.lo for w in k2[:2]], [w.hi - w.lo for w in k2[:2]], [w.st for w in k2[:2]], [w.valid for w in k2[:2]],
                        [w.fs for w in k2[:2]], R, L, 2, layout, buf)
    assert (sm.lib().sim_mix_cached_pairs(), sm.lib().sim_mix_cached_floats()) == (pairs, floats)
    assert np.array_equal(_shaped(buf, 2, L, 2, layout).view(np.uint32), _run_resample(k2[:2], R, L, 2, layout).view(np.uint32))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_large_offsets(layout):
    """out_t0 = 2^40 + 3 for a reduce over two tiles.  At the native rate src_t0 moves by the same amount.  Resampled, the filter
    has period n in the outputs and o in the source: the window moved by q n outputs and q o source samples is the same window."""
    L, big = TILE + 1, (1 << 40) + 3
    x = _signal(40, 2, T=3300)
    w = Cut(x, 3, L)
    got = _run([w], NATIVE, L, 1, layout, shift=big - 3, t_shift=big - 3)
    _compare(got, [w], NATIVE, L, 1, layout)
    fs, R = 44100, 16000
    o, n, _ = sr.pair(fs, R)
    q, st = divmod(big, n)
    w = Win(x, fs, R, st, L)
    assert w.valid == L
    got = _run([w], R, L, 1, layout, shift=q * n, t_shift=q * o)
    assert _compare(got, [w], R, L, 1, layout) <= 1.0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Cs,K", ((2, 1), (3, 1), (1, 2), (2, 2)))
def test_loads_stay_inside_the_span(Cs, K, layout):
    """The span ends on the last float before an inaccessible page, or begins on the first float behind one: a stray load would
    fault.  The window that starts at the stream's end has no span at all and points at the inaccessible page itself."""
    L = 257
    for fs, R in ((44100, 16000), (16000, 44100), (11025, 11025)):
        x = _signal(fs + Cs + K, Cs)
        T_R = T if fs == R else sr.length_at(T, fs, R)
        for st in (0, T_R // 3, max(T_R - L // 2, 0), T_R):
            w = Win(x, fs, R, st, L)
            for at_end in (True, False):
                out = np.full(L * K + 1, NAN_FILL, dtype=np.uint32)
                out[-1] = GUARD
                sm.mix_guarded(x[w.lo:w.hi], w.lo, w.hi - w.lo, st, w.valid, fs, Cs, R, L, K, layout, at_end, out)
                _compare(_shaped(out, 1, L, K, layout), [w], R, L, K, layout)
                assert w.valid or w.hi == w.lo


def test_refused_arguments_and_empty_calls():
    src = np.zeros(64, dtype=np.float32)
    out = np.zeros(64, dtype=np.float32)
    ok = dict(src=src, src_first=[0], src_t0=[0], src_n=[4], out_t0=[0], valid=[4], src_rate=[44100], src_channels=[2], out_rate=16000,
              window_len=4, out_channels=1, layout=sr.TC, out=out)
    sm.mix_windows(**ok)
    for change, why in ((dict(out_channels=0), "out_channels must be 1..8"), (dict(out_channels=9), "out_channels must be 1..8"),
                        (dict(src_channels=[0]), "src_channels[k] must be 1..8"), (dict(src_channels=[9]), "src_channels[k] must be 1..8"),
                        (dict(src_channels=[3], out_channels=2), "no rule brings 3 channels to 2 (window 0)"),
                        (dict(src_channels=[6], out_channels=2), "no rule brings 6 channels to 2 (window 0)"),
                        (dict(src_channels=[2], out_channels=3), "no rule brings 2 channels to 3 (window 0)"),
                        (dict(src_channels=None), "null argument"),
                        (dict(layout=2), "layout must be"), (dict(layout=7), "layout must be"), (dict(valid=[5]), "valid[k] is larger"),
                        (dict(src=None), "null argument"), (dict(out=None), "null argument"), (dict(src_first=None), "null argument"),
                        (dict(src_t0=None), "null argument"), (dict(src_n=None), "null argument"), (dict(out_t0=None), "null argument"),
                        (dict(valid=None), "null argument"), (dict(src_rate=None), "null argument"),
                        (dict(src_rate=[0]), "src_rate[k] must be"), (dict(src_rate=[1 << 20]), "src_rate[k] must be"),
                        (dict(out_rate=0), "out_rate must be"), (dict(out_rate=1 << 20), "out_rate must be"),
                        (dict(out_rate=16001), "coefficient table"), (dict(src_rate=[(1 << 20) - 1], out_rate=(1 << 20) - 3), "coefficient table"),
                        (dict(out_t0=[1 << 43]), "out_t0[k] is too large")):
        with pytest.raises(cx.ClaxonError) as e:
            sm.mix_windows(**dict(ok, **change))
        assert e.value.status == cx.API_ERROR and e.value.message.startswith("clx_mix_windows: ") and why in e.value.message, (change, e.value.message)
    # two windows, the second one refused: its number is in the text
    two = dict(src_first=[0, 0], src_t0=[0, 0], src_n=[4, 4], out_t0=[0, 0], valid=[4, 4], src_rate=[44100, 44100])
    with pytest.raises(cx.ClaxonError) as e:
        sm.mix_windows(**dict(ok, out_channels=2, src_channels=[1, 5], **two))
    assert "no rule brings 5 channels to 2 (window 1)" in e.value.message
    with pytest.raises(cx.ClaxonError) as e:
        sm.mix_windows(**dict(ok, src_channels=[2, 3], **dict(two, valid=[4, 5])))
    assert "valid" in e.value.message
    # more blocks than a grid has
    z = [0] * 512
    with pytest.raises(cx.ClaxonError) as e:
        sm.mix_windows(**dict(ok, src_first=z, src_t0=z, src_n=z, out_t0=z, valid=z, src_rate=[44100] * 512, src_channels=[2] * 512,
                              window_len=(1 << 32) - 1))
    assert "too many" in e.value.message
    # the empty calls succeed, touch nothing and need no pointer
    out[:] = 7.0
    none = dict(src_first=[], src_t0=[], src_n=[], out_t0=[], valid=[], src_rate=[], src_channels=[])
    sm.mix_windows(**dict(ok, **none))
    sm.mix_windows(**dict(ok, src=None, out=None, **none))
    sm.mix_windows(**dict(ok, valid=[0], window_len=0))
    sm.mix_windows(**dict(ok, src=None, out=None, src_channels=None, valid=[0], window_len=0))
    assert np.all(out == 7.0)
    with pytest.raises(cx.ClaxonError):
        sm.mix_windows(**dict(ok, src=None, out=None, out_channels=0, **none))          # (out_channels, layout and out_rate are checked first)
