"""Reflected mel specs -- Kaldi's snip_edges=false -- under the wave simulator (clx_mel.hip: clx_mel_build_reflected, clx_mel_check,
clx_mel_fill_r, clx_k_mel_fr and clx_k_mel_qr).  The equality that carries the feature: for every window the test builds, with Kaldi's
loop written out (simlib_melr.kaldi_index), the explicitly reflected samples p[i] = a[r(i + H/2 - Nw/2)] that the window's live frames
span, runs the existing whole-frame spec with the same tables on the batch of p, and the reflected spec's live cells must be the same
words -- clx_k_mel_fr against clx_k_mel_f and, unconditioned, clx_k_mel; clx_k_mel_qr against clx_k_mel_q, energy row included.  A
cell's order of sums depends on the tap number alone, so this holds on any float input.  Beside it: the count rule, a batch with NaNs
from valid[k] on between inaccessible pages, a group computed once through direct addressing and once through the index map, every new
refusal by its text and the tables of the _reflected constructors."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_mel as sm
import simlib_melr as sr
from test_melq_sim import EPS, GUARD, NAN_FILL, PRE, _bank, _pcm, _same, _tables
from test_melq_sim import _window as _povey

# (Nw, N, H, n_mels, n_bins): Kaldi's defaults; small; odd numbers, where the integer divisions matter; H > Nw, a positive origin and
# reflection at the end only; the smallest; two passes
SHAPES = ((400, 512, 160, 80, 256), (25, 32, 10, 5, 16), (9, 16, 5, 3, 9), (7, 16, 40, 3, 9), (1, 2, 1, 1, 1), (600, 1024, 200, 40, 512))
CEPS = ((400, 512, 160, 23, 256, 13), (400, 512, 160, 128, 256, 40))
LAYOUTS = (sm.CT, sm.TC)
MODES = (sm.LN, sm.POWER)
COND = dict(remove_dc=1, preemph=PRE)
SCALE = 2.0 ** 30


def _window(Nw):
    return _povey(Nw) if Nw > 1 else np.array([32768.0], dtype=np.float32)        # (the povey window of one point is 0)


def _fb(N, n_mels, n_bins):
    return _bank(N, n_mels, n_bins) if N > 2 else np.ones((1, 1), dtype=np.float32)  # (Kaldi's bank of one bin is empty)


def valids(Nw, H):
    """For 400 / 160: 0, 1, 2, 79, 80, 81, 119, 120, 121, 239, 240, 399, 400, 401, 33 * 160, 37 * 160 + 77 -- around the first frame
    (H / 2), where one fold is enough (Nw / 2 - H / 2), where a frame is whole, and long windows; the analogous values otherwise."""
    h, o = H // 2, Nw // 2 - H // 2
    v = [0, 1, 2, h - 1, h, h + 1, o - 1, o, o + 1, Nw - H - 1, Nw - H, Nw - 1, Nw, Nw + 1, 33 * H, 37 * H + 77 * H // 160]
    return np.array([max(x, 0) for x in v], dtype=np.uint32)


def frame_counts(Nw, H):
    V = valids(Nw, H)
    return (1, 33, 37, int(((V.astype(np.int64) + H // 2) // H).max()) + 3)


def batch(Nw, H, seed, noise=False):
    """16-bit audio as load() gives it (or float noise), NaN from valid[k] on: (a [16, L], valid)."""
    V = valids(Nw, H)
    L = int(V.max()) + 5
    a = np.random.default_rng(seed).standard_normal((len(V), L)).astype(np.float32) if noise else _pcm((len(V), L), seed)
    for k in range(len(V)):
        a[k, V[k]:] = np.nan
    return a, V


def _run(h, a, valid, T, layout, guarded=None, tables=False):
    """One call through simlib_melr; the output as [B, T, rows] (a view), after the guard word's check."""
    B, n_rows = a.shape[0], sr.rows(h)
    n = B * n_rows * T
    raw = np.full(n + 8, NAN_FILL, dtype=np.uint32)
    buf = raw[3:3 + n + 1]
    buf[n] = GUARD
    extra = None
    if guarded is None:
        src = np.full(a.size + 16, np.nan, dtype=np.float32)   # the batch between NaNs, at an odd 4-byte alignment
        src[7:7 + a.size] = a.reshape(-1)
        res = sr.mel_windows(h, src[7:7 + a.size].reshape(a.shape), valid, T, layout, buf, **(dict(tables=True) if tables else {}))
        if tables:
            extra = res[1]
    else:
        sr.mel_guarded(h, a, valid, T, layout, guarded, buf)
    assert buf[n] == GUARD and np.all(raw[:3] == NAN_FILL), "a word outside the output was written"
    assert not np.any(buf[:n] == NAN_FILL), "an output word was not written"
    out = buf[:n].view(np.float32)
    out = out.reshape(B, n_rows, T).transpose(0, 2, 1) if layout == sm.CT else out.reshape(B, T, n_rows)
    return (out, extra) if tables else out


def _pair(shape, mode, opts, cep=None):
    """(the reflected spec, its whole-frame sibling with the same tables)."""
    Nw, N, H, n_mels, n_bins = shape[:5]
    w, fb = _window(Nw), _fb(N, n_mels, n_bins)
    hr = sr.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, opts, cep)
    hs = sr.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, dict(opts or {}, whole_frames=1), cep, reflected=False)
    return hr, hs


def _equal_to_the_sibling(shape, a, V, frames, modes, conds, cep=None):
    Nw, N, H = shape[:3]
    for T in frames:
        p, vp, Tk = sr.reflected_batch(a, V, Nw, H, T)
        assert Tk.tolist() == np.minimum((V.astype(np.int64) + H // 2) // H, T).tolist()
        for mode in modes:
            for opts in conds if T == 37 else conds[:1]:
                hr, hs = _pair(shape, mode, opts, cep)
                assert sr.kernel(hr) == ("clx_k_mel_qr" if cep else "clx_k_mel_fr")
                assert sr.kernel(hs) == ("clx_k_mel_q" if cep else "clx_k_mel_f" if opts else "clx_k_mel")
                want, vf_s = _run(hs, p, vp, T, sm.TC, tables=True)
                want = want.copy()
                assert np.array_equal(vf_s, Tk)                 # (the sibling counts the frames the test gave it)
                assert np.all(np.isfinite(want)) and (Nw == 1 or np.any(want != 0))
                for layout in LAYOUTS:
                    got, vf = _run(hr, a, V, T, layout, tables=True)
                    assert np.array_equal(vf, Tk), (T, vf, Tk)
                    for k in range(len(V)):
                        assert np.all(got[k, Tk[k]:].view(np.uint32) == 0), (T, k)      # dead frames are +0.0 in every row
                    assert _same(got, want), (shape, T, mode, layout, opts, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:3])
                sr.destroy(hr)
                sr.destroy(hs)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_reflected_fbank_is_the_whole_frame_spec_on_the_reflected_samples(shape):
    """clx_k_mel_fr against clx_k_mel_f (conditioned) and clx_k_mel (not), 1, 33, 37 and three more frames than the longest window
    has, both layouts, ln and power, on 16-bit audio; windows shorter than Nw / 2 - H / 2 need more than one fold, a window of one
    sample makes every tap sample 0."""
    Nw, N, H, n_mels, n_bins = shape
    a, V = batch(Nw, H, seed=7 * Nw + H)
    _equal_to_the_sibling(shape, a, V, frame_counts(Nw, H), MODES, (COND, None))


def test_the_equality_holds_on_float_noise():
    """A cell's order of sums depends on the tap number alone, so the words are equal on any float input."""
    shape = SHAPES[0]
    a, V = batch(shape[0], shape[2], seed=99, noise=True)
    _equal_to_the_sibling(shape, a, V, (37,), (sm.LN,), (COND, None))
    _equal_to_the_sibling(CEPS[0], a, V, (37,), (sm.LN,), (COND,), dict(n_ceps=13, dct=_tables(13, 23)[0], lifter=_tables(13, 23)[1], energy=1, energy_scale=SCALE))


@pytest.mark.parametrize("shape", CEPS)
def test_the_reflected_cepstrum_is_the_whole_frame_cepstral_spec_on_the_reflected_samples(shape):
    """clx_k_mel_qr against clx_k_mel_q, the energy row included (it is taken over the mapped, mean-removed frame), and without."""
    Nw, N, H, n_mels, n_bins, n_ceps = shape
    D, lift = _tables(n_ceps, n_mels)
    a, V = batch(Nw, H, seed=n_mels)
    frames = frame_counts(Nw, H) if n_mels < 100 else (33, 37)
    _equal_to_the_sibling(shape, a, V, frames, MODES, (COND, None), dict(n_ceps=n_ceps, dct=D, lifter=lift, energy=1, energy_scale=SCALE))
    _equal_to_the_sibling(shape, a, V, (37,), (sm.LN,), (COND,), dict(n_ceps=n_ceps, dct=D))


@pytest.mark.parametrize("shape", SHAPES[:5])
def test_the_count_rule(shape):
    """valid_frames is min(n_frames, (V + H / 2) / H) from the library's table and from MelSpec.valid_frames; window_len is
    n_frames * hop; no condition ties window_len to n_frames."""
    Nw, N, H, n_mels, n_bins = shape
    V = np.concatenate([valids(Nw, H), np.arange(0, 3 * H + 2, max(H // 20, 1), dtype=np.uint32)])
    L = int(V.max())
    a = np.zeros((len(V), max(L, 1)), dtype=np.float32)
    hr, hs = _pair(shape, sm.POWER, None)
    spec = cx.MelSpec.framed(None, 16000, N, Nw, H, _window(Nw), _fb(N, n_mels, n_bins), mode="power", reflect_edges=True)
    assert spec.reflect_edges and not spec.whole_frames and sr.origin(hr) == H // 2 - Nw // 2
    for T in (1, 2, 40):
        rule = [min(T, (int(v) + H // 2) // H) for v in V]
        assert spec.valid_frames(V, T).tolist() == rule and spec.window_len(T) == T * H
        out = np.zeros((len(V), T, n_mels), dtype=np.float32)
        assert sr.mel_windows(hr, a, V, T, sm.TC, out, shape=(len(V), L), tables=True)[1].tolist() == rule
    assert spec.window_len(0) == 0 and spec.valid_frames([0, H - H // 2 - 1, H - H // 2], 5).tolist() == [0, 0, 1]
    with pytest.raises(cx.ClaxonError, match="valid\\[k\\] is larger than window_len"):
        sr.mel_windows(hr, a, V, 3, sm.TC, np.zeros((len(V), 3, n_mels), dtype=np.float32), shape=(len(V), L - 1))
    if (2 - 1) * H + Nw > 1:                                   # the sibling needs the frames inside window_len, the reflected spec does not
        one = np.ones((1, 1), dtype=np.float32)
        with pytest.raises(cx.ClaxonError, match="window_len is less than"):
            sr.mel_windows(hs, one, [1], 2, sm.TC, np.zeros((1, 2, n_mels), dtype=np.float32))
        sr.mel_windows(hr, one, [1], 2, sm.TC, np.zeros((1, 2, n_mels), dtype=np.float32))
    sr.destroy(hr)
    sr.destroy(hs)


@pytest.mark.parametrize("shape", (SHAPES[0], SHAPES[2], SHAPES[3], CEPS[0]))
def test_no_float_outside_the_valid_samples_is_read(shape):
    """NaN in every float from valid[k] on, the batch flush against an inaccessible page at its end and, again, at its start: nothing
    faults, no NaN appears, dead frames are +0.0, and the words are those of the unguarded run."""
    Nw, N, H, n_mels, n_bins = shape[:5]
    cep = None
    if len(shape) == 6:
        D, lift = _tables(shape[5], n_mels)
        cep = dict(n_ceps=shape[5], dct=D, lifter=lift, energy=1, energy_scale=SCALE)
    a, V = batch(Nw, H, seed=3)
    V[-1], a[-1] = a.shape[1], _pcm((a.shape[1],), 4)         # (the last window reaches the batch's last float,
    V[0], a[0] = a.shape[1], _pcm((a.shape[1],), 5)           # the first window's first float is live,
    V[1], a[1] = 0, np.nan                                    # and a window of no sample comes second)
    hr, hs = _pair(shape, sm.LN, COND, cep)
    T = 37
    Tk = sr.count(V, H, T)
    plain = _run(hr, a, V, T, sm.CT).copy()
    for at_end in (True, False):
        for layout in LAYOUTS:
            got = _run(hr, a, V, T, layout, guarded=at_end)
            assert not np.any(np.isnan(got))
            for k in range(len(V)):
                assert np.all(got[k, Tk[k]:].view(np.uint32) == 0)
            assert _same(got, plain)
    sr.destroy(hr)
    sr.destroy(hs)


@pytest.mark.parametrize("cepstral", (False, True))
def test_the_direct_and_the_mapped_path_agree(cepstral):
    """Group 1 of a long window lies wholly inside [0, V) and is addressed directly.  A short window of 32 frames holds the samples
    from 32 hops on of the long one, and the long one is made, around them, the reflected continuation of the short one as far as
    group 1 reads: frames 32 .. 63 of the long window are then frames 0 .. 31 of the short one, whose group touches both of its
    edges and goes through the index map.  The words must be equal."""
    shape = CEPS[0] if cepstral else SHAPES[0]
    Nw, N, H, n_mels, n_bins = shape[:5]
    cep = dict(n_ceps=13, dct=_tables(13, 23)[0], lifter=_tables(13, 23)[1], energy=1, energy_scale=SCALE) if cepstral else None
    org = H // 2 - Nw // 2
    V = 70 * H
    long = _pcm((1, V), 21)
    # the samples that group 1's frames (32 .. 63) read, placed as group 0 of a window of its own: i' = i - 32 H
    lo, hi = 32 * H + org, 63 * H + org + Nw
    assert 0 <= lo and hi <= V
    # frames 0 .. 31 of the short window read [org, 31 H + org + Nw) of it; give it exactly the samples that lie inside, then the
    # rest by continuing `long` with what reflection would produce: p[j] for j < 0 is p[-j - 1]
    n_short = 32 * H - H // 2                                 # (V' + H / 2) / H = 32 live frames
    assert 31 * H + org + Nw > n_short                        # the last frames reach past the short window's end
    short = np.zeros((1, n_short), dtype=np.float32)
    short[0] = long[0, 32 * H:32 * H + n_short]
    # make `long` the reflected continuation of `short` on both sides, as far as group 1's frames read
    for i in range(lo, 32 * H):
        long[0, i] = short[0, 32 * H - 1 - i]
    for i in range(32 * H + n_short, hi):
        long[0, i] = short[0, 2 * n_short - 1 - (i - 32 * H)]
    for mode in MODES:
        hr, hs = _pair(shape, mode, COND, cep)
        inner = _run(hr, long, [V], 64, sm.TC)[0, 32:64].copy()
        edge = _run(hr, short, [n_short], 32, sm.TC)[0]
        assert np.any(inner != 0) and _same(inner, edge), mode
        sr.destroy(hr)
        sr.destroy(hs)


def test_refusals_by_their_texts():
    Nw, N, H, n_mels, n_bins = SHAPES[1]
    w, fb = _window(Nw), _fb(N, n_mels, n_bins)
    D, lift = _tables(3, n_mels)
    ok_cep = dict(n_ceps=3, dct=D, lifter=lift)

    def refused(text, n_fft=N, win=Nw, hop=H, window=w, fbank=fb, bins=n_bins, mels=n_mels, mode=sm.LN, floor=EPS, opts=None, cep=None):
        with pytest.raises(cx.ClaxonError) as e:
            sr.create(n_fft, win, hop, window, fbank, bins, mels, mode, floor, opts, cep)
        assert text in str(e.value), (text, str(e.value))

    refused("clx_mel_create_reflected: whole_frames must be 0", opts=dict(whole_frames=1))
    refused("clx_mel_create_reflected: whole_frames must be 0", opts=dict(whole_frames=1), cep=ok_cep)
    # every refusal of clx_mel_create_framed
    refused("n_fft must be 2..2048", n_fft=1, win=1)
    refused("n_fft must be 2..2048", n_fft=2049)
    refused("win_length must be 1..n_fft", win=0)
    refused("win_length must be 1..n_fft", win=N + 1)
    refused("n_bins must be 1..n_fft / 2 + 1", bins=0)
    refused("n_bins must be 1..n_fft / 2 + 1", bins=N // 2 + 2)
    refused("hop must be at least 1", hop=0)
    refused("n_mels must be 1..256", mels=0)
    refused("n_mels must be 1..256", mels=257)
    refused("mode must be", mode=3)
    refused("floor must be greater than 0", floor=0.0)
    refused("null argument", window=None)
    refused("null argument", fbank=None)
    refused("remove_dc must be 0 or 1", opts=dict(remove_dc=2))
    refused("whole_frames must be 0 or 1", opts=dict(whole_frames=2))
    refused("preemph must be finite and in 0..1", opts=dict(preemph=1.5))
    refused("preemph must be finite and in 0..1", opts=dict(preemph=float("nan")))
    # every refusal of clx_mel_create_cepstral (but a null cep, which is an fbank spec here)
    big = np.zeros((129, n_bins), dtype=np.float32)
    refused("at most 128 bands", fbank=big, mels=129, cep=dict(n_ceps=3, dct=np.zeros((3, 129), dtype=np.float32)))
    refused("at most 256 bins", n_fft=1024, win=600, window=_window(600), fbank=np.zeros((n_mels, 512), dtype=np.float32), bins=512, cep=ok_cep)
    refused("n_ceps must be 1..n_mels", cep=dict(ok_cep, n_ceps=0))
    refused("n_ceps must be 1..n_mels", cep=dict(ok_cep, n_ceps=n_mels + 1))
    refused("null dct", cep=dict(n_ceps=3))
    refused("energy must be 0 or 1", cep=dict(ok_cep, energy=2))
    refused("energy_scale must be finite and greater than 0", cep=dict(ok_cep, energy_scale=0.0))
    refused("energy_floor must be finite and not negative", cep=dict(ok_cep, energy_floor=-1.0))
    h = sr.create(N, Nw, H, w, fb, n_bins, n_mels, sm.LN, EPS, None, None)      # opts == NULL: all zero
    assert sr.kernel(h) == "clx_k_mel_fr"
    sr.destroy(h)
    # the Python side
    with pytest.raises(ValueError, match="reflect_edges=True cannot be combined with whole_frames=True"):
        cx.MelSpec.framed(None, 16000, N, Nw, H, w, fb, whole_frames=True, reflect_edges=True)
    with pytest.raises(ValueError, match="reflect_edges must be True or False"):
        cx.MelSpec.framed(None, 16000, N, Nw, H, w, fb, reflect_edges=1)
    with pytest.raises(ValueError, match="MelSpec.kaldi: snip_edges=False is not supported"):
        cx.MelSpec.kaldi(None, snip_edges=False)
    with pytest.raises(ValueError, match="MelSpec.mfcc: snip_edges=False is not supported"):
        cx.MelSpec.mfcc(None, snip_edges=False)
    for make, who, names in ((cx.MelSpec.kaldi_reflected, "MelSpec.kaldi_reflected", dict(dither=1.0, vtln_warp=1.1, htk_compat=True, use_energy=True, snip_edges=True)),
                             (cx.MelSpec.mfcc_reflected, "MelSpec.mfcc_reflected", dict(dither=1.0, vtln_warp=1.1, htk_compat=True, raw_energy=False, snip_edges=True))):
        for name, v in names.items():
            with pytest.raises(ValueError, match="%s: %s=%r is not supported" % (who, name, v)):
                make(None, **{name: v})
        with pytest.raises(TypeError, match="%s: unknown argument" % who):
            make(None, bogus=1)
        assert make(None, snip_edges=False).reflect_edges


def test_the_reflected_constructors_have_their_siblings_tables():
    """Word for word in Python, and through the builder: the reflected spec's basis, bank, ends, dct and lifter are the sibling's."""
    for refl, snip, kw in ((cx.MelSpec.kaldi_reflected, cx.MelSpec.kaldi, {}), (cx.MelSpec.kaldi_reflected, cx.MelSpec.kaldi, dict(n_mels=40, sample_rate=8000)),
                           (cx.MelSpec.mfcc_reflected, cx.MelSpec.mfcc, {}), (cx.MelSpec.mfcc_reflected, cx.MelSpec.mfcc, dict(use_energy=True, n_ceps=20, n_mels=40))):
        r, s = refl(None, **kw), snip(None, **kw)
        assert r.reflect_edges and not r.whole_frames and s.whole_frames and not s.reflect_edges
        for name in ("sample_rate", "n_fft", "win_length", "hop", "n_mels", "n_bins", "mode", "floor", "remove_dc", "preemph", "n_ceps", "n_out", "energy",
                     "energy_scale", "energy_floor"):
            assert getattr(r, name) == getattr(s, name), name
        for name in ("window", "fbank", "dct", "lifter"):
            x, y = getattr(r, name), getattr(s, name)
            assert (x is None and y is None) or (x.dtype == np.float32 and _same(x, y)), name
        cep = None if r.n_ceps is None else dict(n_ceps=r.n_ceps, dct=r.dct, lifter=r.lifter, energy=int(r.energy), energy_scale=r.energy_scale)
        args = (r.n_fft, r.win_length, r.hop, r.window, r.fbank, r.n_bins, r.n_mels, sm.LN, r.floor)
        hr = sr.create(*args, dict(remove_dc=1, preemph=r.preemph), cep)
        hs = sr.create(*args, dict(remove_dc=1, preemph=r.preemph, whole_frames=1), cep, reflected=False)
        assert np.array_equal(sr.table_words(hr), sr.table_words(hs))
        sr.destroy(hr)
        sr.destroy(hs)
    assert not cx.MelSpec(None, 16000).reflect_edges and not cx.MelSpec.whisper(None).reflect_edges
