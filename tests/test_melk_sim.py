"""Framed mel specs -- Kaldi's fbank -- under the wave simulator (clx_mel.hip: clx_mel_build_framed, clx_mel_check, clx_mel_fill with
the whole-frame rule, clx_k_mel and clx_k_mel_f).  Three plain equalities hold a framed spec without conditioning, word for word, to
clx_mel_create's spec; the conditioning is held, word for word, to the unconditioned framed spec fed one frame per window that numpy
conditioned in float32 (16-bit audio: the frame sums are exact in any order, and a cell's order of sums does not depend on the
frame's place in its group); general float input is held to the float64 reference under the derived bound of claxon_hip.h.  The
batch sits between NaNs, and in the guarded runs next to inaccessible pages; the output starts as a NaN pattern with a guard word
behind it."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_mel as sm
import simlib_melc as sc
import simlib_melk as sk

NAN_FILL = 0x7fc0dead
GUARD = 0xffc0beef
SR = 16000
FLOOR = 1e-10
# (Nw, N, H, n_mels, n_bins): Kaldi's standard frame; a small one; H > Nw with every bin; the smallest of everything; two passes
SHAPES = ((400, 512, 160, 80, 256), (25, 32, 10, 5, 16), (7, 16, 40, 3, 9), (1, 2, 1, 1, 1), (600, 1024, 200, 40, 512))
FRAMES = (1, 33, 37)
LAYOUTS = (sm.CT, sm.TC)
MODES = (sm.POWER, sm.LN, sm.LOG10)
CONDS = ((1, 0.0), (0, 0.97), (1, 0.97))                      # (remove_dc, preemph)
PRE = float(np.float32(0.97))


def _window(Nw):
    """The povey window in the int16 range (a rectangular one for a single point)."""
    return (sk.kaldi_window("povey" if Nw > 1 else "rectangular", Nw) * 32768.0).astype(np.float32)


def _bank(N, n_mels, n_bins):
    """Kaldi's bank where the shape leaves the Nyquist bin out, HTK triangles over every bin, a single weight for a single bin."""
    if n_bins == N // 2 and n_bins > 1:
        return sk.kaldi_fbank(SR, N, n_mels).astype(np.float32)
    if n_bins == N // 2 + 1:
        return sm.triangles(SR, N, n_mels)
    return np.full((n_mels, n_bins), 0.75, dtype=np.float32)


def _pcm(shape, Nw, seed):
    """16-bit audio as FLAC decodes it: the 2^-15 grid, |x| < 1 (|x| < 0.5 for frames of more than 512 samples), so that a frame's
    sum is exact in float32 in any order."""
    top = 32767 if Nw <= 512 else 16383
    return (np.random.default_rng(seed).integers(-top, top + 1, size=shape).astype(np.float64) / 32768.0).astype(np.float32)


def _run(mod, h, a, valid, T, n_mels, layout, guarded=None, tables=False):
    """One call through simlib_mel, simlib_melc or simlib_melk; the output as [B, T, n_mels] (a view), after the guard word's check."""
    B = a.shape[0]
    n = B * n_mels * T
    raw = np.full(n + 8, NAN_FILL, dtype=np.uint32)
    buf = raw[3:3 + n + 1]
    buf[n] = GUARD
    extra = None
    if guarded is None:
        src = np.full(a.size + 16, np.nan, dtype=np.float32)   # the batch between NaNs, at an odd 4-byte alignment
        src[7:7 + a.size] = a.reshape(-1)
        res = mod.mel_windows(h, src[7:7 + a.size].reshape(a.shape), valid, T, layout, buf, **(dict(tables=True) if tables else {}))
        if tables:
            extra = res[1]
    else:
        mod.mel_guarded(h, a, valid, T, layout, guarded, buf)
    assert buf[n] == GUARD and np.all(raw[:3] == NAN_FILL), "a word outside the output was written"
    out = buf[:n].view(np.float32)
    out = out.reshape(B, n_mels, T).transpose(0, 2, 1) if layout == sm.CT else out.reshape(B, T, n_mels)
    return (out, extra) if tables else out


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins", SHAPES)
def test_plain_equalities(Nw, N, H, n_mels, n_bins):
    """(i) zero options, Nw == N, all bins: clx_mel_create's tables and words.  (ii) Nw < N: the plain spec whose window is
    zero-padded to N, power mode, on a batch long enough for both.  (iii) n_bins < N/2+1: the plain spec whose bank has zero
    columns from n_bins on.  None of the three framed specs conditions, so clx_k_mel runs them."""
    J = N // 2 + 1
    wN, fbJ = sm.hann(N), sm.triangles(SR, N, n_mels)
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    wpad = np.concatenate([w, np.zeros(N - Nw, np.float32)])
    fbz = np.concatenate([fb, np.zeros((n_mels, J - n_bins), np.float32)], axis=1)
    for T in FRAMES:
        L = (T - 1) * H + N
        a = np.random.default_rng(Nw + T).uniform(-1.0, 1.0, size=(3, L)).astype(np.float32)
        valid = np.array([0, min(Nw + H, L), L], dtype=np.uint32)
        for k, v in enumerate(valid):
            a[k, v:] = 0.0
        for mode in MODES if T == 37 else (sm.POWER,):        # (the log modes on two frame groups only: the simulator is slow)
            specs = [(sm.create(N, H, wN, fbJ, n_mels, mode, FLOOR), sk.create(N, N, H, wN, fbJ, J, n_mels, mode, FLOOR, {})),
                     (sm.create(N, H, wN, fbJ, n_mels, mode, FLOOR), sk.create(N, N, H, wN, fbJ, J, n_mels, mode, FLOOR, None)),
                     (sm.create(N, H, wN, fb if n_bins == J else fbz, n_mels, mode, FLOOR), sk.create(N, N, H, wN, fb, n_bins, n_mels, mode, FLOOR))]
            if mode == sm.POWER:
                specs.append((sm.create(N, H, wpad, fbJ, n_mels, mode, FLOOR), sk.create(N, Nw, H, w, fbJ, J, n_mels, mode, FLOOR)))
            for i, (hp, hf) in enumerate(specs):
                assert sk.kernel(hf) == "clx_k_mel"
                if i < 2 and T == 1:
                    plain = sc.create(N, H, wN, fbJ, n_mels, mode, FLOOR)
                    assert np.array_equal(sk.table_words(hf), sc.table_words(plain)), "the tables differ from clx_mel_create's"
                    sc.destroy(plain)
                for layout in LAYOUTS if mode == sm.POWER else (sm.CT,):
                    got, vf = _run(sk, hf, a, valid, T, n_mels, layout, tables=True)
                    assert np.array_equal(vf, sm.valid_frames(valid, H, T))
                    assert _same(got, _run(sm, hp, a, valid, T, n_mels, layout)), (i, T, mode, layout)
                sm.destroy(hp)
                sk.destroy(hf)


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins", SHAPES)
def test_conditioning_is_float32_numpy_in_front_of_the_unconditioned_spec(Nw, N, H, n_mels, n_bins):
    """remove_dc alone, preemph alone and both, on 16-bit audio: the same words as the unconditioned framed spec (clx_k_mel) on a
    batch of single frames that numpy conditioned in float32.  1, 33 and 37 frames, both layouts, three modes; the second window
    has dead frames under the whole-frame rule."""
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    for T in FRAMES:
        L = (T - 1) * H + Nw
        a = _pcm((2, L), Nw, seed=7 * Nw + T)
        valid = np.array([L, max(L - H - 1, 0)], dtype=np.uint32)
        a[1, valid[1]:] = 0.0
        vf = sk.valid_frames(valid, Nw, H, T, whole=True)
        assert vf[0] == T and (T == 1 or 0 < vf[1] < T)
        X = sk.frames_of(a, Nw, H, T)                         # [2, T, Nw]
        for dc, c in CONDS:
            Y = sk.condition32(X, dc, np.float32(c)).reshape(2 * T, Nw)
            h0 = sk.create(N, Nw, H, w, fb, n_bins, n_mels, sm.POWER, FLOOR)
            assert sk.kernel(h0) == "clx_k_mel"
            power = _run(sk, h0, Y, np.full(2 * T, Nw, np.uint32), 1, n_mels, sm.TC).reshape(2, T, n_mels).copy()
            sk.destroy(h0)
            for mode in MODES if T == 37 else (sm.POWER,):    # (the modes differ in the last step only: M is bitwise the same in all)
                hf = sk.create(N, Nw, H, w, fb, n_bins, n_mels, mode, FLOOR, dict(remove_dc=dc, preemph=c, whole_frames=1))
                assert sk.kernel(hf) == "clx_k_mel_f"
                want = sm.finish(mode, FLOOR, power).reshape(power.shape)
                for k in range(2):
                    want[k, vf[k]:] = 0.0
                for layout in LAYOUTS if mode == sm.POWER else (sm.TC,):
                    got, vf_lib = _run(sk, hf, a, valid, T, n_mels, layout, tables=True)
                    assert np.array_equal(vf_lib, vf)
                    assert _same(got, want), (dc, c, T, mode, layout)
                sk.destroy(hf)


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins", SHAPES)
def test_general_input_is_within_the_bound(Nw, N, H, n_mels, n_bins):
    """Uniform noise in [-1, 1) and the same noise times 0.1 plus 0.05 (a large mean): |M - M64| <= dM per live cell, 37 frames, power
    mode, every conditioning.  For Kaldi's standard shape the bound is also held to be tight -- dM <= 0.25 M64 in at least 99 % of
    the cells, median of dM / M64 at most 1e-2 (evaluated in float64: 99.9 %, 2.9e-3 .. 3.3e-3) -- so that it cannot go vacuous.  The
    small shapes are not held to that: with one or seven taps a frame without its mean is next to nothing and M64 is near zero."""
    T, L = 37, 36 * H + Nw
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    noise = np.random.default_rng(Nw).uniform(-1.0, 1.0, size=(2, L)).astype(np.float32)
    for name, a in (("noise", noise), ("offset", (noise * np.float32(0.1) + np.float32(0.05)).astype(np.float32))):
        for dc, c in CONDS:
            hf = sk.create(N, Nw, H, w, fb, n_bins, n_mels, sm.POWER, FLOOR, dict(remove_dc=dc, preemph=c))
            got = _run(sk, hf, a, [L, L], T, n_mels, sm.CT).astype(np.float64)
            sk.destroy(hf)
            M64, dM = sk.reference(a, w, fb, N, H, T, dc, c)
            err = np.abs(got - M64)
            live = M64 > 0
            ratio = dM[live] / M64[live]
            print("%s dc %d c %.2f: worst error / bound %.3g, dM <= 0.25 M64 in %.2f %%, median dM / M64 %.3g"
                  % (name, dc, c, float((err[dM > 0] / dM[dM > 0]).max()) if np.any(dM > 0) else 0.0,
                     100.0 * float(np.mean(ratio <= 0.25)) if ratio.size else 100.0, float(np.median(ratio)) if ratio.size else 0.0))
            assert np.all(err <= dM), (name, dc, c, float((err - dM).max()))
            if (Nw, N) == (400, 512) and dc and c:
                assert np.mean(ratio <= 0.25) >= 0.99 and np.median(ratio) <= 1e-2


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins", SHAPES)
def test_validity_rules_and_dead_frames(Nw, N, H, n_mels, n_bins):
    """valid of 0, Nw-1, Nw, Nw+H-1, Nw+H and L under both rules, 1, 33 and 37 frames: valid_frames by the formula, dead frames +0.0
    in every mode and layout, live frames the words of the same frames with everything valid.  The floats that lie in no live frame
    are NaN: none of them is read."""
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    for T in FRAMES:
        L = (T - 1) * H + Nw
        valids = sorted({0, Nw - 1, Nw, Nw + H - 1, Nw + H, L} & set(range(L + 1)))
        valid = np.array(valids, dtype=np.uint32)
        a = _pcm((1, L), Nw, seed=T + Nw).repeat(len(valids), axis=0)
        for whole in (0, 1):
            vf = sk.valid_frames(valid, Nw, H, T, whole)
            assert vf[0] == 0 and vf[-1] == T
            b = a.copy()
            for k, v in enumerate(valids):
                b[k, v:] = 0.0
                dead = np.ones(L, dtype=bool)
                for t in range(int(vf[k])):
                    dead[t * H:t * H + Nw] = False
                b[k, dead] = np.nan
            for mode in MODES if T == 37 else (sm.LN,):
                hf = sk.create(N, Nw, H, w, fb, n_bins, n_mels, mode, FLOOR, dict(remove_dc=1, preemph=PRE, whole_frames=whole))
                for layout in LAYOUTS if mode == sm.LN else (sm.CT,):
                    got, vf_lib = _run(sk, hf, b, valid, T, n_mels, layout, tables=True)
                    assert np.array_equal(vf_lib, vf), (whole, T, vf_lib, vf)
                    full = _run(sk, hf, np.where(np.isnan(b), 0, b).astype(np.float32), valid * 0 + L, T, n_mels, layout)
                    for k in range(len(valids)):
                        assert np.all(got[k, vf[k]:].view(np.uint32) == 0), (whole, T, k, mode)
                        assert _same(got[k, :vf[k]], full[k, :vf[k]]), (whole, T, k, mode, layout)
                sk.destroy(hf)


def test_an_empty_band_gives_the_finish_of_zero():
    Nw, N, H, n_mels, n_bins = SHAPES[1]
    w, fb = _window(Nw), _bank(N, n_mels, n_bins).copy()
    fb[1] = 0.0
    T, L = 5, 4 * H + Nw
    a = _pcm((1, L), Nw, seed=3)
    for mode in MODES:
        y0 = sm.finish(mode, FLOOR, [0.0])[0]
        for opts in ({}, dict(remove_dc=1, preemph=PRE)):
            hf = sk.create(N, Nw, H, w, fb, n_bins, n_mels, mode, FLOOR, opts)
            got = _run(sk, hf, a, [L], T, n_mels, sm.CT)
            sk.destroy(hf)
            assert np.all(got[0, :, 1].view(np.uint32) == y0.view(np.uint32)) and np.all(got[0, :, 0] != y0)
    # Kaldi's own bank has such bands once the bands are many: 128 at 512 points
    fbk = cx.mel_fbank_kaldi(SR, 512, 128)
    assert fbk.shape == (128, 256) and not np.all(np.any(fbk != 0, axis=1))
    assert cx.MelSpec.kaldi(None, n_mels=128).n_mels == 128


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins", SHAPES)
def test_loads_stay_inside_the_batch(Nw, N, H, n_mels, n_bins):
    """The batch ends on the last float before an inaccessible page, or begins on the first float behind one: a stray load (the
    pre-emphasis tap in front of a frame's first sample, a tap past win_length) faults."""
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    hf = sk.create(N, Nw, H, w, fb, n_bins, n_mels, sm.POWER, FLOOR, dict(remove_dc=1, preemph=PRE, whole_frames=1))
    for T in (1, 37):
        L = (T - 1) * H + Nw
        a = _pcm((2, L), Nw, seed=T)
        want = _run(sk, hf, a, [L, L], T, n_mels, sm.CT).copy()
        for at_end in (True, False):
            assert _same(_run(sk, hf, a, [L, L], T, n_mels, sm.CT, guarded=at_end), want), (T, at_end)
    sk.destroy(hf)


def test_new_refusals():
    Nw, N, H, n_mels, n_bins = SHAPES[1]
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    ok = dict(n_fft=N, win_length=Nw, hop=H, window=w, fbank=fb, n_bins=n_bins, n_mels=n_mels, mode=sm.LN, floor=FLOOR)
    nan, inf = float("nan"), float("inf")
    for kw, opts, why in ((dict(win_length=0), {}, "clx_mel_create_framed: win_length must be 1..n_fft"),
                          (dict(win_length=N + 1), {}, "clx_mel_create_framed: win_length must be 1..n_fft"),
                          (dict(n_bins=0), {}, "clx_mel_create_framed: n_bins must be 1..n_fft / 2 + 1"),
                          (dict(n_bins=N // 2 + 2), {}, "clx_mel_create_framed: n_bins must be 1..n_fft / 2 + 1"),
                          ({}, dict(remove_dc=2), "clx_mel_create_framed: remove_dc must be 0 or 1"),
                          ({}, dict(whole_frames=2), "clx_mel_create_framed: whole_frames must be 0 or 1"),
                          ({}, dict(preemph=-0.5), "clx_mel_create_framed: preemph must be finite and in 0..1"),
                          ({}, dict(preemph=1.5), "clx_mel_create_framed: preemph must be finite and in 0..1"),
                          ({}, dict(preemph=nan), "clx_mel_create_framed: preemph must be finite and in 0..1"),
                          ({}, dict(preemph=inf), "clx_mel_create_framed: preemph must be finite and in 0..1"),
                          (dict(n_fft=1), {}, "n_fft must be 2..2048"), (dict(n_fft=2049), {}, "n_fft must be 2..2048"),
                          (dict(hop=0), {}, "hop must be at least 1"), (dict(n_mels=0), {}, "n_mels must be 1..256"),
                          (dict(mode=3), {}, "mode must be CLX_MEL_POWER, CLX_MEL_LN or CLX_MEL_LOG10"),
                          (dict(floor=0.0), {}, "floor must be greater than 0 in a log mode"),
                          (dict(window=None), {}, "null argument"), (dict(fbank=None), {}, "null argument")):
        with pytest.raises(cx.ClaxonError) as e:
            sk.create(**dict(ok, **kw), opts=opts)
        assert e.value.status == cx.API_ERROR and why in e.value.message, (kw, opts, e.value.message)
    sk.destroy(sk.create(**ok, opts=dict(preemph=1.0, remove_dc=1, whole_frames=1)))          # (the ends of the range are inside it)
    sk.destroy(sk.create(**dict(ok, win_length=N, window=_window(N)), opts=dict(preemph=0.0)))
    # the length condition is win_length's
    T = 9
    h = sk.create(**ok, opts=dict(remove_dc=1))
    out = np.zeros(4 * T * n_mels, dtype=np.float32)
    a = np.zeros((1, (T - 1) * H + Nw), dtype=np.float32)
    sk.mel_windows(h, a, [a.shape[1]], T, sm.CT, out)
    for call, why in ((dict(audio=a[:, :-1].copy(), valid=[1], n_frames=T), "window_len is less than (n_frames - 1) * hop + win_length"),
                      (dict(audio=a, valid=[a.shape[1] + 1], n_frames=T), "valid[k] is larger than window_len"),
                      (dict(audio=a, valid=[1], n_frames=T, layout=2), "layout must be CLX_WINDOW_TC or CLX_WINDOW_CT")):
        with pytest.raises(cx.ClaxonError) as e:
            sk.mel_windows(h, call["audio"], call["valid"], call["n_frames"], call.get("layout", sm.CT), out)
        assert why in e.value.message, (call, e.value.message)
    out[:] = 7.0                                                                               # the empty calls touch nothing
    sk.mel_windows(h, None, [], T, sm.CT, None, shape=(0, 100))
    sk.mel_windows(h, a, [3], 0, sm.CT, out)
    assert np.all(out == 7.0)
    sk.destroy(h)


def test_kaldi_tables_are_the_formulas():
    """mel_fbank_kaldi and the four windows against the formulas in float64, cell by cell; MelSpec.kaldi's shape, rules and refusals."""
    for sr, N, n_mels, lo, hi in ((16000, 512, 80, 20.0, 0.0), (16000, 512, 23, 20.0, -400.0), (8000, 256, 40, 0.0, 3800.0), (16000, 32, 5, 20.0, 0.0)):
        fb = cx.mel_fbank_kaldi(sr, N, n_mels, lo, hi)
        want = sk.kaldi_fbank(sr, N, n_mels, lo, hi)
        assert fb.dtype == np.float32 and fb.shape == (n_mels, N // 2)
        assert np.max(np.abs(fb.astype(np.float64) - want)) <= 2.0 ** -24 and np.array_equal(fb != 0, want.astype(np.float32) != 0)
        assert np.all(fb >= 0) and np.all(fb <= 1) and np.all(fb[:, 0] == 0)
    for kind in cx.KALDI_WINDOWS:
        for Nw, scale in ((400, 32768.0), (25, 1.0), (2, 1.0)):
            w = cx.mel_window_kaldi(kind, Nw, scale)
            assert w.dtype == np.float32 and np.array_equal(w, (sk.kaldi_window(kind, Nw) * scale).astype(np.float32)), (kind, Nw)
    assert np.array_equal(cx.mel_window_kaldi("rectangular", 1), np.ones(1, np.float32))
    with pytest.raises(ValueError, match="window_type"):
        cx.mel_window_kaldi("blackman", 400)
    with pytest.raises(ValueError, match="low_freq"):
        cx.mel_fbank_kaldi(16000, 512, 80, 20.0, 9000.0)
    s = cx.MelSpec.kaldi(None)
    assert (s.sample_rate, s.n_fft, s.win_length, s.hop, s.n_mels, s.n_bins) == (16000, 512, 400, 160, 80, 256)
    assert (s.mode, s.remove_dc, s.whole_frames, s.center, s.top) == ("ln", True, True, False, None)
    assert np.float32(s.floor) == np.finfo(np.float32).eps and np.float32(s.preemph) == np.float32(0.97)
    assert np.array_equal(s.window, (sk.kaldi_window("povey", 400) * 32768.0).astype(np.float32))
    assert np.array_equal(s.fbank, cx.mel_fbank_kaldi(16000, 512, 80))
    assert s.window_len(0) == 0 and s.window_len(1) == 400 and s.window_len(98) == 97 * 160 + 400
    assert list(s.valid_frames([0, 399, 400, 559, 560, 10 ** 6], 98)) == [0, 0, 1, 1, 2, 98]
    assert list(sk.valid_frames([0, 399, 400, 559, 560, 10 ** 6], 400, 160, 98, True)) == [0, 0, 1, 1, 2, 98]
    s8 = cx.MelSpec.kaldi(None, sample_rate=8000, n_mels=23, window_type="hamming", remove_dc_offset=False, preemphasis=0.0, scale=1.0)
    assert (s8.n_fft, s8.win_length, s8.hop, s8.n_bins, s8.remove_dc, s8.preemph) == (256, 200, 80, 128, False, 0.0)
    assert cx.MelSpec.kaldi(None, dither=0.0, snip_edges=True, use_energy=False, vtln_warp=1.0, htk_compat=False).n_fft == 512
    for kw, err, text in ((dict(dither=1.0), ValueError, "dither"), (dict(use_energy=True), ValueError, "use_energy"),
                          (dict(snip_edges=False), ValueError, "snip_edges"), (dict(vtln_warp=1.1), ValueError, "vtln_warp"),
                          (dict(htk_compat=True), ValueError, "htk_compat"), (dict(subtract_mean=True), TypeError, "subtract_mean"),
                          (dict(frame_length_ms=200.0), ValueError, "2..2048"), (dict(window_type="blackman"), ValueError, "window_type"),
                          (dict(scale=0.0), ValueError, "scale"), (dict(preemphasis=1.5), ValueError, "preemph")):
        with pytest.raises(err, match=text):
            cx.MelSpec.kaldi(None, **kw)
    # the plain spec's rules are what they were
    p = cx.MelSpec(None, 16000)
    assert (p.win_length, p.n_bins, p.whole_frames, p.window_len(3)) == (400, 201, False, 720) and list(p.valid_frames([0, 1, 161], 5)) == [0, 1, 2]
    with pytest.raises(ValueError, match="win_length"):
        cx.MelSpec.framed(None, 16000, 512, 513, 160, np.ones(513), np.ones((3, 256)))
    with pytest.raises(ValueError, match="n_bins"):
        cx.MelSpec.framed(None, 16000, 512, 400, 160, np.ones(400), np.ones((3, 258)))
