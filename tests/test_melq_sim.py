"""Cepstral mel specs -- Kaldi's MFCC -- under the wave simulator (clx_mel.hip: clx_mel_build_cepstral, clx_mel_check, clx_mel_fill and
clx_k_mel_q).  The cepstrum is held, word for word, to the definition's chain of the host libm's fmaf over the output of the framed
spec with the same tables (clx_k_mel_f or clx_k_mel), then the lifter product in numpy float32: that ties the log-mel cells to the
framed spec's words and fixes the order of the sums.  The energy row is held to the logarithm of the exact integer energy where every
sum is exact, and of the energy emulated in the stated lane order otherwise, within LOG_ULPS.  The batch sits between NaNs, and in
the guarded runs next to inaccessible pages; the output starts as a NaN pattern with a guard word behind it."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_mel as sm
import simlib_melk as sk
import simlib_melq as sq

NAN_FILL = 0x7fc0dead
GUARD = 0xffc0beef
SR = 16000
EPS = float(np.finfo(np.float32).eps)
# (Nw, N, H, n_mels, n_bins, n_ceps): Kaldi's defaults; n_ceps == n_mels; H > Nw with one coefficient; the register cap
SHAPES = ((400, 512, 160, 23, 256, 13), (25, 32, 10, 5, 16, 5), (7, 16, 40, 3, 9, 1), (400, 512, 160, 128, 256, 40))
FRAMES = (1, 33, 37)
LAYOUTS = (sm.CT, sm.TC)
MODES = (sm.LN, sm.POWER)
PRE = float(np.float32(0.97))
COND = dict(remove_dc=1, preemph=PRE, whole_frames=1)


def _window(Nw):
    return (sk.kaldi_window("povey", Nw) * 32768.0).astype(np.float32)


def _bank(N, n_mels, n_bins):
    """Kaldi's bank where the shape leaves the Nyquist bin out (with 128 bands the lowest are empty), HTK triangles over every bin."""
    return sk.kaldi_fbank(SR, N, n_mels).astype(np.float32) if n_bins == N // 2 else sm.triangles(SR, N, n_mels)


def _tables(n_ceps, n_mels):
    return sq.dct_kaldi(n_ceps, n_mels).astype(np.float32), sq.lifter_kaldi(n_ceps).astype(np.float32)


def _pcm(shape, seed, top=32767):
    """16-bit audio as FLAC decodes it: the 2^-15 grid."""
    return (np.random.default_rng(seed).integers(-top, top + 1, size=shape).astype(np.float64) / 32768.0).astype(np.float32)


def _run(h, a, valid, T, layout, guarded=None, tables=False):
    """One call through simlib_melq; the output as [B, T, rows] (a view), after the guard word's check."""
    B, n_rows = a.shape[0], sq.rows(h)
    n = B * n_rows * T
    raw = np.full(n + 8, NAN_FILL, dtype=np.uint32)
    buf = raw[3:3 + n + 1]
    buf[n] = GUARD
    extra = None
    if guarded is None:
        src = np.full(a.size + 16, np.nan, dtype=np.float32)   # the batch between NaNs, at an odd 4-byte alignment
        src[7:7 + a.size] = a.reshape(-1)
        res = sq.mel_windows(h, src[7:7 + a.size].reshape(a.shape), valid, T, layout, buf, **(dict(tables=True) if tables else {}))
        if tables:
            extra = res[1]
    else:
        sq.mel_guarded(h, a, valid, T, layout, guarded, buf)
    assert buf[n] == GUARD and np.all(raw[:3] == NAN_FILL), "a word outside the output was written"
    assert not np.any(buf[:n] == NAN_FILL), "an output word was not written"
    out = buf[:n].view(np.float32)
    out = out.reshape(B, n_rows, T).transpose(0, 2, 1) if layout == sm.CT else out.reshape(B, T, n_rows)
    return (out, extra) if tables else out


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins,n_ceps", SHAPES)
def test_the_cepstrum_is_the_fmaf_chain_over_the_framed_specs_words(Nw, N, H, n_mels, n_bins, n_ceps):
    """Conditioned (clx_k_mel_f's words) and unconditioned (clx_k_mel's), 1, 33 and 37 frames, both layouts, ln and power; the second
    window has dead frames under the whole-frame rule.  With the energy on, rows 1.. are the same words and row 0 is within LOG_ULPS
    of the logarithm of E emulated in the stated lane order."""
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    D, lift = _tables(n_ceps, n_mels)
    scale = 2.0 ** 30
    for T in FRAMES:
        L = (T - 1) * H + Nw
        a = _pcm((2, L), seed=11 * Nw + T + n_mels)
        valid = np.array([L, max(L - H - 1, 0)], dtype=np.uint32)
        a[1, valid[1]:] = 0.0
        vf = sk.valid_frames(valid, Nw, H, T, whole=True)
        assert vf[0] == T and (T == 1 or 0 < vf[1] < T)
        E = sq.energy32(sk.frames_of(a, Nw, H, T), True, scale)
        le64 = sq.log_energy64(E)
        for mode in MODES:
            for opts in (COND, dict(whole_frames=1)) if T == 37 else (COND,):
                hf = sq.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, opts, sq.FRAMED)
                assert sq.kernel(hf) == ("clx_k_mel_f" if opts is COND else "clx_k_mel") and sq.rows(hf) == n_mels
                Y = _run(hf, a, valid, T, sm.TC).copy()
                sq.destroy(hf)
                want = sq.chain(D, Y, lift)
                for k in range(2):
                    want[k, vf[k]:] = 0.0
                hq = sq.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, opts, dict(n_ceps=n_ceps, dct=D, lifter=lift))
                he = sq.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, opts,
                               dict(n_ceps=n_ceps, dct=D, lifter=lift, energy=1, energy_scale=scale))
                assert sq.kernel(hq) == sq.kernel(he) == "clx_k_mel_q" and sq.rows(hq) == n_ceps
                for layout in LAYOUTS:
                    got, vf_lib = _run(hq, a, valid, T, layout, tables=True)
                    assert np.array_equal(vf_lib, vf)
                    assert _same(got, want), (T, mode, layout, opts)
                    if opts is COND:
                        gote = _run(he, a, valid, T, layout)
                        assert _same(gote[:, :, 1:], want[:, :, 1:]), (T, mode, layout)
                        for k in range(2):
                            assert np.all(gote[k, vf[k]:, 0].view(np.uint32) == 0)
                            ulps = sq.ulps_of(gote[k, :vf[k], 0], le64[k, :vf[k]])
                            assert np.all(ulps <= sm.LOG_ULPS), (T, mode, layout, k, float(ulps.max()))
                sq.destroy(hq)
                sq.destroy(he)


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins,n_ceps", SHAPES)
def test_the_energy_of_small_integers_is_exact(Nw, N, H, n_mels, n_bins, n_ceps):
    """Audio k / 32768 with |k| <= 127, the mean left in, energy_scale 2^30: every square and every sum is an integer below 2^24, so
    E is the integer energy in any order and row 0 lies within LOG_ULPS of its logarithm in float64.  A quiet frame under a floor
    gives logf(energy_floor) exactly as the simulator's libm computes it, a frame of zeros without one logf(FLT_EPSILON)."""
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    D, lift = _tables(n_ceps, n_mels)
    floor = 1000.0
    for T in FRAMES:
        L = (T - 1) * H + Nw
        a = _pcm((2, L), seed=5 * Nw + T, top=127)
        a[1, :Nw] = np.float32(1.0 / 32768.0)                 # frame 0 of window 1: quiet (energy Nw), the rest of window 1 louder
        if T > 1:
            a[0, (T - 1) * H:(T - 1) * H + Nw] = 0.0          # the last frame of window 0: zeros
        X = sk.frames_of(a, Nw, H, T).astype(np.float64) * 32768.0
        exact = (X * X).sum(axis=-1)                          # [2, T] integers
        assert np.array_equal(exact, np.round(exact)) and exact.max() < 2 ** 24 and exact[1, 0] == Nw < floor
        for fl in (0.0, floor):
            he = sq.create(N, Nw, H, w, fb, n_bins, n_mels, sm.LN, EPS, dict(preemph=PRE, whole_frames=1),
                           dict(n_ceps=n_ceps, dct=D, lifter=lift, energy=1, energy_scale=2.0 ** 30, energy_floor=fl))
            for layout in LAYOUTS:
                got = _run(he, a, [L, L], T, layout)[:, :, 0]
                ulps = sq.ulps_of(got, sq.log_energy64(exact, fl))
                assert np.all(ulps <= sm.LOG_ULPS), (T, fl, layout, float(ulps.max()))
                if fl:
                    assert got[1, 0].view(np.uint32) == sq.logf(fl).view(np.uint32) and np.all(got >= sq.logf(fl))
                elif T > 1:
                    assert exact[0, T - 1] == 0 and got[0, T - 1].view(np.uint32) == sq.logf(EPS).view(np.uint32)
            sq.destroy(he)


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins,n_ceps", SHAPES)
def test_no_lifter_is_a_lifter_of_ones_and_an_identity_dct_gives_the_cells_back(Nw, N, H, n_mels, n_bins, n_ceps):
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    D, _ = _tables(n_ceps, n_mels)
    T, L = 37, 36 * H + Nw
    a = _pcm((2, L), seed=Nw + 1)
    valid = [L, L - H]
    for mode in MODES:
        h0 = sq.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, COND, dict(n_ceps=n_ceps, dct=D))
        h1 = sq.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, COND, dict(n_ceps=n_ceps, dct=D, lifter=np.ones(n_ceps, np.float32)))
        hi = sq.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, COND, dict(n_ceps=n_ceps, dct=np.eye(n_ceps, n_mels, dtype=np.float32)))
        hf = sq.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, COND, sq.FRAMED)
        for layout in LAYOUTS:
            assert _same(_run(h0, a, valid, T, layout), _run(h1, a, valid, T, layout)), (mode, layout)
            got, Y = _run(hi, a, valid, T, layout), _run(hf, a, valid, T, layout)[:, :, :n_ceps]
            assert _same(got + np.float32(0.0), Y + np.float32(0.0)), (mode, layout)             # (-0.0 aside)
        for h in (h0, h1, hi, hf):
            sq.destroy(h)


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins,n_ceps", SHAPES)
def test_validity_rules_and_dead_frames(Nw, N, H, n_mels, n_bins, n_ceps):
    """valid of 0, Nw-1, Nw, Nw+H-1, Nw+H and L under both rules, 1, 33 and 37 frames, the energy on: valid_frames by the formula,
    dead frames +0.0 in all n_ceps rows, live frames the words of the same frames with everything valid.  The floats that lie in no
    live frame are NaN: none of them is read, no NaN comes out."""
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    D, lift = _tables(n_ceps, n_mels)
    for T in FRAMES:
        L = (T - 1) * H + Nw
        valids = sorted({0, Nw - 1, Nw, Nw + H - 1, Nw + H, L} & set(range(L + 1)))
        valid = np.array(valids, dtype=np.uint32)
        a = _pcm((1, L), seed=T + Nw).repeat(len(valids), axis=0)
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
                hq = sq.create(N, Nw, H, w, fb, n_bins, n_mels, mode, EPS, dict(remove_dc=1, preemph=PRE, whole_frames=whole),
                               dict(n_ceps=n_ceps, dct=D, lifter=lift, energy=1, energy_scale=2.0 ** 30))
                for layout in LAYOUTS:
                    got, vf_lib = _run(hq, b, valid, T, layout, tables=True)
                    assert np.array_equal(vf_lib, vf), (whole, T, vf_lib, vf)
                    assert not np.any(np.isnan(got))
                    full = _run(hq, np.where(np.isnan(b), 0, b).astype(np.float32), valid * 0 + L, T, layout)
                    for k in range(len(valids)):
                        assert np.all(got[k, vf[k]:].view(np.uint32) == 0), (whole, T, k, mode)
                        assert _same(got[k, :vf[k]], full[k, :vf[k]]), (whole, T, k, mode, layout)
                sq.destroy(hq)


@pytest.mark.parametrize("Nw,N,H,n_mels,n_bins,n_ceps", SHAPES)
def test_loads_stay_inside_the_batch(Nw, N, H, n_mels, n_bins, n_ceps):
    """The batch ends on the last float before an inaccessible page, or begins on the first float behind one: a stray load of the
    energy's pass or of the staging faults."""
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    D, lift = _tables(n_ceps, n_mels)
    for opts in (COND, dict(whole_frames=1)):
        hq = sq.create(N, Nw, H, w, fb, n_bins, n_mels, sm.LN, EPS, opts, dict(n_ceps=n_ceps, dct=D, lifter=lift, energy=1, energy_scale=2.0 ** 30))
        for T in (1, 37):
            L = (T - 1) * H + Nw
            a = _pcm((2, L), seed=T)
            want = _run(hq, a, [L, L], T, sm.CT).copy()
            for at_end in (True, False):
                assert _same(_run(hq, a, [L, L], T, sm.CT, guarded=at_end), want), (T, at_end)
        sq.destroy(hq)


def test_new_refusals():
    Nw, N, H, n_mels, n_bins, n_ceps = SHAPES[1]
    w, fb = _window(Nw), _bank(N, n_mels, n_bins)
    D, lift = _tables(n_ceps, n_mels)
    ok = dict(n_fft=N, win_length=Nw, hop=H, window=w, fbank=fb, n_bins=n_bins, n_mels=n_mels, mode=sm.LN, floor=EPS)
    cep = dict(n_ceps=n_ceps, dct=D, lifter=lift)
    nan, inf = float("nan"), float("inf")
    big = dict(n_fft=1024, win_length=600, window=_window(600))
    for kw, q, why in ((dict(n_mels=129, fbank=np.ones((129, n_bins), np.float32)), dict(cep, dct=np.ones((5, 129), np.float32)),
                        "clx_mel_create_cepstral: a cepstral spec has at most 128 bands"),
                       (dict(big, n_bins=257, fbank=np.ones((n_mels, 257), np.float32)), cep, "clx_mel_create_cepstral: a cepstral spec has at most 256 bins"),
                       ({}, dict(cep, n_ceps=0), "clx_mel_create_cepstral: n_ceps must be 1..n_mels"),
                       ({}, dict(cep, n_ceps=n_mels + 1), "clx_mel_create_cepstral: n_ceps must be 1..n_mels"),
                       ({}, dict(cep, dct=None), "clx_mel_create_cepstral: null dct"),
                       ({}, dict(cep, energy=2), "clx_mel_create_cepstral: energy must be 0 or 1"),
                       ({}, dict(cep, energy_scale=0.0), "clx_mel_create_cepstral: energy_scale must be finite and greater than 0"),
                       ({}, dict(cep, energy_scale=-1.0), "clx_mel_create_cepstral: energy_scale must be finite and greater than 0"),
                       ({}, dict(cep, energy_scale=inf), "clx_mel_create_cepstral: energy_scale must be finite and greater than 0"),
                       ({}, dict(cep, energy_scale=nan), "clx_mel_create_cepstral: energy_scale must be finite and greater than 0"),
                       ({}, dict(cep, energy_floor=-1.0), "clx_mel_create_cepstral: energy_floor must be finite and not negative"),
                       ({}, dict(cep, energy_floor=inf), "clx_mel_create_cepstral: energy_floor must be finite and not negative"),
                       ({}, dict(cep, energy_floor=nan), "clx_mel_create_cepstral: energy_floor must be finite and not negative"),
                       ({}, None, "clx_mel_create_cepstral: null cepstral options"),
                       (dict(win_length=N + 1), cep, "clx_mel_create_framed: win_length must be 1..n_fft"),       # (the framed spec's stay)
                       (dict(window=None), cep, "null argument")):
        with pytest.raises(cx.ClaxonError) as e:
            sq.create(**dict(ok, **kw), opts={}, cep=q)
        assert e.value.status == cx.API_ERROR and why in e.value.message, (kw, q, e.value.message)
    # the ends of the ranges are inside them; NULL frame options are all zero
    sq.destroy(sq.create(**dict(ok, n_mels=128, fbank=np.ones((128, n_bins), np.float32)), opts=None, cep=dict(n_ceps=128, dct=np.ones((128, 128), np.float32))))
    sq.destroy(sq.create(**dict(big, hop=H, n_bins=256, fbank=np.ones((n_mels, 256), np.float32), n_mels=n_mels, mode=sm.LN, floor=EPS), opts={}, cep=cep))
    h = sq.create(**ok, opts=None, cep=dict(cep, energy=1, energy_floor=0.0))
    # clx_mel_windows' refusals are the framed spec's
    T = 9
    out = np.zeros(4 * T * n_ceps, dtype=np.float32)
    a = np.zeros((1, (T - 1) * H + Nw), dtype=np.float32)
    sq.mel_windows(h, a, [a.shape[1]], T, sm.CT, out)
    for call, why in ((dict(audio=a[:, :-1].copy(), valid=[1], n_frames=T), "window_len is less than (n_frames - 1) * hop + win_length"),
                      (dict(audio=a, valid=[a.shape[1] + 1], n_frames=T), "valid[k] is larger than window_len"),
                      (dict(audio=a, valid=[1], n_frames=T, layout=2), "layout must be CLX_WINDOW_TC or CLX_WINDOW_CT")):
        with pytest.raises(cx.ClaxonError) as e:
            sq.mel_windows(h, call["audio"], call["valid"], call["n_frames"], call.get("layout", sm.CT), out)
        assert why in e.value.message, (call, e.value.message)
    out[:] = 7.0                                                                               # the empty calls touch nothing
    sq.mel_windows(h, None, [], T, sm.CT, None, shape=(0, 100))
    sq.mel_windows(h, a, [3], 0, sm.CT, out)
    assert np.all(out == 7.0)
    sq.destroy(h)


def test_python_tables_are_the_formulas():
    """mel_dct and mel_lifter_kaldi against the formulas in float64, cell by cell; MelSpec.mfcc's shape, rules and refusals."""
    for n_ceps, n_mels in ((13, 23), (5, 5), (1, 3), (40, 128), (80, 80)):
        d = cx.mel_dct(n_ceps, n_mels)
        assert d.dtype == np.float32 and d.shape == (n_ceps, n_mels)
        assert np.max(np.abs(d.astype(np.float64) - sq.dct_kaldi(n_ceps, n_mels))) <= 2.0 ** -25        # (half an ulp below 1)
        if n_ceps == n_mels:
            assert np.max(np.abs(d.astype(np.float64) @ d.astype(np.float64).T - np.eye(n_mels))) <= 4.0 * n_mels * 2.0 ** -24
        try:
            from scipy.fft import dct as scipy_dct
        except ImportError:
            scipy_dct = None
        if scipy_dct is not None:
            want = scipy_dct(np.eye(n_mels), type=2, norm="ortho", axis=1).T[:n_ceps]            # row k: basis k
            assert np.max(np.abs(d - want)) <= 2.0 ** -23
    for n_ceps, Q in ((13, 22.0), (5, 22.0), (1, 22.0), (40, 30.5)):
        l = cx.mel_lifter_kaldi(n_ceps, Q)
        assert l.dtype == np.float32 and l.shape == (n_ceps,) and l[0] == 1.0
        assert np.max(np.abs(l - sq.lifter_kaldi(n_ceps, Q))) <= 2.0 ** -24 * 16
    assert cx.mel_lifter_kaldi(13, 0) is None and cx.mel_lifter_kaldi(13, 0.0) is None
    with pytest.raises(ValueError, match="n_ceps"):
        cx.mel_dct(24, 23)
    with pytest.raises(ValueError, match="n_ceps"):
        cx.mel_dct(0, 23)
    s = cx.MelSpec.mfcc(None)
    assert (s.sample_rate, s.n_fft, s.win_length, s.hop, s.n_mels, s.n_bins, s.n_ceps, s.n_out) == (16000, 512, 400, 160, 23, 256, 13, 13)
    assert (s.mode, s.remove_dc, s.whole_frames, s.center, s.top, s.energy, s.energy_floor) == ("ln", True, True, False, None, False, 0.0)
    assert np.float32(s.floor) == np.finfo(np.float32).eps and np.float32(s.preemph) == np.float32(0.97) and s.energy_scale == 2.0 ** 30
    k = cx.MelSpec.kaldi(None, n_mels=23)
    assert np.array_equal(s.window, k.window) and np.array_equal(s.fbank, k.fbank) and k.n_out == k.n_mels == 23 and k.n_ceps is None
    assert np.array_equal(s.dct, cx.mel_dct(13, 23)) and np.array_equal(s.lifter, cx.mel_lifter_kaldi(13, 22.0))
    assert s.window_len(98) == 97 * 160 + 400 and list(s.valid_frames([0, 399, 400, 559, 560, 10 ** 6], 98)) == [0, 0, 1, 1, 2, 98]
    e = cx.MelSpec.mfcc(None, sample_rate=8000, n_ceps=10, n_mels=15, cepstral_lifter=0.0, use_energy=True, energy_floor=1.5, scale=1.0)
    assert (e.n_fft, e.win_length, e.hop, e.n_bins, e.n_out, e.lifter, e.energy, e.energy_scale, e.energy_floor) == (256, 200, 80, 128, 10, None, True, 1.0, 1.5)
    assert cx.MelSpec.mfcc(None, dither=0.0, snip_edges=True, vtln_warp=1.0, htk_compat=False, raw_energy=True).n_out == 13
    for kw, err, text in ((dict(dither=1.0), ValueError, "dither"), (dict(snip_edges=False), ValueError, "snip_edges"),
                          (dict(vtln_warp=1.1), ValueError, "vtln_warp"), (dict(htk_compat=True), ValueError, "htk_compat"),
                          (dict(raw_energy=False), ValueError, "raw_energy"), (dict(subtract_mean=True), TypeError, "subtract_mean"),
                          (dict(n_ceps=24), ValueError, "n_ceps"), (dict(n_mels=129, n_ceps=13), ValueError, "n_mels"),
                          (dict(use_energy=1), ValueError, "use_energy"), (dict(energy_floor=-1.0), ValueError, "energy_floor"),
                          (dict(cepstral_lifter=-1.0), ValueError, "Q"), (dict(scale=0.0), ValueError, "scale")):
        with pytest.raises(err, match=text):
            cx.MelSpec.mfcc(None, **kw)
    # MelSpec.kaldi refuses use_energy as before; a framed spec without a dct is what it was
    with pytest.raises(ValueError, match="use_energy"):
        cx.MelSpec.kaldi(None, use_energy=True)
    f = cx.MelSpec.framed(None, 16000, 512, 400, 160, np.ones(400), np.ones((3, 256)))
    assert f.n_ceps is None and f.n_out == 3 and cx.MelSpec(None, 16000).n_out == 80
    with pytest.raises(ValueError, match="need a dct"):
        cx.MelSpec.framed(None, 16000, 512, 400, 160, np.ones(400), np.ones((3, 256)), energy=True)
    with pytest.raises(ValueError, match="dct must be"):
        cx.MelSpec.framed(None, 16000, 512, 400, 160, np.ones(400), np.ones((3, 256)), dct=np.ones((4, 3)))
    with pytest.raises(ValueError, match="at most 128 bands"):
        cx.MelSpec.framed(None, 16000, 512, 400, 160, np.ones(400), np.ones((129, 256)), dct=np.ones((4, 129)))
