"""Centred frames and per-window range scaling (clx_mel.hip: clx_mel_build with options, clx_mel_check, clx_mel_fill_c, clx_k_mel_c and
clx_k_mel_range) under the wave simulator.  The centred output is held, word for word, to the uncentred kernel on the batch padded
on the host (np.pad, reflect or constant) -- the definition of claxon_hip.h --, the ranged output to numpy float32 maximum, add and
multiply on the unranged output, the padding definition itself to torch.stft(center=True) in float64.  The batch sits between NaNs,
and in the guarded runs next to inaccessible pages; the output starts as a NaN pattern with a guard word behind it."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_mel as sm
import simlib_melc as sc

NAN_FILL = 0x7fc0dead
GUARD = 0xffc0beef
SR = 16000
FLOOR = 1e-10
# (n_fft, hop, n_mels): the workload's shape; P > H (several frames reflect on the left); odd N (2P = N - 1: the frame-count rule);
# H > N; a second pass (the maximum is folded on the last only)
SHAPES = ((400, 160, 80), (50, 7, 5), (51, 7, 5), (16, 40, 3), (600, 200, 40))
FRAMES = (1, 33, 37)
LAYOUTS = (sm.CT, sm.TC)
PADS = (sc.PAD_REFLECT, sc.PAD_ZERO)
RANGES = ((8.0, 4.0, 0.25), (8.0, 0.0, 10.0))


def _tables(N, n_mels):
    return sm.hann(N), sm.triangles(SR, N, n_mels)


def _lengths(N, H, T):
    """The window lengths of a frame count: T * H and the smallest allowed, (T - 1) * H + N - 2P (the deepest right reflection); for
    one frame P + 1, the smallest with P < L (and T * H beside it where that is a legal length)."""
    P = N // 2
    if T == 1:
        return sorted({P + 1} | ({H} if P < H else set()))
    return sorted({T * H, (T - 1) * H + N - 2 * P})


def _cases(N, H):
    """Every (T, L, valid list) of the shape."""
    P = N // 2
    return [(T, L, sorted({0, 1, P, L - 1, L} & set(range(L + 1)))) for T in FRAMES for L in _lengths(N, H, T)]


def _batch(L, valid, seed):
    a = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(len(valid), L)).astype(np.float32)
    for k, v in enumerate(valid):
        a[k, v:] = 0.0
    return a, np.array(valid, dtype=np.uint32)


def _run(mod, h, a, valid, T, n_mels, layout, guarded=None, shift=0, tables=False):
    """One call through simlib_mel or simlib_melc; the output as [B, T, n_mels] (a view), after the guard word's check.  `shift`
    moves the output off the 16-byte grid by that many floats."""
    B = a.shape[0]
    n = B * n_mels * T
    raw = np.full(n + 8, NAN_FILL, dtype=np.uint32)
    off = (-(raw.ctypes.data // 4) % 4 + shift) % 4            # (buf starts `shift` floats behind a 16-byte boundary)
    buf = raw[off:off + n + 1]
    buf[n] = GUARD
    extra = None
    if guarded is None:
        src = np.full(a.size + 16, np.nan, dtype=np.float32)   # the batch between NaNs, at an odd 4-byte alignment
        src[7:7 + a.size] = a.reshape(-1)
        res = mod.mel_windows(h, src[7:7 + a.size].reshape(a.shape), valid, T, layout, buf, **(dict(tables=True) if tables else {}))
        if tables:
            extra = res[1:]
    else:
        mod.mel_guarded(h, a, valid, T, layout, guarded, buf)
    assert buf[n] == GUARD and np.all(raw[:off] == NAN_FILL), "a word outside the output was written"
    out = buf[:n].view(np.float32)
    out = out.reshape(B, n_mels, T).transpose(0, 2, 1) if layout == sm.CT else out.reshape(B, T, n_mels)
    return (out,) + tuple(extra) if tables else out


def _corner(N, H, T, L, v):
    """A dead frame whose reflected taps reach below valid: frame t >= valid_frames whose last tap t*H + N - 1 - P lies at or past L
    and reflects to 2(L-1) - (t*H + N - 1 - P) < valid.  Both kernels leave such a frame uncomputed, so the comparison covers it."""
    P = N // 2
    vf = int(sc.valid_frames([v], H, T, P)[0])
    return any(t * H + N - 1 - P >= L and 2 * (L - 1) - (t * H + N - 1 - P) < v for t in range(vf, T))


@pytest.mark.parametrize("N,H,n_mels", SHAPES)
def test_centred_is_the_uncentred_kernel_on_the_padded_batch(N, H, n_mels):
    """Every frame count, length, valid, layout and pad mode in power mode, and ln in one layout: the same words as clx_k_mel on
    np.pad's batch with valid' = valid + P (0 for valid == 0).  Power mode is also under the bound of the float64 reference on the
    padded batch.  No listed case is left out: a dead frame is not computed by either kernel, so the comparison also holds in the
    corner where a dead frame's reflected taps would reach below valid (it needs t*H >= L - 1 with valid < L).  The cases in that
    corner are counted -- at most one per shape is allowed, and none of the listed cases falls into it: the print names them."""
    P = N // 2
    w, fb = _tables(N, n_mels)
    plain = {mode: sm.create(N, H, w, fb, n_mels, mode, FLOOR) for mode in (sm.POWER, sm.LN)}
    corners = []
    for pad in PADS:
        hc = {mode: sc.create(N, H, w, fb, n_mels, mode, FLOOR, dict(center=1, pad=pad)) for mode in (sm.POWER, sm.LN)}
        for T, L, valids in _cases(N, H):
            a, valid = _batch(L, valids, seed=N + T + L)
            ap = sc.pad_batch(a, P, pad)
            vp = np.where(valid > 0, valid + P, 0).astype(np.uint32)
            vf = sc.valid_frames(valid, H, T, P)
            assert vf[0] == 0 and vf[-1] == T and np.array_equal(vf, sm.valid_frames(vp, H, T)), (T, L, vf)
            if pad == sc.PAD_REFLECT:
                corners += [(T, L, v) for v in valids if v < L and _corner(N, H, T, L, v)]
            M64, dM = sm.reference(ap, w, fb, N, H, T)
            for layout in LAYOUTS:
                got, vf_lib, _ = _run(sc, hc[sm.POWER], a, valid, T, n_mels, layout, tables=True)
                want = _run(sm, plain[sm.POWER], ap, vp, T, n_mels, layout)
                assert np.array_equal(vf_lib, vf), (T, L, vf_lib, vf)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, pad, T, L, layout)
                for k in range(len(valids)):
                    assert np.all(got[k, vf[k]:].view(np.uint32) == 0), (pad, T, L, k)
                    assert np.all(np.abs(got[k, :vf[k]].astype(np.float64) - M64[k, :vf[k]]) <= dM[k, :vf[k]]), (pad, T, L, k)
            got = _run(sc, hc[sm.LN], a, valid, T, n_mels, sm.TC)
            assert np.array_equal(got.view(np.uint32), _run(sm, plain[sm.LN], ap, vp, T, n_mels, sm.TC).view(np.uint32)), (N, pad, T, L, "ln")
        for h in hc.values():
            sc.destroy(h)
    for h in plain.values():
        sm.destroy(h)
    print("n_fft %d hop %d: dead frames with reflected taps below valid in %r" % (N, H, corners))
    assert len(corners) <= 1, corners


def _ranged_batch(N, H, T, L, center, seed):
    """Five windows: the loudest frames in the last frame group; in the first; some frames dead (valid inside); valid = 0; a window
    of zeros that is live to its end (computed frames of silence)."""
    rng = np.random.default_rng(seed)
    a = (1e-3 * rng.uniform(-1.0, 1.0, size=(5, L))).astype(np.float32)
    loud = 31 * H + (N // 2 if center else N)                # (behind every tap of the first group's frames)
    a[0, loud:] = rng.uniform(-1.0, 1.0, size=L - loud).astype(np.float32)
    a[1, :N] = rng.uniform(-1.0, 1.0, size=N).astype(np.float32)
    a[2] = rng.uniform(-1.0, 1.0, size=L).astype(np.float32)
    a[4] = 0.0
    valid = np.array([L, L, L // 3, 0, L], dtype=np.uint32)
    for k, v in enumerate(valid):
        a[k, v:] = 0.0
    return a, valid


@pytest.mark.parametrize("N,H,n_mels,center", ((400, 160, 80, 1), (50, 7, 5, 1), (600, 200, 40, 1), (51, 7, 5, 0)))
def test_range_scaling_is_float32_numpy_on_the_unranged_output(N, H, n_mels, center):
    """37 frames (two groups).  The ranged output equals float32 maximum(y, max_k - D), + shift, * scale on the unranged output of the
    same spec shape with the dead frames set to finish(mode, floor, 0); wmax is that maximum; both log modes, both (D, shift, scale),
    both layouts, the output on and off the 16-byte grid (n_mels * n_frames is odd for two of the shapes)."""
    T, P = 37, N // 2
    L = T * H if center else (T - 1) * H + N
    w, fb = _tables(N, n_mels)
    a, valid = _ranged_batch(N, H, T, L, center, seed=N)
    vf = sc.valid_frames(valid, H, T, P) if center else sm.valid_frames(valid, H, T)
    assert vf[0] == T and 0 < vf[2] < T and vf[3] == 0 and vf[4] == T
    for mode in (sm.LN, sm.LOG10):
        y0 = sm.finish(mode, FLOOR, [0.0])[0]
        hu = sc.create(N, H, w, fb, n_mels, mode, FLOOR, dict(center=center, pad=sc.PAD_REFLECT))
        u = _run(sc, hu, a, valid, T, n_mels, sm.TC).copy()
        sc.destroy(hu)
        assert np.all(u[4].view(np.uint32) == y0.view(np.uint32)), "a computed frame of zeros is not the silence value"
        for k in range(5):
            assert np.all(u[k, vf[k]:].view(np.uint32) == 0)
            u[k, vf[k]:] = y0
        mx = u.reshape(5, -1).max(axis=1)
        assert np.argmax(u[0].max(axis=1)) >= 32 and np.argmax(u[1].max(axis=1)) < 32 and mx[3] == y0
        for D, shift, scale in RANGES:
            lo = (mx - np.float32(D)).astype(np.float32)
            want = ((np.maximum(u, lo[:, None, None]) + np.float32(shift)).astype(np.float32) * np.float32(scale)).astype(np.float32)
            silence = np.float32(np.float32(np.maximum(y0, np.float32(y0 - np.float32(D))) + np.float32(shift)) * np.float32(scale))
            assert np.all(want[3].view(np.uint32) == silence.view(np.uint32))
            hr = sc.create(N, H, w, fb, n_mels, mode, FLOOR, dict(center=center, pad=sc.PAD_REFLECT, range=1, range_width=D, shift=shift, scale=scale))
            for layout in LAYOUTS:
                for off in (0, 1, 3):
                    got, vf_lib, wmax = _run(sc, hr, a, valid, T, n_mels, layout, shift=off, tables=True)
                    assert np.array_equal(vf_lib, vf) and np.array_equal(wmax.view(np.uint32), mx.view(np.uint32)), (mode, wmax, mx)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, mode, D, shift, scale, layout, off)
            sc.destroy(hr)


def test_the_encoding_keeps_the_order():
    vals = np.array([-np.inf, -3.4e38, -10.0, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 9.999, 10.0, 3.4e38, np.inf], dtype=np.float32)
    enc = [sc.lib().sim_melc_enc(float(v)) for v in vals]
    assert enc == sorted(enc) and len(set(enc)) == len(enc) and enc[0] == 0x007fffff
    assert all(np.float32(sc.lib().sim_melc_dec(e)).view(np.uint32) == v.view(np.uint32) for e, v in zip(enc, vals))


@pytest.mark.parametrize("pad", PADS)
def test_loads_stay_inside_the_batch_and_below_valid(pad):
    """The batch ends on the last float before an inaccessible page, or begins on the first float behind one: a stray load faults.
    Zero mode: the floats from valid[k] on are NaN here (valid < L; a NaN-filled tail behind every window's live part) and change
    nothing, so none of them is loaded."""
    for N, H, n_mels in SHAPES:
        w, fb = _tables(N, n_mels)
        h = sc.create(N, H, w, fb, n_mels, sm.POWER, FLOOR, dict(center=1, pad=pad))
        for T, L, valids in _cases(N, H):
            if T == 33:
                continue
            a, valid = _batch(L, valids, seed=5 * N + T + L)
            want = _run(sc, h, a, valid, T, n_mels, sm.CT).copy()
            for at_end in (True, False):
                got = _run(sc, h, a, valid, T, n_mels, sm.CT, guarded=at_end)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, pad, T, L, at_end)
            if pad == sc.PAD_ZERO:
                b = a.copy()
                for k, v in enumerate(valids):
                    b[k, v:] = np.nan
                assert any(v < L for v in valids)
                for layout in LAYOUTS:
                    got = _run(sc, h, b, valid, T, n_mels, layout, guarded=True)
                    assert np.array_equal(got.view(np.uint32), (want if layout == sm.CT else _run(sc, h, a, valid, T, n_mels, sm.TC)).view(np.uint32)), (N, T, L, layout)
        sc.destroy(h)


def test_new_refusals_and_the_plain_spec_unchanged():
    N, H, n_mels, T = 50, 7, 5, 9
    w, fb = _tables(N, n_mels)
    ok = dict(n_fft=N, hop=H, window=w, fbank=fb, n_mels=n_mels, mode=sm.LOG10, floor=FLOOR)
    rng = dict(range=1, range_width=8.0, shift=4.0, scale=0.25)
    nan, inf = float("nan"), float("inf")
    for kw, opts, why in ((dict(mode=sm.POWER), rng, "clx_mel_create_ex: range scaling needs a log mode"),
                          ({}, dict(rng, range_width=0.0), "range_width must be finite and greater than 0"),
                          ({}, dict(rng, range_width=-1.0), "range_width must be finite and greater than 0"),
                          ({}, dict(rng, range_width=inf), "range_width must be finite and greater than 0"),
                          ({}, dict(rng, range_width=nan), "range_width must be finite and greater than 0"),
                          ({}, dict(rng, shift=inf), "shift must be finite"), ({}, dict(rng, shift=nan), "shift must be finite"),
                          ({}, dict(rng, scale=0.0), "scale must be finite and not zero"), ({}, dict(rng, scale=-inf), "scale must be finite and not zero"),
                          ({}, dict(rng, scale=nan), "scale must be finite and not zero"),
                          ({}, dict(pad=2), "pad must be CLX_MEL_PAD_REFLECT or CLX_MEL_PAD_ZERO"),
                          ({}, dict(center=1, pad=7), "pad must be CLX_MEL_PAD_REFLECT or CLX_MEL_PAD_ZERO"),
                          ({}, dict(range=2), "range must be 0 or 1"), ({}, dict(center=2), "center must be 0 or 1"),
                          (dict(floor=0.0), rng, "floor must be greater than 0 in a log mode"), (dict(window=None), rng, "clx_mel_create: null argument")):
        with pytest.raises(cx.ClaxonError) as e:
            sc.create(**dict(ok, **kw), opts=opts)
        assert e.value.status == cx.API_ERROR and why in e.value.message, (opts, e.value.message)
    sc.destroy(sc.create(**ok, opts=dict(rng, scale=-2.0, shift=-1.0)))                    # (a negative scale or shift is a value like any other)
    sc.destroy(sc.create(**dict(ok, mode=sm.POWER), opts=dict(range=0, range_width=nan, scale=0.0)))   # (not ranged: the numbers are not looked at)
    # the centred length conditions: P < window_len, and torch.stft's frame count
    P = N // 2
    hc = sc.create(**ok, opts=dict(center=1))
    out = np.zeros(4 * T * n_mels, dtype=np.float32)
    a = np.zeros((1, T * H), dtype=np.float32)
    sc.mel_windows(hc, a, [T * H], T + 1, sm.CT, out)                                      # 1 + L // H frames
    for call, why in ((dict(audio=a, valid=[1], n_frames=T + 2), "window_len + 2 * (n_fft / 2) is less than (n_frames - 1) * hop + n_fft"),
                      (dict(audio=a[:, :P].copy(), valid=[1], n_frames=1), "a centred spec needs n_fft / 2 less than window_len"),
                      (dict(audio=a, valid=[T * H + 1], n_frames=T), "valid[k] is larger than window_len"),
                      (dict(audio=a, valid=[1], n_frames=T, layout=2), "layout must be CLX_WINDOW_TC or CLX_WINDOW_CT")):
        with pytest.raises(cx.ClaxonError) as e:
            sc.mel_windows(hc, call["audio"], call["valid"], call["n_frames"], call.get("layout", sm.CT), out)
        assert why in e.value.message, (call, e.value.message)
    sc.mel_windows(hc, a[:, :P + 1].copy(), [1], 1, sm.CT, out)
    h51 = sc.create(**dict(ok, n_fft=51, window=sm.hann(51), fbank=sm.triangles(SR, 51, n_mels)), opts=dict(center=1))
    sc.mel_windows(h51, a[:, :8 * H + 1].copy(), [1], 9, sm.CT, out)                        # odd N: (T - 1) * H + 1 <= L
    with pytest.raises(cx.ClaxonError) as e:
        sc.mel_windows(h51, a[:, :8 * H].copy(), [1], 9, sm.CT, out)
    assert "window_len + 2 * (n_fft / 2)" in e.value.message
    # the uncentred condition stays as it is, for a ranged spec too
    hr = sc.create(**ok, opts=rng)
    with pytest.raises(cx.ClaxonError) as e:
        sc.mel_windows(hr, a[:, :(T - 1) * H + N - 1].copy(), [1], T, sm.CT, out)
    assert "window_len is less than (n_frames - 1) * hop + n_fft" in e.value.message
    out[:] = 7.0                                                                             # the empty calls touch nothing
    sc.mel_windows(hr, None, [], T, sm.CT, None, shape=(0, 100))
    sc.mel_windows(hc, a, [3], 0, sm.CT, out)
    assert np.all(out == 7.0)
    for h in (hc, h51, hr):
        sc.destroy(h)
    # opts == NULL and all-zero opts: the same tables and the same words as clx_mel_create's spec
    L = (T - 1) * H + N
    a, valid = _batch(L, [0, 1, H + 1, L], seed=9)
    for mode in (sm.POWER, sm.LN, sm.LOG10):
        h0, h1, h2 = sm.create(N, H, w, fb, n_mels, mode, FLOOR), sc.create(N, H, w, fb, n_mels, mode, FLOOR), sc.create(N, H, w, fb, n_mels, mode, FLOOR, {})
        assert np.array_equal(sc.table_words(h1), sc.table_words(h2))
        for layout in LAYOUTS:
            want = _run(sm, h0, a, valid, T, n_mels, layout).copy()
            for h in (h1, h2):
                assert np.array_equal(_run(sc, h, a, valid, T, n_mels, layout).view(np.uint32), want.view(np.uint32)), (mode, layout)
        sm.destroy(h0)
        sc.destroy(h1)
        sc.destroy(h2)


@pytest.mark.parametrize("N,H", ((400, 160), (51, 7)))
def test_the_padding_definition_is_torch_stft_centred(N, H):
    """torch.stft(center=True, pad_mode="reflect") in float64 on random audio against the definition's re^2 + im^2 in float64 on the
    np.pad-reflected batch (simlib_mel.basis64), 1e-9 relative per cell; the frame count is torch's, for odd N too."""
    import torch
    P, L = N // 2, 13 * H + 5
    x = np.random.default_rng(N).uniform(-1.0, 1.0, size=(3, L))
    w = sm.hann(N)
    S = torch.stft(torch.from_numpy(x), N, hop_length=H, win_length=N, window=torch.from_numpy(w.astype(np.float64)), center=True,
                   pad_mode="reflect", return_complex=True)
    want = (S.real ** 2 + S.imag ** 2).numpy().transpose(0, 2, 1)                           # [B, T, J]
    T = want.shape[1]
    assert (T - 1) * H + N <= L + 2 * P < T * H + N                                        # (clx_mel_check's count is torch's)
    xp = np.pad(x, ((0, 0), (P, P)), mode="reflect")
    X = xp[:, np.arange(T)[:, None] * H + np.arange(N)[None, :]]
    Cb, Sb = sm.basis64(w, N)
    re, im = X @ Cb.T, X @ Sb.T
    got = re * re + im * im
    rel = np.abs(got - want) / np.maximum(got, want)
    print("n_fft %d: worst relative difference %.3g over %d cells" % (N, float(rel.max()), rel.size))
    assert np.all(rel <= 1e-9)
    # the index map of the header, tap by tap, is np.pad's
    i = np.arange(-P, L + P)
    refl = np.where(i < 0, -i, np.where(i >= L, 2 * (L - 1) - i, i))
    assert np.array_equal(xp, x[:, refl])
