"""The mel feature kernel (clx_mel.hip: clx_mel_build, clx_mel_check, clx_mel_fill and clx_k_mel) under the wave simulator, against
the definition evaluated in float64 with numpy (simlib_mel.reference: from the float32 window and filterbank, the basis in exact
double).  Power mode: |M - M64| <= dM per cell, dM the bound of claxon_hip.h (any summation order; derived, not tuned).  Log modes:
within LOG_ULPS ulps of float64 log(max(float64(M), floor)) with M the power-mode output of the same call shape -- the modes share M
bitwise.  A frame at or past valid_frames is the word 0.  The batch sits between NaNs, and in the guarded runs next to an
inaccessible page; the output starts as a NaN pattern with a guard word behind it."""
import numpy as np
import pytest

import claxon_amd as cx
import simlib_mel as sm

NAN_FILL = 0x7fc0dead            # a quiet NaN with a payload: what the output holds before the call
GUARD = 0xffc0beef               # the word behind the output
SR = 16000
# (n_fft, hop, n_mels): (16, 40, 3) has hop > n_fft; (600, 200, 40) has J = 301 bins, two passes of the kernel's 256, the second
# partial; (512, 128, 64) has J = 257, a second pass of one bin; (510, 170, 64) has J = 256, one pass that is exactly full
SHAPES = ((400, 160, 80), (64, 24, 13), (50, 7, 5), (16, 40, 3), (600, 200, 40), (512, 128, 64), (510, 170, 64))
GROUP = 32                       # clx_mel::kF, a block's frame group
FRAMES = (1, 37, GROUP + 1)
LAYOUTS = (sm.CT, sm.TC)
FLOOR = 1e-10


def _tables(N, n_mels):
    return sm.hann(N), sm.triangles(SR, N, n_mels)


def _valids(H, L):
    return sorted({0, 1, H, H + 1, L // 2, L} & set(range(L + 1)))


def _batch(N, H, T, seed, kind="noise"):
    """audio [B, L] with one window per valid value, zero from valid[k] on; valid."""
    L = (T - 1) * H + N
    valid = np.array(_valids(H, L), dtype=np.uint32)
    rng = np.random.default_rng(seed)
    if kind == "noise":
        a = rng.uniform(-1.0, 1.0, size=(valid.size, L))
    elif kind == "quiet":                                    # 16-bit samples, sigma of 3 LSB
        a = np.round(rng.normal(0.0, 3.0, size=(valid.size, L))) / 32768.0
    else:                                                    # a 1 kHz tone with 1e-3 noise: ill-conditioned away from the tone
        a = np.sin(2.0 * np.pi * 1000.0 * np.arange(L) / SR)[None, :] + 1e-3 * rng.uniform(-1.0, 1.0, size=(valid.size, L))
    a = a.astype(np.float32)
    for k, v in enumerate(valid):
        a[k, v:] = 0.0
    return a, valid


def _run(h, a, valid, T, n_mels, layout, guarded=None):
    """One call; the output as [B, T, n_mels] float32 (a view of the buffer), after the guard word's check."""
    B = a.shape[0]
    n = B * n_mels * T
    buf = np.full(n + 1, NAN_FILL, dtype=np.uint32)
    buf[n] = GUARD
    if guarded is None:
        src = np.full(a.size + 16, np.nan, dtype=np.float32)  # the batch between NaNs, at an odd 4-byte alignment
        src[7:7 + a.size] = a.reshape(-1)
        sm.mel_windows(h, src[7:7 + a.size].reshape(a.shape), valid, T, layout, buf)
    else:
        sm.mel_guarded(h, a, valid, T, layout, guarded, buf)
    assert buf[n] == GUARD, "the word behind the output was written"
    out = buf[:n].view(np.float32)
    return out.reshape(B, n_mels, T).transpose(0, 2, 1) if layout == sm.CT else out.reshape(B, T, n_mels)


def _check_power(got, ref, valid, H, T, what):
    """Power-mode output against (M64, dM); returns the worst |error| / bound."""
    M64, dM = ref
    vf = sm.valid_frames(valid, H, T)
    worst = 0.0
    for k in range(got.shape[0]):
        assert np.all(got[k, vf[k]:].view(np.uint32) == 0), (what, k, "a frame past valid_frames is not the word 0")
        live = got[k, :vf[k]].astype(np.float64)
        err = np.abs(live - M64[k, :vf[k]])
        bad = np.argwhere(~(err <= dM[k, :vf[k]]))
        assert bad.size == 0, (what, "window %d frame %d band %d: %r, expected %r, bound %.3g" % (
            k, bad[0][0], bad[0][1], live[tuple(bad[0])], M64[k][tuple(bad[0])], dM[k][tuple(bad[0])]))
        if vf[k]:
            worst = max(worst, float(np.max(err / np.where(dM[k, :vf[k]] > 0, dM[k, :vf[k]], 1.0))))
    return worst


@pytest.mark.parametrize("N,H,n_mels", SHAPES)
def test_power_under_the_bound_and_the_log_modes(N, H, n_mels):
    """Every frame count, layout and mode; per frame count one window for each valid of 0, 1, H, H + 1, L // 2 and L."""
    w, fb = _tables(N, n_mels)
    hs = {mode: sm.create(N, H, w, fb, n_mels, mode, FLOOR) for mode in (sm.POWER, sm.LN, sm.LOG10)}
    for T in FRAMES:
        a, valid = _batch(N, H, T, seed=N + T)
        ref = sm.reference(a, w, fb, N, H, T)
        vf = sm.valid_frames(valid, H, T)
        assert vf[0] == 0 and vf[-1] == T and (T == 1 or 0 < vf[len(vf) // 2] < T), vf
        power = {}
        for layout in LAYOUTS:
            got = _run(hs[sm.POWER], a, valid, T, n_mels, layout)
            worst = _check_power(got, ref, valid, H, T, (N, H, n_mels, T, layout))
            print("n_fft %d hop %d bands %d frames %d layout %d: worst |error| / bound %.4f" % (N, H, n_mels, T, layout, worst))
            power[layout] = got.copy()
        assert np.array_equal(power[sm.CT].view(np.uint32), power[sm.TC].view(np.uint32)), "the layouts differ in M"
        for mode in (sm.LN, sm.LOG10):
            for layout in LAYOUTS:
                got = _run(hs[mode], a, valid, T, n_mels, layout)
                for k in range(got.shape[0]):
                    assert np.all(got[k, vf[k]:].view(np.uint32) == 0), (N, T, mode, layout, k)
                    ulps = sm.log_ulps(got[k, :vf[k]], power[layout][k, :vf[k]], mode, FLOOR)
                    assert np.all(ulps <= sm.LOG_ULPS), (N, T, mode, layout, k, float(ulps.max()))
    for h in hs.values():
        sm.destroy(h)


def test_the_bound_is_not_vacuous_and_the_tone():
    """On the reference alone: at least 99 % of the live cells of the two noise inputs have dM <= 1e-2 * M64 (n_fft 400, hop 160,
    80 HTK bands at 16 kHz).  The tone with 1e-3 noise is checked in power mode under the absolute bound only."""
    N, H, n_mels, T = 400, 160, 80, 37
    w, fb = _tables(N, n_mels)
    h = sm.create(N, H, w, fb, n_mels, sm.POWER, FLOOR)
    for kind in ("noise", "quiet", "tone"):
        a, valid = _batch(N, H, T, seed=7, kind=kind)
        M64, dM = ref = sm.reference(a, w, fb, N, H, T)
        if kind != "tone":
            k = len(valid) - 1                               # the window that is live to its end
            share = float(np.mean(dM[k] <= 1e-2 * M64[k]))
            print("%s: share of cells with dM <= 1e-2 M64: %.4f, median dM / M64 %.2e" % (kind, share, float(np.median(dM[k] / M64[k]))))
            assert share >= 0.99, (kind, share)
        for layout in LAYOUTS:
            worst = _check_power(_run(h, a, valid, T, n_mels, layout), ref, valid, H, T, (kind, layout))
            print("%s, layout %d: worst |error| / bound %.4f" % (kind, layout, worst))
    sm.destroy(h)


def test_an_all_zero_window():
    """Exactly 0.0 in power mode; log(floor) within LOG_ULPS in the log modes (the window is valid to its end: its frames are live)."""
    N, H, n_mels, T = 64, 24, 13, 5
    w, fb = _tables(N, n_mels)
    L = (T - 1) * H + N
    a, valid = np.zeros((1, L), dtype=np.float32), np.array([L], dtype=np.uint32)
    for layout in LAYOUTS:
        for mode in (sm.POWER, sm.LN, sm.LOG10):
            h = sm.create(N, H, w, fb, n_mels, mode, FLOOR)
            got = _run(h, a, valid, T, n_mels, layout)
            if mode == sm.POWER:
                assert np.all(got.view(np.uint32) == 0)
            else:
                assert np.all(sm.log_ulps(got, np.zeros_like(got), mode, FLOOR) <= sm.LOG_ULPS), got
                assert abs(float(got[0, 0, 0]) - (np.log(FLOOR) if mode == sm.LN else -10.0)) < 1e-5
            sm.destroy(h)


def test_the_log_step_and_its_ulps():
    """What LOG_ULPS rests on: the worst error of the simulator's logf / log10f over the values the tests above feed them (the power
    outputs of every shape) and over a sweep of the float32 range from the floor up, in ulps of the result."""
    vals = [np.float32(FLOOR) * np.float32(2.0) ** np.linspace(0.0, 60.0, 20001, dtype=np.float32)]
    for N, H, n_mels in SHAPES:
        w, fb = _tables(N, n_mels)
        h = sm.create(N, H, w, fb, n_mels, sm.POWER, FLOOR)
        a, valid = _batch(N, H, 37, seed=N + 37)
        vals.append(_run(h, a, valid, 37, n_mels, sm.TC).reshape(-1).copy())
        sm.destroy(h)
    m = np.concatenate(vals)
    for mode, name in ((sm.LN, "logf"), (sm.LOG10, "log10f")):
        worst = float(sm.log_ulps(sm.finish(mode, FLOOR, m), m, mode, FLOOR).max())
        print("%s: worst error %.3f ulp over %d values" % (name, worst, m.size))
        assert 2.0 * worst <= sm.LOG_ULPS, (name, worst)
    assert sm.LOG_ULPS >= 2.0


@pytest.mark.parametrize("layout", LAYOUTS)
def test_loads_stay_inside_the_batch(layout):
    """The batch ends on the last float before an inaccessible page, or begins on the first float behind one: a stray load faults.
    Every window's frames reach the window's last float, so the last window's reach the batch's."""
    for N, H, n_mels in SHAPES:
        w, fb = _tables(N, n_mels)
        h = sm.create(N, H, w, fb, n_mels, sm.POWER, FLOOR)
        for T in (1, GROUP + 1):
            a, valid = _batch(N, H, T, seed=3 * N + T)
            ref = sm.reference(a, w, fb, N, H, T)
            for at_end in (True, False):
                _check_power(_run(h, a, valid, T, n_mels, layout, guarded=at_end), ref, valid, H, T, (N, T, layout, at_end))
        sm.destroy(h)


def test_a_longer_window_and_a_row_of_zeros():
    """window_len above (n_frames - 1) * hop + n_fft: the samples behind the last frame are not read into any sum (they are NaN
    here, and valid may point into them).  A filterbank row of zeros gives 0 (log(floor) in a log mode); a row is summed over its
    first to last non-zero bin only, so a NaN power outside that range does not reach it."""
    N, H, n_mels, T = 50, 7, 5, 9
    w, fb = _tables(N, n_mels)
    fb = fb.copy()
    fb[2] = 0.0
    h = sm.create(N, H, w, fb, n_mels, sm.POWER, FLOOR)
    c, s, ends = sm.tables(h, N, n_mels)
    assert ends[2, 0] == ends[2, 1] and all(ends[m, 0] < ends[m, 1] for m in (0, 1, 3, 4))
    for m in (0, 1, 3, 4):
        nz = np.nonzero(fb[m])[0]
        assert (ends[m, 0], ends[m, 1]) == (nz[0], nz[-1] + 1)
    L = (T - 1) * H + N
    a = np.full((2, L + 11), np.nan, dtype=np.float32)
    a[:, :L] = np.random.default_rng(2).uniform(-1, 1, size=(2, L)).astype(np.float32)
    valid = np.array([L + 11, L + 3], dtype=np.uint32)
    ref = sm.reference(a[:, :L], w, fb, N, H, T)
    for layout in LAYOUTS:
        got = _run(h, a, valid, T, n_mels, layout)
        _check_power(got, ref, np.array([L, L]), H, T, layout)
        assert np.all(got[:, :, 2].view(np.uint32) == 0)
    sm.destroy(h)
    hl = sm.create(N, H, w, fb, n_mels, sm.LN, FLOOR)
    got = _run(hl, a, valid, T, n_mels, sm.CT)
    assert np.all(sm.log_ulps(got[:, :, 2], np.zeros((2, T)), sm.LN, FLOOR) <= sm.LOG_ULPS)
    sm.destroy(hl)


def test_refused_arguments_and_empty_calls():
    N, H, n_mels, T = 16, 40, 3, 2
    w, fb = _tables(N, n_mels)
    ok = dict(n_fft=N, hop=H, window=w, fbank=fb, n_mels=n_mels, mode=sm.LN, floor=FLOOR)
    for change, why in ((dict(n_fft=1), "n_fft must be 2..2048"), (dict(n_fft=2049), "n_fft must be 2..2048"), (dict(hop=0), "hop must be at least 1"),
                        (dict(n_mels=0), "n_mels must be 1..256"), (dict(n_mels=257), "n_mels must be 1..256"),
                        (dict(mode=3), "mode must be CLX_MEL_POWER, CLX_MEL_LN or CLX_MEL_LOG10"),
                        (dict(floor=0.0), "floor must be greater than 0 in a log mode"), (dict(floor=-1.0), "floor must be greater than 0 in a log mode"),
                        (dict(floor=float("nan")), "floor must be greater than 0 in a log mode"),
                        (dict(mode=sm.LOG10, floor=0.0), "floor must be greater than 0 in a log mode"),
                        (dict(window=None), "clx_mel_create: null argument"), (dict(fbank=None), "clx_mel_create: null argument")):
        with pytest.raises(cx.ClaxonError) as e:
            sm.create(**dict(ok, **change))
        assert e.value.status == cx.API_ERROR and why in e.value.message, (change, e.value.message)
    sm.destroy(sm.create(**dict(ok, mode=sm.POWER, floor=0.0)))          # (power mode does not use the floor)
    sm.destroy(sm.create(**dict(ok, n_fft=2, window=sm.hann(2), fbank=np.ones((3, 2), np.float32))))
    big = sm.create(2048, 1 << 31, sm.hann(2048), np.ones((256, 1025), np.float32), 256, sm.POWER, 0.0)    # (the largest of each)
    sm.destroy(big)
    h = sm.create(**ok)
    L = (T - 1) * H + N
    a, out = np.zeros((2, L), dtype=np.float32), np.zeros(2 * T * n_mels, dtype=np.float32)
    call = dict(h=h, audio=a, valid=[L, 3], n_frames=T, layout=sm.CT, out=out)
    sm.mel_windows(**call)
    for change, why in ((dict(layout=2), "layout must be CLX_WINDOW_TC or CLX_WINDOW_CT"), (dict(layout=7), "layout must be"),
                        (dict(audio=None, shape=(2, L)), "clx_mel_windows: null argument"), (dict(out=None), "clx_mel_windows: null argument"),
                        (dict(valid=None), "clx_mel_windows: null argument"), (dict(h=-1), "clx_mel_windows: null spec"),
                        (dict(n_frames=T + 1), "window_len is less than (n_frames - 1) * hop + n_fft"),
                        (dict(audio=a[:, :L - 1].copy()), "window_len is less than (n_frames - 1) * hop + n_fft"),
                        (dict(valid=[L, L + 1]), "valid[k] is larger than window_len")):
        with pytest.raises(cx.ClaxonError) as e:
            sm.mel_windows(**dict(call, **change))
        assert e.value.status == cx.API_ERROR and why in e.value.message, (change, e.value.message)
    # more blocks than a grid has (refused before anything is looked at on the device side): hop 1, 2^32 - 1 - n_fft frames, 64 windows
    h1 = sm.create(**dict(ok, hop=1))
    with pytest.raises(cx.ClaxonError) as e:
        sm.mel_windows(h1, None, [0] * 64, (1 << 32) - 1 - N, sm.CT, out, shape=(64, (1 << 32) - 1))
    assert "null" in e.value.message
    with pytest.raises(cx.ClaxonError) as e:
        sm.mel_windows(h1, out, [0] * 64, (1 << 32) - 1 - N, sm.CT, out, shape=(64, (1 << 32) - 1))
    assert "too many" in e.value.message
    # the empty calls succeed, touch nothing and need no pointer
    out[:] = 7.0
    sm.mel_windows(h, None, [], T, sm.CT, None, shape=(0, L))
    sm.mel_windows(h, a, [L, 3], 0, sm.CT, out)
    sm.mel_windows(h, None, None, 0, sm.TC, None, shape=(2, 0))
    assert np.all(out == 7.0)
    with pytest.raises(cx.ClaxonError):
        sm.mel_windows(h, None, [], T, 5, None, shape=(0, L))            # (the layout is checked first)
    for x in (h, h1):
        sm.destroy(x)


def test_table_parity():
    """The library's basis against numpy's (double, rounded once): equal as words, or one float32 ulp apart where the two libms'
    doubles round apart -- fewer than 1 in 10^4.  MelSpec's window and HTK filterbank equal this file's own construction; each row
    of the Slaney-normalised bank is 2 / (f_hi - f_lo) times the row of plain triangles (compared by their sums, 1e-6 relative:
    the sum of a plain row is the triangle's area in units of the bin spacing)."""
    apart = total = 0
    for N, H, n_mels in SHAPES + ((2048, 512, 128),):
        spec = cx.MelSpec(None, SR, n_fft=N, hop=H, n_mels=n_mels, mode="power")
        assert spec.window.dtype == np.float32 and np.array_equal(spec.window.view(np.uint32), sm.hann(N).view(np.uint32))
        assert spec.fbank.dtype == np.float32 and spec.fbank.shape == (n_mels, N // 2 + 1)
        assert np.array_equal(spec.fbank.view(np.uint32), sm.triangles(SR, N, n_mels).view(np.uint32))
        h = sm.create(N, H, spec.window, spec.fbank, n_mels, sm.POWER, 0.0)
        c, s, ends = sm.tables(h, N, n_mels)
        sm.destroy(h)
        c64, s64 = sm.basis64(spec.window, N)
        for got, want in ((c, c64.astype(np.float32)), (s, s64.astype(np.float32))):
            diff = got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)
            zero = (got == 0) & (want == 0)                  # (+0 and -0: sin(0) negated)
            diff[zero] = 0
            assert np.all(np.abs(diff) <= 1), (N, int(np.abs(diff).max()))
            apart += int(np.count_nonzero(diff))
            total += diff.size
    print("basis entries one ulp apart: %d of %d" % (apart, total))
    assert apart * 10 ** 4 < total
    for scale in ("htk", "slaney"):
        N, n_mels = 400, 80
        normed = cx.MelSpec(None, SR, n_fft=N, n_mels=n_mels, mel_scale=scale, norm="slaney").fbank.astype(np.float64)
        plain = cx.MelSpec(None, SR, n_fft=N, n_mels=n_mels, mel_scale=scale).fbank.astype(np.float64)
        assert np.array_equal(cx.MelSpec(None, SR, n_fft=N, n_mels=n_mels, mel_scale=scale).fbank, sm.triangles(SR, N, n_mels, scale=scale))
        pts = sm.mel_points(SR, n_mels, scale=scale)
        want = 2.0 / (pts[2:] - pts[:-2]) * plain.sum(axis=1)
        assert np.all(np.abs(normed.sum(axis=1) - want) <= 1e-6 * want)
    spec = cx.MelSpec(None, 22050, n_fft=512, hop=128, n_mels=40, f_min=50.0, f_max=8000.0, mel_scale="slaney", norm="slaney", mode="log10")
    assert np.array_equal(spec.fbank, sm.triangles(22050, 512, 40, 50.0, 8000.0, "slaney", True)) and spec.window_len(3) == 768


def test_melspec_refusals():
    with pytest.raises(ValueError, match="band 0 "):
        cx.MelSpec(None, SR, n_fft=64, n_mels=80)            # (more bands than bins: the first band falls between two bins)
    for kw in (dict(n_fft=1), dict(n_fft=4096), dict(hop=0), dict(n_mels=0), dict(n_mels=300), dict(mode="db"), dict(floor=0.0),
               dict(mel_scale="bark"), dict(norm="l2"), dict(f_max=9000.0), dict(f_min=-1.0), dict(n_fft=400.5)):
        with pytest.raises(ValueError):
            cx.MelSpec(None, SR, **kw)
    assert cx.MelSpec(None, SR, mode="power", floor=0.0).floor == 0.0
