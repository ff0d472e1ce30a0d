"""The float kernels on the GPU against the wave simulator, word for word: clx_k_mel (power mode), clx_k_resample and clx_k_mix write
the same 32-bit words as the same source built by g++ and run on host arrays (simlib_mel, simlib_resample, simlib_mix).  Every sum in
these kernels is a chain of explicit fmaf in a fixed order over tables built on the host in double, so the two builds have nothing to
differ in; a difference is a miscompile, a race the simulator's fixed schedule hides, a table that differs between the two host
compilers, or a contraction.  The float64 definition under its derived bound stays beside the equality as the check that what the
two share is right (simlib_mel.reference, simlib_resample.assert_close), and the log modes, whose last step is the device's logf /
log10f, are held to LOG_ULPS of float64 log(max(float64(M), floor)) with M the power output of the same call shape.  The other four
mel kernels -- clx_k_mel_c, clx_k_mel_range, clx_k_mel_f and clx_k_mel_q -- are held in the same way in test_gpu_mel_forms.py.

The shapes are those where a device build can go its own way: mel with more than one pass of 256 bins (J = 301; J = 257, a second
pass of one bin; n_fft 2048, five passes of 128 K-slices), one pass exactly full (J = 256) and hop > n_fft; the resampler going up
(16000 -> 44100, 44100 -> 48000) and down, 1, 3 and 8 channels, windows of one output and of a tile and a few, and windows that end
just below output 2^43; the mixer reducing 2, 3 and 8 channels and replicating to 2 and 8 under resampling.

Every output is a slice of a buffer filled with a NaN pattern, 64 guard words before it and 64 behind: the guards stay, no word of
the slice keeps the pattern, and what lies past the valid part is the word 0."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_mel as sml
import simlib_mix as smx
import simlib_resample as sr
from gpu_guarded import DEV, NAN_FILL, device_out as _device_out, written as _written
from test_gpu_resample import SHAPES as STREAMS, Case, _starts, _stream
from test_mel_sim import _batch, _check_power
from test_resample_sim import far_windows

pytestmark = pytest.mark.gpu
SR = 16000
FLOOR = 1e-10
TC, CT = cx.WINDOW_TC, cx.WINDOW_CT


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


# ---- the output buffer and the comparison -------------------------------------------------------------------------------------------

def _same_words(got, want, axes, what):
    """got and want ([B, x, y] float32) as 32-bit words; returns the cells compared."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    if bad.size:
        at = tuple(int(i) for i in bad[0])
        where = ", ".join("%s %d" % (name, i) for name, i in zip(axes, at))
        raise AssertionError("%r: %d of %d cells differ from the simulator; the first is %s: GPU 0x%08x (%r), simulator 0x%08x (%r)" % (
            what, bad.shape[0], g.size, where, int(g[at]), float(got[at]), int(w[at]), float(want[at])))
    return int(g.size)


# ---- mel ----------------------------------------------------------------------------------------------------------------------------

# (n_fft, hop, n_mels): frames.  33 is two frame groups, the second of one frame; 9 is one group with two live waves, the second
# wave with one live frame.
MEL = {(600, 200, 40): 33,       # J = 301: two passes, the second partial
       (512, 128, 64): 33,       # J = 257: the second pass holds one bin
       (510, 170, 64): 33,       # J = 256: one pass, exactly full
       (16, 40, 3): 33,          # hop > n_fft, one K-slice
       (2048, 512, 128): 9}      # the largest n_fft: 5 passes, 128 K-slices
TINY = np.float32(2.0 ** -70)    # noise scaled by this has every power below the smallest normal float32


@pytest.fixture(scope="module")
def mel_data():
    """Per spec, made once and shared by the layouts and modes: (audio [B, L], valid, frames, window, filterbank, (M64, dM)).  One
    window per valid of 0, 1, H, H + 1, L // 2 and L (test_mel_sim._batch); the 2048 spec keeps the windows of L and 0 only."""
    made = {}

    def get(N, H, n_mels):
        if (N, H, n_mels) not in made:
            T = MEL[(N, H, n_mels)]
            a, valid = _batch(N, H, T, seed=N + T)
            if N == 2048:
                a, valid = np.ascontiguousarray(a[[-1, 0]]), valid[[-1, 0]]
            assert valid.max() == a.shape[1] == (T - 1) * H + N and valid.min() == 0
            w, fb = sml.hann(N), sml.triangles(SR, N, n_mels)
            made[(N, H, n_mels)] = (a, valid, T, w, fb, sml.reference(a, w, fb, N, H, T))
        return made[(N, H, n_mels)]

    return get


def _spec(ctx, N, H, n_mels, mode, w, fb):
    spec = cx.MelSpec(ctx, SR, n_fft=N, hop=H, n_mels=n_mels, mode=mode, floor=FLOOR)
    assert np.array_equal(spec.fbank.view(np.uint32), fb.view(np.uint32)) and np.array_equal(spec.window.view(np.uint32), w.view(np.uint32))
    return spec


def _gpu_mel(ctx, spec, audio, valid, T, layout, what):
    """One call on the GPU; the output as [B, T, n_mels] float32 after the guard and fill checks."""
    B, n_mels = audio.shape[0], spec.n_mels
    n = B * n_mels * T
    flat, out = _device_out(n)
    shape = (B, n_mels, T) if layout == CT else (B, T, n_mels)
    torch.cuda.synchronize()                                 # (the fill first: on torch's default stream the launch goes to the context's own)
    ctx.mel_windows(spec, audio, valid, T, layout, out.view(shape))
    torch.cuda.synchronize()
    got = _written(flat, n, what).view(np.float32).reshape(shape)
    return got.transpose(0, 2, 1) if layout == CT else got


def _sim_mel(h, a, valid, T, n_mels, layout):
    B = a.shape[0]
    buf = np.full(B * n_mels * T, NAN_FILL, dtype=np.uint32)
    sml.mel_windows(h, a, valid, T, layout, buf)
    out = buf.view(np.float32)
    return out.reshape(B, n_mels, T).transpose(0, 2, 1) if layout == CT else out.reshape(B, T, n_mels)


@pytest.mark.parametrize("layout", (CT, TC))
@pytest.mark.parametrize("N,H,n_mels", tuple(MEL))
def test_mel_power_is_the_simulators_word_for_word(ctx, mel_data, N, H, n_mels, layout):
    """Uniform noise in [-1, 1); for (600, 200, 40) also the same noise times 2^-70, where every power is subnormal or zero: the
    float64 bound ignores underflow and is not applied there, the equality and "no NaN" are (the kernel keeps float32 subnormals,
    as the host build does)."""
    a, valid, T, w, fb, ref = mel_data(N, H, n_mels)
    vf = sml.valid_frames(valid, H, T)
    spec = _spec(ctx, N, H, n_mels, "power", w, fb)
    h = sml.create(N, H, w, fb, n_mels, sml.POWER, 0.0)
    try:
        for name, x in (("noise", a), ("noise * 2^-70", a * TINY))[:2 if N == 600 else 1]:
            what = (N, H, n_mels, T, "ct" if layout == CT else "tc", name)
            got = _gpu_mel(ctx, spec, torch.from_numpy(x).to(DEV), valid, T, layout, what)
            want = _sim_mel(h, x, valid, T, n_mels, layout)
            cells = _same_words(got, want, ("window", "frame", "band"), what)
            if name == "noise":
                worst = _check_power(got, ref, valid, H, T, what)        # (the bound, and the word 0 past valid_frames)
                print("%r: worst |error| / bound %.4f; %d cells word for word, 0 differ" % (what, worst, cells))
            else:
                assert np.all(np.isfinite(got)), (what, "a NaN or an infinity")
                live = np.concatenate([want[k, :vf[k]].reshape(-1) for k in range(len(vf))])
                assert np.all(np.abs(live) < np.float32(2.0 ** -126)) and np.count_nonzero(live) > live.size // 2, (what, "the batch is not subnormal")
                for k in range(len(vf)):
                    assert np.all(got[k, vf[k]:].view(np.uint32) == 0), (what, k, "a frame past valid_frames is not the word 0")
                print("%r: %d of %d live cells are non-zero subnormals; %d cells word for word, 0 differ" % (
                    what, int(np.count_nonzero(live)), live.size, cells))
    finally:
        spec.close()
        sml.destroy(h)


@pytest.mark.parametrize("N,H,n_mels", tuple(MEL))
def test_mel_log_modes_within_log_ulps(ctx, mel_data, N, H, n_mels):
    """ln and log10 in the [B, n_frames, n_mels] layout against float64 log(max(float64(M), floor)), M the power output of the same
    call shape (the modes share M bitwise); that M is the simulator's again."""
    a, valid, T, w, fb, ref = mel_data(N, H, n_mels)
    vf = sml.valid_frames(valid, H, T)
    dev = torch.from_numpy(a).to(DEV)
    got = {}
    for mode in ("power", "ln", "log10"):
        spec = _spec(ctx, N, H, n_mels, mode, w, fb)
        got[mode] = _gpu_mel(ctx, spec, dev, valid, T, TC, (N, H, n_mels, T, mode))
        spec.close()
    h = sml.create(N, H, w, fb, n_mels, sml.POWER, 0.0)
    _same_words(got["power"], _sim_mel(h, a, valid, T, n_mels, TC), ("window", "frame", "band"), (N, H, n_mels, T, "power"))
    sml.destroy(h)
    for mode in ("ln", "log10"):
        for k in range(len(vf)):
            assert np.all(got[mode][k, vf[k]:].view(np.uint32) == 0), (N, mode, k, "a frame past valid_frames is not the word 0")
        ulps = np.concatenate([sml.log_ulps(got[mode][k, :vf[k]], got["power"][k, :vf[k]], sml.MODES[mode], FLOOR).reshape(-1)
                               for k in range(len(vf))])
        print("(%d, %d, %d), %s: worst error %.3f ulp over %d cells" % (N, H, n_mels, mode, float(ulps.max()), ulps.size))
        assert np.all(ulps <= sml.LOG_ULPS), (N, mode, float(ulps.max()))


# ---- resample and mix ---------------------------------------------------------------------------------------------------------------

RS_T = 3000                      # source samples per channel and rate
TARGETS = {44100: (16000, 44100), 48000: (44100, 48000), 16000: (44100, 8000, 16000)}     # target: the source rates of its one call
LENGTHS = (1, 1030)              # one output; one tile of 1024 and a partial one


def _sources(seed, rates, Cs):
    """Noise [RS_T, Cs] per rate, back to back in one buffer from float 3 on: (the buffer, the arrays, each one's first float)."""
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(-1.0, 1.0, size=(RS_T, Cs)).astype(np.float32) for _ in rates]
    src = np.concatenate([np.zeros(3, np.float32)] + [x.reshape(-1) for x in xs])
    return src, xs, [3 + i * RS_T * Cs for i in range(len(rates))]


def _jobs(rates, R, Cs, L, base):
    """The per-window arguments (src_first, src_t0, src_n, out_t0, valid, src_rate) and, per window, (index of its source, start):
    per rate the windows from output 0, from T_R // 3, across the end (T_R - 400) and behind it (T_R: all zeros)."""
    per, which = ([], [], [], [], [], []), []
    for i, rate in enumerate(rates):
        T_R = RS_T if rate == R else sr.length_at(RS_T, rate, R)
        for st in (0, T_R // 3, T_R - 400, T_R):
            v = min(max(T_R - st, 0), L)
            lo, hi = (0, 0) if v == 0 else (st, st + v) if rate == R else sr.span(st, st + v - 1, RS_T, rate, R)
            for lst, val in zip(per, (base[i] + lo * Cs, lo, hi - lo, st, v, rate)):
                lst.append(val)
            which.append((i, st))
    return per, which


def _both(gpu_fn, sim_fn, src, src_dev, per, R, L, K, layout, what):
    """One call on the GPU and the same call under the simulator: the GPU's output as [B, L, K] after the guard, fill and
    word-for-word checks, and the cells compared."""
    B = len(per[0])
    n = B * L * K
    shape = (B, L, K) if layout == TC else (B, K, L)
    flat, out = _device_out(n)
    torch.cuda.synchronize()                                 # (the fill first, as above)
    gpu_fn(src_dev, *per, R, L, K, layout, out.view(shape))
    torch.cuda.synchronize()
    got = _written(flat, n, what).view(np.float32).reshape(shape)
    buf = np.full(n, NAN_FILL, dtype=np.uint32)
    sim_fn(src, *per, R, L, K, layout, buf)
    want = buf.view(np.float32).reshape(shape)
    if layout == CT:
        got, want = got.transpose(0, 2, 1), want.transpose(0, 2, 1)
    return got, _same_words(got, want, ("window", "sample", "channel"), what)


@pytest.mark.parametrize("C", (1, 3, 8))
def test_resample_windows_are_the_simulators_word_for_word(ctx, C):
    """clx_resample_windows on noise: up (16000 -> 44100: 441 phases; 44100 -> 48000), down (44100 -> 16000) and times two, with a
    copy beside them in the same call, one call per target, window length and layout."""
    for R, rates in TARGETS.items():
        src, xs, base = _sources(100 * C + R % 97, rates, C)
        src_dev = torch.from_numpy(src).to(DEV)
        for L in LENGTHS:
            per, which = _jobs(rates, R, C, L, base)
            valid = per[4]
            assert valid[0] == L and valid[1] > 0 and valid[3] == 0 and (L == 1 or 0 < valid[2] < L)
            for layout in (TC, CT):
                what = (rates, R, C, L, "ct" if layout == CT else "tc")
                got, cells = _both(ctx.resample_windows, sr.resample_windows, src, src_dev, per, R, L, C, layout, what)
                worst = 0.0
                for k, (i, st) in enumerate(which):
                    v = valid[k]
                    assert np.all(got[k, v:].view(np.uint32) == 0), (what, k, "the window's tail is not zeros")
                    if rates[i] == R:
                        assert np.array_equal(got[k, :v].view(np.uint32), xs[i][st:st + v].view(np.uint32)), (what, k, "not a copy")
                    elif v:
                        worst = max(worst, sr.assert_close(got[k, :v], xs[i], rates[i], R, np.arange(st, st + v), (what, k)))
                print("%r: worst |error| / bound %.4f; %d cells word for word, 0 differ" % (what, worst, cells))


@pytest.mark.parametrize("layout", (TC, CT))
def test_resample_windows_that_end_just_below_two_to_the_43(ctx, layout):
    """44100 -> 16000, two channels, three windows whose out_t0 + L is just below 2^43 at three phases: the block's one 64-bit
    product and quotient (software division on the device) at their largest, in the window's first tile and in its second.  Only the
    positions are large; the reference takes them as int64."""
    C, L, fs, R = 2, 1030, 44100, 16000
    src, per, xs = far_windows(43, C, L, fs, R)
    what = ("out_t0 + L just below 2^43", "ct" if layout == CT else "tc")
    got, cells = _both(ctx.resample_windows, sr.resample_windows, src, torch.from_numpy(src).to(DEV), per, R, L, C, layout, what)
    worst = max(sr.assert_close(got[k], x, fs, R, per[3][k] + np.arange(L, dtype=np.int64), (what, k), t0=per[1][k]) for k, x in enumerate(xs))
    print("%r: worst |error| / bound %.4f; %d cells word for word, 0 differ" % (what, worst, cells))


@pytest.mark.parametrize("Cs,K", ((2, 1), (3, 1), (8, 1), (1, 2), (1, 8)))
def test_mix_windows_under_resampling_are_the_simulators_word_for_word(ctx, Cs, K):
    """clx_mix_windows from 44100 to 16000: the mean of 2, 3 and 8 channels and a mono source copied to 2 and 8, the mix before the
    filter.  The float64 bound is the resampler's on the mixed signal (simlib_mix.mix: the mix is exact by definition)."""
    fs, R, L = 44100, SR, 1030
    src, xs, base = _sources(7 * Cs + K, (fs,), Cs)
    src_dev = torch.from_numpy(src).to(DEV)
    per, which = _jobs((fs,), R, Cs, L, base)
    per = per + ([Cs] * len(which),)
    valid, mixed = per[4], smx.mix(xs[0], K)
    outs = []
    for layout in (TC, CT):
        what = (Cs, K, L, "ct" if layout == CT else "tc")
        got, cells = _both(ctx.mix_windows, smx.mix_windows, src, src_dev, per, R, L, K, layout, what)
        worst = 0.0
        for k, (_, st) in enumerate(which):
            v = valid[k]
            assert np.all(got[k, v:].view(np.uint32) == 0), (what, k, "the window's tail is not zeros")
            if v:
                worst = max(worst, sr.assert_close(got[k, :v], mixed, fs, R, np.arange(st, st + v), (what, k)))
            for c in range(1, K):
                assert np.array_equal(got[k, :, c].view(np.uint32), got[k, :, 0].view(np.uint32)), (what, k, "replicated channels differ")
        print("%r: worst |error| / bound %.4f; %d cells word for word, 0 differ" % (what, worst, cells))
        outs.append(got)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "the layouts differ"


def test_a_16_khz_stream_read_at_44100(ctx):
    """Upsampling through StreamSet.read's planner: the 16 kHz stereo stream of test_gpu_resample read with sample_rate=44100, its
    windows at every frame boundary mapped to 44.1 kHz, across the end and behind it; the frames decoded are those of the formula's
    source span."""
    R, L = 44100, 100
    c = Case(ctx, *_stream(np.random.default_rng(2025), *STREAMS["c16"]), at=R)
    assert c.rate == 16000 and c.C == 2 and c.set.lengths_at(R).tolist() == [c.T_R] == [-(-c.T * 441 // 160)]
    starts = _starts(c, L)
    want_valid = [min(max(c.T_R - s, 0), L) for s in starts]
    assert want_valid[0] == L and 0 in want_valid and any(0 < v < L for v in want_valid)
    for layout in ("tc", "ct"):
        n0 = c.set.frames_decoded
        out, valid = c.set.read([0] * len(starts), starts, L, layout=layout, sample_rate=R)
        assert c.set.frames_decoded - n0 == sum(c.frames_for(s, L) for s in starts)
        assert out.shape == ((len(starts), L, 2) if layout == "tc" else (len(starts), 2, L)) and out.is_contiguous()
        assert valid.tolist() == want_valid
        h = out.cpu().numpy()
        for k, s in enumerate(starts):
            c.check(h[k] if layout == "tc" else np.ascontiguousarray(h[k].T), s, L, (layout, s))
    print("16000 -> 44100 through read(): worst |error| / bound %.4f" % c.worst)
