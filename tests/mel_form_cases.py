"""The case matrix of the four newer mel kernels -- clx_k_mel_c (centred), clx_k_mel_f (framed), clx_k_mel_q (cepstral) and clx_k_mel_c
followed by clx_k_mel_range (ranged) --, shared by the wave simulator (test_mel_forms_sim.py) and the GPU (test_gpu_mel_forms.py).
A case names the form, the spec's shape, n_frames, the window length and the list of valid; it builds its noise batch from a fixed
seed (uniform in [-1, 1), zeros from valid[k] on), its tables by the formulas of simlib_mel / simlib_melk / simlib_melq, its float64
reference with the derived bound, and its simulator output.  What is built is kept per process and handed out read-only, so the
tests of a module share it.

The shapes are those at which the one templated body takes another path: a second pass of 256 bins (whole, partial, of one bin),
four and five passes, a K-slice with 14 live taps, hop > win_length, one tap, the shortest centred crop, a range step of two and
three tiles with a full, an empty and a ragged last tile, and valid_frames on every wave and group boundary."""
import numpy as np

import simlib_mel as sm
import simlib_melc as sc
import simlib_melk as sk
import simlib_melq as sq
from test_melc_sim import RANGES
from test_melk_sim import CONDS, _bank as melk_bank, _window as melk_window
from test_melq_sim import SHAPES as CEP_SHAPES, _bank as melq_bank

NAN_FILL = 0x7fc0dead            # a quiet NaN with a payload: what an output holds before the call
GUARD = 0xffc0beef               # the word behind a simulator output
SR = 16000
FLOOR = 1e-10
PRE = float(np.float32(0.97))
TC, CT = sm.TC, sm.CT
LAYOUTS = (CT, TC)
LAYOUT_NAMES = {CT: "ct", TC: "tc"}
PADS = {sc.PAD_REFLECT: "reflect", sc.PAD_ZERO: "zeros"}
OFFSETS = (0, 1, 2, 3)           # words behind a 16-byte boundary at which a ranged output starts
BOUNDARY_FRAMES = (0, 1, 8, 9, 31, 32, 33, 64, 65)           # valid_frames on the wave (8) and group (32) boundaries, n_frames = 65
ENERGY_SCALE = 2.0 ** 30


class Case:
    def __init__(self, form, name, **kw):
        self.form, self.name, self.layouts = form, name, LAYOUTS
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name

    @property
    def rows(self):
        return self.n_ceps if self.form == "cepstral" else self.n_mels

    @property
    def taps(self):
        return self.Nw if self.form in ("framed", "cepstral") else self.N


def _valids(values, L):
    return sorted(set(int(v) for v in values) & set(range(L + 1)))


# ---- the valid_frames rules and their inverses ------------------------------------------------------------------------------------

def valid_frames(case, valid=None):
    """valid_frames by the form's formula (simlib_mel / simlib_melc / simlib_melk), int64."""
    valid = case.valid if valid is None else valid
    if case.form in ("framed", "cepstral"):
        return sk.valid_frames(valid, case.Nw, case.H, case.T, case.whole)
    if case.center:
        return sc.valid_frames(valid, case.H, case.T, case.N // 2)
    return sm.valid_frames(valid, case.H, case.T)


def _boundary_valids(case):
    """One valid per valid_frames of BOUNDARY_FRAMES, by inverting the form's rule: the whole-frame rule gives vf for
    Nw + (vf - 1) H, the centred rule for vf H - P, the plain rule for vf H.  A centred spec with P > H has no valid that gives fewer
    than ceil((1 + P) / H) frames but 0; such a count is asserted to be out of reach and left out.  Every valid is asserted to land
    on the count it was chosen for."""
    out = []
    for vf in BOUNDARY_FRAMES:
        if vf == 0:
            v = 0
        elif case.form in ("framed", "cepstral"):
            v = case.Nw + (vf - 1) * case.H
        elif case.center:
            v = vf * case.H - case.N // 2
            if v < 1:
                assert int(valid_frames(case, [1])[0]) > vf, (case, vf)
                continue
        else:
            v = vf * case.H
        assert 0 <= v <= case.L and int(valid_frames(case, [v])[0]) == vf, (case, vf, v)
        out.append(v)
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------

def _centred_cases():
    out = []
    # (n_fft, hop, n_mels), n_frames: J = 301, two passes, the second partial; J = 257, the second pass holds one bin; hop > n_fft;
    # five passes (three windows only: the simulator is slow there)
    for (N, H, M), T in (((600, 200, 40), 33), ((512, 128, 64), 33), ((16, 40, 3), 33), ((2048, 512, 128), 9)):
        P = N // 2
        for L in [T * H] + ([(T - 1) * H + N - 2 * P] if N < 2048 else []):
            vals = (0, L // 2, L) if N == 2048 else (0, 1, P, L // 2, L - 1, L)
            for pad in PADS:
                out.append(Case("centred", "c%dx%dx%d-T%d-L%d-%s" % (N, H, M, T, L, PADS[pad]), N=N, H=H, n_mels=M, T=T, L=L, pad=pad, center=1,
                                valid=_valids(vals, L), seed=N + T + L))
    N, H, M, T, L = 50, 7, 5, 4, 26                          # L = P + 1, the shortest crop: frame 3 reflects about both ends
    assert L == N // 2 + 1 and 3 * H - N // 2 < 0 and 3 * H - N // 2 + N - 1 >= L
    for pad in PADS:
        out.append(Case("centred", "c50x7x5-T4-L26-%s" % PADS[pad], N=N, H=H, n_mels=M, T=T, L=L, pad=pad, center=1,
                        valid=_valids((0, 1, N // 2, L // 2, L - 1, L), L), seed=N + T + L))
    for pad in PADS:
        c = Case("centred", "c50x7x5-T65-boundaries-%s" % PADS[pad], N=50, H=7, n_mels=5, T=65, L=65 * 7, pad=pad, center=1, seed=65)
        c.valid = _boundary_valids(c)
        assert len(c.valid) == len(BOUNDARY_FRAMES) - 1      # (a count of 1 is out of reach: P > H)
        out.append(c)
    return out


def _framed_cases():
    out = []
    # (win_length, n_fft, hop, n_mels, n_bins), n_frames, sample rate: two full passes; the second pass holds one bin; 4 passes and 69
    # K-slices, the last with 14 live taps; hop > win_length; one tap
    shapes = (((600, 1024, 200, 40, 512), 33, SR), ((600, 1024, 200, 40, 257), 33, SR), ((1102, 2048, 441, 80, 1024), 9, 44100),
              ((7, 16, 40, 3, 8), 33, SR), ((1, 2, 1, 1, 1), 33, SR))
    for (Nw, N, H, M, J), T, rate in shapes:
        L = (T - 1) * H + Nw
        vals = (0, L // 2, L) if N == 2048 else (0, 1, Nw - 1, Nw, Nw + H, L // 2, L)
        for dc, c in CONDS:
            case = Case("framed", "f%dx%dx%dx%dx%d-T%d-dc%d-c%s" % (Nw, N, H, M, J, T, dc, c), Nw=Nw, N=N, H=H, n_mels=M, n_bins=J, T=T, L=L,
                        rate=rate, dc=dc, c=c, whole=1, valid=_valids(vals, L), seed=Nw + T)
            if N == 2048 and not (dc and c):
                case.layouts = (TC,)
            out.append(case)
    Nw, N, H, M, J, T = 600, 1024, 200, 40, 512, 33          # frames that hang past valid are computed over zeros
    L = (T - 1) * H + Nw
    out.append(Case("framed", "f600x1024x200x40x512-T33-dc1-c0.97-part", Nw=Nw, N=N, H=H, n_mels=M, n_bins=J, T=T, L=L, rate=SR, dc=1, c=0.97,
                    whole=0, valid=_valids((0, 1, Nw - 1, Nw, Nw + H, L // 2, L), L), seed=Nw + T + 1))
    Nw, N, H, M, J, T = 25, 32, 10, 5, 16, 65
    c = Case("framed", "f25x32x10x5x16-T65-boundaries", Nw=Nw, N=N, H=H, n_mels=M, n_bins=J, T=T, L=(T - 1) * H + Nw, rate=SR, dc=1, c=0.97,
             whole=1, seed=65)
    c.valid = _boundary_valids(c)
    assert len(c.valid) == len(BOUNDARY_FRAMES)
    out.append(c)
    return out


def _cepstral_cases():
    out = []
    T = 33
    for Nw, N, H, M, J, n_ceps in CEP_SHAPES:
        if M == 128:
            n_ceps = 128                                     # both limits at once: 16 band cells and 16 output cells in every lane
        L = (T - 1) * H + Nw
        for lifter in (1, 0):
            out.append(Case("cepstral", "q%dx%dx%dx%dx%dx%d-T%d-%s" % (Nw, N, H, M, J, n_ceps, T, "lifter" if lifter else "plain"), Nw=Nw, N=N,
                            H=H, n_mels=M, n_bins=J, n_ceps=n_ceps, T=T, L=L, rate=SR, dc=1, c=0.97, whole=1, lifter=lifter, energy=0,
                            valid=_valids((0, 1, Nw - 1, Nw, Nw + H, L // 2, L), L), seed=Nw + M))
    e = _copy(next(c for c in out if c.name.startswith("q25x32x10x5x16x5") and c.lifter), "q25x32x10x5x16x5-T33-lifter-energy", energy=1)
    out.append(e)
    Nw, N, H, M, J, n_ceps, T = 25, 32, 10, 5, 16, 5, 65
    c = Case("cepstral", "q25x32x10x5x16x5-T65-boundaries", Nw=Nw, N=N, H=H, n_mels=M, n_bins=J, n_ceps=n_ceps, T=T, L=(T - 1) * H + Nw, rate=SR,
             dc=1, c=0.97, whole=1, lifter=1, energy=0, seed=66)
    c.valid = _boundary_valids(c)
    assert len(c.valid) == len(BOUNDARY_FRAMES)
    out.append(c)
    return out


def _copy(case, name, **kw):
    c = Case(case.form, name)
    c.__dict__.update({k: v for k, v in case.__dict__.items() if k != "name"})
    c.__dict__.update(kw)
    return c


def without_energy(case):
    """The same spec and batch without the energy row."""
    twin = next(c for c in CEPSTRAL if not c.energy and c.lifter == case.lifter and c.T == case.T and
                (c.Nw, c.N, c.H, c.n_mels, c.n_bins, c.n_ceps) == (case.Nw, case.N, case.H, case.n_mels, case.n_bins, case.n_ceps))
    assert twin.seed == case.seed and twin.valid == case.valid
    return twin


def _ranged_cases():
    out = []
    # (n_fft, hop, n_mels), n_frames, centred: 4096 cells, one tile exactly full and a second that is empty or holds the ragged tail,
    # depending on the offset; 4104 cells, two tiles; 4500 cells, two tiles and an odd count, so that windows 1.. start off the
    # 16-byte grid whatever the offset; 8200 cells, three tiles behind a two-pass launch
    for (N, H, M), T, center in (((50, 7, 8), 512, 1), ((50, 7, 8), 513, 0), ((50, 7, 5), 900, 1), ((600, 200, 40), 205, 1)):
        L = T * H if center else (T - 1) * H + N
        out.append(Case("ranged", "r%dx%dx%d-T%d-%s" % (N, H, M, T, "centred" if center else "plain"), N=N, H=H, n_mels=M, T=T, L=L,
                        center=center, pad=sc.PAD_REFLECT, seed=N + T, boundaries=0))
    c = Case("ranged", "r50x7x5-T65-boundaries", N=50, H=7, n_mels=5, T=65, L=64 * 7 + 50, center=0, pad=sc.PAD_REFLECT, seed=67, boundaries=1)
    c.valid = _boundary_valids(c) + [c.L]                    # (the last window is zeros, live to its end)
    assert len(c.valid) == len(BOUNDARY_FRAMES) + 1
    out.append(c)
    return out


CENTRED, FRAMED, CEPSTRAL, RANGED = _centred_cases(), _framed_cases(), _cepstral_cases(), _ranged_cases()
POWER_CASES = CENTRED + FRAMED + CEPSTRAL
ENERGY_CASES = [c for c in CEPSTRAL if c.energy]
ZERO_PAD_CASES = [c for c in CENTRED if c.pad == sc.PAD_ZERO]
# the multi-pass centred and framed cases, for the log modes (the three conditionings share the last step: one of them)
LOG_CASES = [c for c in CENTRED if c.N // 2 + 1 > 256 and c.L == c.T * c.H] + [c for c in FRAMED if c.n_bins > 256 and c.dc and c.c and c.whole]
TWO_PASS_400 = [c for c in CEPSTRAL if c.Nw == 400]           # the shapes whose cepstral bound is held to be narrow


def with_layouts(cases):
    """(case, layout) for pytest.mark.parametrize, with readable ids."""
    pairs = [(c, layout) for c in cases for layout in c.layouts]
    return dict(argvalues=pairs, ids=["%s-%s" % (c.name, LAYOUT_NAMES[layout]) for c, layout in pairs])


# ---- batches and tables -----------------------------------------------------------------------------------------------------------

_MADE = {}


def _once(key, make):
    if key not in _MADE:
        made = make()
        for a in made if isinstance(made, tuple) else (made,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _MADE[key] = made
    return _MADE[key]


def _ranged_batch(case):
    """test_melc_sim._ranged_batch for any frame count: the loudest frames in the last frame group; in the first; some frames dead
    (valid inside); valid = 0; a window of zeros that is live to its end."""
    N, H, T, L = case.N, case.H, case.T, case.L
    rng = np.random.default_rng(case.seed)
    a = (1e-3 * rng.uniform(-1.0, 1.0, size=(5, L))).astype(np.float32)
    last = 32 * ((T - 1) // 32)                              # the first frame of the last group
    loud = (last - 1) * H + (N // 2 if case.center else N)   # (behind every tap of the frames in front of it)
    a[0, loud:] = rng.uniform(-1.0, 1.0, size=L - loud).astype(np.float32)
    a[1, :N] = rng.uniform(-1.0, 1.0, size=N).astype(np.float32)
    a[2] = rng.uniform(-1.0, 1.0, size=L).astype(np.float32)
    a[4] = 0.0
    valid = np.array([L, L, L // 3, 0, L], dtype=np.uint32)
    for k, v in enumerate(valid):
        a[k, v:] = 0.0
    return a, valid


def batch(case):
    """(audio [B, L] float32, valid uint32), read-only: uniform noise in [-1, 1) from the case's seed, zeros from valid[k] on."""
    def make():
        if case.form == "ranged" and not case.boundaries:
            return _ranged_batch(case)
        valid = np.array(case.valid, dtype=np.uint32)
        a = np.random.default_rng(case.seed).uniform(-1.0, 1.0, size=(valid.size, case.L)).astype(np.float32)
        for k, v in enumerate(valid):
            a[k, v:] = 0.0
        if case.form == "ranged":
            a[-1] = 0.0
        return a, valid
    return _once(("batch", case.name), make)


def nan_tailed(case):
    """The batch with NaN in place of the zeros from valid[k] on."""
    a, valid = batch(case)
    b = a.copy()
    for k, v in enumerate(valid):
        b[k, v:] = np.nan
    assert np.any(np.isnan(b))
    return b


def tables(case):
    """The spec's tables as float32, read-only: (window, fbank) and, for a cepstral case, (.., dct, lifter or None)."""
    def make():
        if case.form in ("centred", "ranged"):
            return sm.hann(case.N), sm.triangles(SR, case.N, case.n_mels)
        Nw, N, M, J = case.Nw, case.N, case.n_mels, case.n_bins
        if case.form == "cepstral":
            w, fb = melk_window(Nw), melq_bank(N, M, J)
            D = sq.dct_kaldi(case.n_ceps, M).astype(np.float32)
            return w, fb, D, (sq.lifter_kaldi(case.n_ceps).astype(np.float32) if case.lifter else None)
        if Nw <= 7:                                          # (the bank builder of test_melk_sim: n_bins and the bank's columns agree)
            return melk_window(Nw), melk_bank(N, M, J)
        w = (sk.kaldi_window("povey", Nw) * 32768.0).astype(np.float32)
        return w, np.ascontiguousarray(sk.kaldi_fbank(case.rate, N, M).astype(np.float32)[:, :J])
    made = _once(("tables", case.form, case.taps, case.N, case.n_mels, getattr(case, "n_bins", 0), getattr(case, "rate", SR),
                  getattr(case, "n_ceps", 0), getattr(case, "lifter", 0)), make)
    assert made[0].shape == (case.taps,) and made[1].shape == (case.n_mels, getattr(case, "n_bins", case.N // 2 + 1))
    return made


def reference(case):
    """(X64, dX), each [B, T, rows] float64, read-only: the power-mode definition in float64 and the bound that holds for a float32
    evaluation in any order -- simlib_mel.reference on the host-padded batch (centred), simlib_melk.reference (framed),
    simlib_melq.reference_power (cepstral; with the energy on, row 0 is not the cepstrum's and must not be compared)."""
    def make():
        a, _ = batch(case)
        t = tables(case)
        if case.form == "centred":
            return sm.reference(sc.pad_batch(a, case.N // 2, case.pad), t[0], t[1], case.N, case.H, case.T)
        if case.form == "framed":
            return sk.reference(a, t[0], t[1], case.N, case.H, case.T, case.dc, case.c)
        return sq.reference_power(a, t[0], t[1], case.N, case.H, case.T, case.dc, case.c, t[2], t[3])
    return _once(("reference", case.name), make)


def check_bound(got, case, what, first_row=0):
    """got [B, T, rows] float32 in power mode: every frame past valid_frames is the word 0, every live cell lies within the bound of
    the float64 reference.  Returns (worst |error| / bound, live cells compared)."""
    X64, dX = reference(case)
    vf = valid_frames(case)
    worst, cells = 0.0, 0
    for k in range(got.shape[0]):
        assert np.all(got[k, vf[k]:].view(np.uint32) == 0), (what, k, "a frame past valid_frames is not the word 0")
        live = got[k, :vf[k], first_row:].astype(np.float64)
        ref, bound = X64[k, :vf[k], first_row:], dX[k, :vf[k], first_row:]
        err = np.abs(live - ref)
        bad = np.argwhere(~(err <= bound))
        assert bad.size == 0, (what, "window %d frame %d row %d: %r, expected %r, bound %.3g" % (
            k, bad[0][0], bad[0][1] + first_row, live[tuple(bad[0])], ref[tuple(bad[0])], bound[tuple(bad[0])]))
        if live.size:
            worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
            cells += live.size
    return worst, cells


# ---- the simulator ----------------------------------------------------------------------------------------------------------------

def _sim_spec(case, mode, ranged=None):
    """(module, handle) of the case's spec under the simulator."""
    t = tables(case)
    if case.form in ("centred", "ranged"):
        opts = dict(center=case.center, pad=case.pad)
        if ranged is not None:
            opts.update(range=1, range_width=ranged[0], shift=ranged[1], scale=ranged[2])
        return sc, sc.create(case.N, case.H, t[0], t[1], case.n_mels, mode, FLOOR, opts)
    opts = dict(remove_dc=case.dc, preemph=case.c, whole_frames=case.whole)
    if case.form == "framed":
        h = sk.create(case.N, case.Nw, case.H, t[0], t[1], case.n_bins, case.n_mels, mode, FLOOR, opts)
        assert sk.kernel(h) == "clx_k_mel_f"
        return sk, h
    cep = dict(n_ceps=case.n_ceps, dct=t[2], lifter=t[3], energy=case.energy, energy_scale=ENERGY_SCALE)
    h = sq.create(case.N, case.Nw, case.H, t[0], t[1], case.n_bins, case.n_mels, mode, FLOOR, opts, cep)
    assert sq.kernel(h) == "clx_k_mel_q" and sq.rows(h) == case.n_ceps
    return sq, h


def _sim_call(mod, h, case, audio, layout, offset):
    """One call: the output [B, T, rows] float32 (a copy), valid_frames and what else the module's tables=True returns.  The batch
    sits between NaNs at an odd 4-byte alignment; the output starts `offset` words behind a 16-byte boundary as a NaN pattern with
    four words of the pattern in front and a guard word behind: those stay, and no output word keeps the pattern."""
    _, valid = batch(case)
    B, rows, T = audio.shape[0], case.rows, case.T
    n = B * rows * T
    raw = np.full(n + 16, NAN_FILL, dtype=np.uint32)
    at = (-(raw.ctypes.data // 4)) % 4 + 4 + offset
    buf = raw[at:at + n + 1]
    buf[n] = GUARD
    src = np.full(audio.size + 16, np.nan, dtype=np.float32)
    src[7:7 + audio.size] = audio.reshape(-1)
    res = mod.mel_windows(h, src[7:7 + audio.size].reshape(audio.shape), valid, T, layout, buf, tables=True)
    assert buf[n] == GUARD and np.all(raw[:at] == NAN_FILL) and np.all(raw[at + n + 1:] == NAN_FILL), (case, "a word outside the output was written")
    left = int(np.count_nonzero(buf[:n] == NAN_FILL))
    assert left == 0, (case, "%d of %d output words still hold the fill pattern" % (left, n))
    out = buf[:n].view(np.float32)
    out = out.reshape(B, rows, T).transpose(0, 2, 1) if layout == CT else out.reshape(B, T, rows)
    return (np.ascontiguousarray(out),) + tuple(res[1:])


def sim(case, layout, mode=sm.POWER, nan_tail=False):
    """(out [B, T, rows] float32, valid_frames) of a centred, framed or cepstral case under the simulator, read-only; the output
    sits one word behind a 16-byte boundary."""
    def make():
        mod, h = _sim_spec(case, mode)
        try:
            res = _sim_call(mod, h, case, nan_tailed(case) if nan_tail else batch(case)[0], layout, 1)
        finally:
            mod.destroy(h)
        return res[0], res[1]
    return _once(("sim", case.name, layout, mode, nan_tail), make)


def sim_unranged(case, mode):
    """The unranged output [B, T, n_mels] of a ranged case's shape in its log mode (TC), as the simulator wrote it."""
    def make():
        mod, h = _sim_spec(case, mode)
        try:
            return _sim_call(mod, h, case, batch(case)[0], TC, 0)[:2]
        finally:
            mod.destroy(h)
    return _once(("unranged", case.name, mode), make)


def sim_ranged(case, mode, ranged):
    """A generator of (layout, offset, out, valid_frames, wmax) over both layouts and the four offsets of one ranged spec."""
    mod, h = _sim_spec(case, mode, ranged)
    try:
        for layout in LAYOUTS:
            for offset in OFFSETS:
                yield (layout, offset) + _sim_call(mod, h, case, batch(case)[0], layout, offset)
    finally:
        mod.destroy(h)


def ranged_want(u, vf, y0, ranged):
    """float32 numpy on the unranged output u [B, T, n_mels]: the dead frames take y0, then max(y, max_k - D), + shift, * scale, each
    rounded once.  Returns (want, the windows' maxima)."""
    u = u.copy()
    for k in range(u.shape[0]):
        u[k, vf[k]:] = y0
    mx = u.reshape(u.shape[0], -1).max(axis=1)
    D, shift, scale = (np.float32(x) for x in ranged)
    lo = (mx - D).astype(np.float32)
    want = ((np.maximum(u, lo[:, None, None]) + shift).astype(np.float32) * scale).astype(np.float32)
    return want, mx


def same_words(got, want, what, other="the simulator"):
    """got and want ([B, T, rows] float32) as 32-bit words; returns the cells compared."""
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    if bad.size:
        at = tuple(int(i) for i in bad[0])
        raise AssertionError("%r: %d of %d cells differ from %s; the first is window %d, frame %d, row %d: 0x%08x (%r), expected 0x%08x (%r)" % (
            what, bad.shape[0], g.size, other, at[0], at[1], at[2], int(g[at]), float(got[at]), int(w[at]), float(want[at])))
    return int(g.size)


def energy_ulps(got, case):
    """The error of row 0 of got [B, T, n_ceps] in the live frames, in float32 ulps of log_energy64(energy32(..)) -- the energy
    emulated in the kernel's lane order, its logarithm in float64."""
    a, _ = batch(case)
    vf = valid_frames(case)
    le64 = _once(("energy", case.name), lambda: sq.log_energy64(sq.energy32(sk.frames_of(a, case.Nw, case.H, case.T), bool(case.dc), ENERGY_SCALE)))
    return np.concatenate([sq.ulps_of(got[k, :vf[k], 0], le64[k, :vf[k]]).reshape(-1) for k in range(got.shape[0])])
