"""clx_mel_windows and clx_mix_windows queued without waiting, the way test_gpu_queued_calls.py queues the gather and the resampler:
some tens of milliseconds of matrix products on the stream first, then the calls back to back -- growing B (a larger table each
time), then the same B twice (the table reused), alternating between the current stream and a second one -- and one synchronise at
the end.  Every call has its own input and its own output inside guard words (gpu_guarded.py) and every output word is compared:
the mel calls with the same call made alone on a fresh context (two specs share the context's one table: a plain one, a word a
window, and a centred ranged one, three words a window, the third of which its kernels write), the mix calls with the wave
simulator's words.  Each test works out from the growth rule how often its calls replace the table."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_mix as sm
import simlib_resample as sr
from gpu_guarded import DEV, NAN_FILL, device_out, written
from test_gpu_queued_calls import _work_in_front

pytestmark = pytest.mark.gpu
TC, CT = cx.WINDOW_TC, cx.WINDOW_CT


@pytest.fixture
def ctx():
    """A context of the test's own: its tables start empty."""
    c = cx.Context(0, wait_s=120)
    yield c
    c.close()


def _mel_specs(c):
    """(the plain spec, the centred one) on context c."""
    return (cx.MelSpec(c, 16000, n_fft=64, hop=24, n_mels=13),
            cx.MelSpec(c, 16000, n_fft=64, hop=24, n_mels=13, mode="log10", center=True, top=8.0, shift=4.0, scale=0.25))


def test_mel_windows_queued_behind_pending_work(ctx):
    """B = 1 and 70 with the plain spec (1 and 70 words), 200 with the centred one (600 words): the table of w + w / 2 + 64 words is
    made for the first and replaced for the other two with launches pending on the tables they replace; then B = 50 twice, plain
    and centred, on the table of the 600."""
    n_frames, n_mels, L = 5, 13, 4 * 24 + 64
    rng = np.random.default_rng(47)
    calls = []
    for B, centred, layout in ((1, 0, TC), (70, 0, CT), (200, 1, TC), (50, 0, CT), (50, 1, CT)):
        audio = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(B, L)).astype(np.float32)).to(DEV)
        valid = rng.integers(L // 2, L + 1, size=B).astype(np.uint32)
        valid[0], valid[B // 2] = 0, L                       # (a window without a sample, unless it is the only one)
        calls.append((B, centred, layout, audio, valid, (B, n_frames, n_mels) if layout == TC else (B, n_mels, n_frames)))
    cap = grown = 0
    for B, centred in ((c[0], c[1]) for c in calls):
        w = 3 * B if centred else B
        if w > cap:
            cap, grown = w + w // 2 + 64, grown + 1
    assert grown == 3 and cap >= 150
    want = []
    for i, (B, centred, layout, audio, valid, shape) in enumerate(calls):       # each call alone, on a context that has made no other
        alone = cx.Context(0)
        spec = _mel_specs(alone)[centred]
        flat, out = device_out(B * n_frames * n_mels)
        torch.cuda.synchronize()
        alone.mel_windows(spec, audio, valid, n_frames, layout, out.view(shape))
        torch.cuda.synchronize()
        want.append(written(flat, B * n_frames * n_mels, ("alone", i, B, centred, layout)).copy())
        alone.close()
    specs = _mel_specs(ctx)
    outs = [device_out(c[0] * n_frames * n_mels) for c in calls]
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    done, _ = _work_in_front(side)
    pending = []
    for i, (B, centred, layout, audio, valid, shape) in enumerate(calls):
        ctx.mel_windows(specs[centred], audio, valid, n_frames, layout, outs[i][1].view(shape), stream=side if i % 2 else None)
        pending.append(not done.query())
    torch.cuda.synchronize()
    words = 0
    for i, (B, centred, layout, audio, valid, shape) in enumerate(calls):
        got = written(outs[i][0], B * n_frames * n_mels, ("call", i, B, centred, layout))
        bad = np.nonzero(got != want[i])[0]
        assert bad.size == 0, ("call", i, B, centred, layout, "%d words differ from the call alone; the first is word %d" % (bad.size, bad[0]))
        assert np.count_nonzero(got) > got.size // 4         # (most frames are live: the words are not all zeros)
        words += got.size
    print("mel queued: 5 calls of two specs, 2 table growths with launches pending, 2 reuses; the work in front was pending at the "
          "calls: %r; %d words compared with the calls alone, 0 differ" % (pending, words))


def _mix_call(rng, B, L, T, fs, R, bases):
    """B windows of two streams of T samples, a mono one (at float bases[0]) and a stereo one (bases[1]), in turn: at output 0,
    across the end, at the end, the rest anywhere up to a little behind the end."""
    T_R = sr.length_at(T, fs, R)
    st = rng.integers(0, T_R + 20, size=B)
    st[:4] = (0, T_R - L // 2, T_R - L // 2, T_R)
    per = ([], [], [], [], [], [], [])
    for k, s in enumerate(st.tolist()):
        Cs = 1 + k % 2
        v = min(max(T_R - s, 0), L)
        lo, hi = (0, 0) if v == 0 else sr.span(s, s + v - 1, T, fs, R)
        for lst, val in zip(per, (bases[Cs - 1] + lo * Cs, lo, hi - lo, s, v, fs, Cs)):
            lst.append(val)
    return per


def test_mix_windows_queued_behind_pending_work(ctx):
    """16000 -> 44100, mono and stereo sources to two channels.  A first call of B = 4 meets the rate pair (its coefficient upload is
    a blocking copy, which would wait for the work in front) and makes the table; then, behind the work, B = 120, 400 and 1600: with
    40 bytes a job, 32 for the two rate entries and a table of bytes + bytes / 2 + 4096, each of the three replaces the table
    before it."""
    fs, R, K, L, T = 16000, 44100, 2, 64, 3000
    rng = np.random.default_rng(53)
    src = np.concatenate([np.zeros(3, np.float32), rng.uniform(-1.0, 1.0, size=T * 3).astype(np.float32)])
    bases = (3, 3 + T)                                       # (the mono stream's T floats, then the stereo stream's 2 T)
    dev = torch.from_numpy(src).to(DEV)
    calls = []
    for i, B in enumerate((4, 120, 400, 1600)):
        layout = CT if i % 2 else TC
        flat, out = device_out(B * L * K)
        calls.append((B, layout, _mix_call(rng, B, L, T, fs, R, bases), flat, out))
    cap = grown = 0
    for B in (c[0] for c in calls):
        if 40 * B + 32 > cap:
            cap, grown = (40 * B + 32) * 3 // 2 + 4096, grown + 1
    assert grown == 4
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    B, layout, per, flat, out = calls[0]
    ctx.mix_windows(dev, *per, R, L, K, layout, out.view((B, L, K)))
    done, _ = _work_in_front(side)
    pending = []
    for i, (B, layout, per, flat, out) in enumerate(calls[1:]):
        ctx.mix_windows(dev, *per, R, L, K, layout, out.view((B, L, K) if layout == TC else (B, K, L)), stream=None if i % 2 else side)
        pending.append(not done.query())
    torch.cuda.synchronize()
    words = 0
    for i, (B, layout, per, flat, out) in enumerate(calls):
        got = written(flat, B * L * K, ("call", i, B, layout))
        want = np.full(B * L * K, NAN_FILL, dtype=np.uint32)
        sm.mix_windows(src, *per, R, L, K, layout, want)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, ("call", i, B, layout, "%d words differ from the simulator; the first is word %d" % (bad.size, bad[0]))
        assert np.count_nonzero(got) > got.size // 4         # (most windows lie inside the streams: the words are not all zeros)
        words += want.size
    print("mix queued: 1 + 3 calls, 3 table growths with launches pending; the work in front was pending at the calls: %r; "
          "%d words compared with the simulator, 0 differ" % (pending, words))
