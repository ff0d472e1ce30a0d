"""clx_gather_windows and clx_resample_windows queued without waiting, as a data loader issues them: the calls are asynchronous, share
one pinned staging table and one device table per context, hand them over with two events and, when a call needs a larger table,
replace it while the earlier launches may still read the old one.  Each test puts some tens of milliseconds of matrix products on
the stream first, so that everything issued after them is pending while the host goes on, then issues its calls back to back --
growing B (a larger table each time), then the same B twice (the table reused), alternating between the current stream and a
second one -- and synchronises once at the end.  Every call has its own source offsets and its own output inside guard words
(gpu_guarded.py); every output word is compared, with numpy's slices for the gather and with the wave simulator's words for the
resampler (test_gpu_float_parity.py holds the two to each other call by call).  The simulator cannot run this host code at all."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_resample as sr
import window_cases as wc
from gpu_guarded import DEV, NAN_FILL, device_out, written

pytestmark = pytest.mark.gpu
TC, CT = cx.WINDOW_TC, cx.WINDOW_CT


@pytest.fixture
def ctx():
    """A context of the test's own: its tables start empty."""
    c = cx.Context(0, wait_s=120)
    yield c
    c.close()


def _work_in_front(side):
    """A few large matrix products on the current stream, `side` behind them; returns an event behind the products."""
    a = torch.randn(8192, 8192, device=DEV)
    (a @ a).sum().item()                                     # (the library's first call: loaded and tuned before the clock matters)
    torch.cuda.synchronize()
    for _ in range(4):
        b = a @ a
    done = torch.cuda.Event()
    done.record()
    side.wait_stream(torch.cuda.current_stream())
    return done, b


def test_gather_windows_queued_behind_pending_work(ctx):
    """B = 1, 70, 200, 1000: the table of n + n / 2 + 64 entries is made for 1 and replaced for 70, 200 and 1000 (three growths with
    launches pending on the tables they replace), then B = 50 twice on the table of the 1000."""
    rng = np.random.default_rng(41)
    n_src = 1 << 16
    src = wc.source(rng, n_src)
    dev = torch.from_numpy(src.view(np.float32)).to(DEV)
    calls = []
    for B, L, C, layout in ((1, 257, 2, TC), (70, 64, 3, CT), (200, 100, 8, CT), (1000, 65, 2, CT), (50, 256, 5, TC), (50, 1000, 2, CT)):
        first = rng.integers(0, n_src - L * C, size=B)
        valid = rng.integers(0, L + 1, size=B)
        valid[0] = L
        flat, out = device_out(B * L * C)
        calls.append((B, L, C, layout, first, valid, flat, out))
    cap = grown = 0
    for B in (c[0] for c in calls):
        if B > cap:
            cap, grown = B + B // 2 + 64, grown + 1
    assert grown == 4 and cap >= 50
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    done, _ = _work_in_front(side)
    pending = []
    for i, (B, L, C, layout, first, valid, flat, out) in enumerate(calls):
        ctx.gather_windows(dev, first, valid, L, C, layout, out, stream=side if i % 2 else None)
        pending.append(not done.query())
    torch.cuda.synchronize()
    words = 0
    for i, (B, L, C, layout, first, valid, flat, out) in enumerate(calls):
        got = written(flat, B * L * C, ("call", i, B, L, C, layout))
        want = wc.expect(src, first, valid, L, C, layout).reshape(-1)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, ("call", i, B, L, C, layout, "%d words differ; the first is word %d" % (bad.size, bad[0]))
        words += want.size
    print("gather queued: 6 calls, 3 table growths with launches pending, 2 reuses; the work in front was pending at the calls: %r; "
          "%d words compared with numpy, 0 differ" % (pending, words))


def _rs_call(rng, B, L, C, T, fs, R, base):
    """B windows of the one stream: at output 0, across the end, at the end, the rest anywhere up to a little behind the end."""
    T_R = sr.length_at(T, fs, R)
    st = rng.integers(0, T_R + 20, size=B)
    st[:3] = (0, T_R - L // 2, T_R)
    per = ([], [], [], [], [], [])
    for s in st.tolist():
        v = min(max(T_R - s, 0), L)
        lo, hi = (0, 0) if v == 0 else sr.span(s, s + v - 1, T, fs, R)
        for lst, val in zip(per, (base + lo * C, lo, hi - lo, s, v, fs)):
            lst.append(val)
    return per


def test_resample_windows_queued_behind_pending_work(ctx):
    """16000 -> 44100, two channels.  A first call of B = 4 meets the rate pair (its coefficient upload is a blocking copy, which
    would wait for the work in front) and makes the table; then, behind the work, B = 120, 400, 1600 and 4000: with 40 bytes a job,
    32 for the two rate entries and a table of bytes + bytes / 2 + 4096, each of the four replaces the table before it."""
    fs, R, C, L, T = 16000, 44100, 2, 64, 3000
    rng = np.random.default_rng(43)
    src = np.concatenate([np.zeros(3, np.float32), rng.uniform(-1.0, 1.0, size=T * C).astype(np.float32)])
    dev = torch.from_numpy(src).to(DEV)
    calls = []
    for i, B in enumerate((4, 120, 400, 1600, 4000)):
        layout = CT if i % 2 else TC
        flat, out = device_out(B * L * C)
        calls.append((B, layout, _rs_call(rng, B, L, C, T, fs, R, 3), flat, out))
    cap = grown = 0
    for B in (c[0] for c in calls):
        if 40 * B + 32 > cap:
            cap, grown = (40 * B + 32) * 3 // 2 + 4096, grown + 1
    assert grown == 5
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    B, layout, per, flat, out = calls[0]
    ctx.resample_windows(dev, *per, R, L, C, layout, out.view((B, L, C)))
    done, _ = _work_in_front(side)
    pending = []
    for i, (B, layout, per, flat, out) in enumerate(calls[1:]):
        ctx.resample_windows(dev, *per, R, L, C, layout, out.view((B, L, C) if layout == TC else (B, C, L)), stream=None if i % 2 else side)
        pending.append(not done.query())
    torch.cuda.synchronize()
    words = 0
    for i, (B, layout, per, flat, out) in enumerate(calls):
        got = written(flat, B * L * C, ("call", i, B, layout))
        want = np.full(B * L * C, NAN_FILL, dtype=np.uint32)
        sr.resample_windows(src, *per, R, L, C, layout, want)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, ("call", i, B, layout, "%d words differ from the simulator; the first is word %d" % (bad.size, bad[0]))
        assert np.count_nonzero(got) > got.size // 4         # (most windows lie inside the stream: the words are not all zeros)
        words += want.size
    print("resample queued: 1 + 4 calls, 4 table growths with launches pending; the work in front was pending at the calls: %r; "
          "%d words compared with the simulator, 0 differ" % (pending, words))
