"""clx_norm_windows, clx_add_windows, clx_reverb_windows, clx_reverb_windows_fft and clx_specaug_windows queued without waiting
across two streams, the way test_gpu_queued_calls.py queues the gather and the resampler: some tens of milliseconds of matrix
products on the stream first, then the calls of one context back to back, the current stream and a second one in turn, and one
synchronise at the end.  These five sets carry device-only buffers beside the table (the double partial sums; the FFT reverb's
workspace too), and a call may replace any of them while earlier launches are pending; on one stream the stream's own order makes
every answer right, so only calls on two streams can see a wait that clx_call_scratch (clx_api.hip) leaves out.  Each test works
out from the growth rules -- a table of need + need / 2 + slack units, p + p / 2 + 64 partial sums, a workspace of b + b / 2 bytes
-- how often its calls replace each buffer, and asserts that before it launches.  Every call has its own inputs and its own
outputs inside guard words (gpu_guarded.py), and every output word is compared: with the wave simulator's words where the
simulator runs the call in well under a second (`sim` in the call), else with the same call made alone on a context that has made
no other, synchronised before and after (the per-kernel GPU tests hold the device to the simulator call by call).  The expected
words never come from the context under test.  The simulator cannot run this host code at all.
The summary line says at which calls the work in front was still pending.  A call that keeps its table first waits on the host for
the upload before it, and that upload stands behind the work in front: from the first such call of a test on the list reads False
whatever the size of that work (20 products of 8192 x 8192 floats in place of the 4 gave the same lists on an MI355X), and what
is pending at those calls is the launches of the calls before them, microseconds old."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import simlib_add as sa
import simlib_norm as sn
import simlib_reverb as sr
import simlib_reverb_fft as sf
import simlib_specaug as ss
from gpu_guarded import DEV, NAN_FILL, device_out, written
from test_gpu_queued_calls import _work_in_front

pytestmark = pytest.mark.gpu
TC, CT = cx.WINDOW_TC, cx.WINDOW_CT
CHUNK = 4096                             # cells of the time axis behind one partial sum (clx_norm's and clx_add's)


@pytest.fixture
def ctx():
    """A context of the test's own: its tables start empty."""
    c = cx.Context(0, wait_s=120)
    yield c
    c.close()


def _made(needs, slack):
    """(how often the calls make or replace a buffer, its last capacity): a need above the capacity makes one of
    need + need / 2 + slack; None is a call that does not reserve the buffer."""
    cap = n = 0
    for need in needs:
        if need is not None and need > cap:
            cap, n = need + need // 2 + slack, n + 1
    return n, cap


def _shape(c):
    return (c["B"], c["T"], c["rows"]) if c["layout"] == TC else (c["B"], c["rows"], c["T"])


def _batch(rng, c, offset=0.0):
    """The call's batch in its layout, float32: unit normals with a scale and an offset per row."""
    B, rows, T = c["B"], c["rows"], c["T"]
    x = rng.standard_normal((B, rows, T), dtype=np.float32) * rng.uniform(0.5, 3.0, (B, rows, 1)).astype(np.float32) \
        + rng.uniform(-2.0, 2.0, (B, rows, 1)).astype(np.float32) + np.float32(offset)
    return np.ascontiguousarray(x.transpose(0, 2, 1)) if c["layout"] == TC else x


def _valid(rng, B, T, least=0):
    """Anything from `least` to T; the first window whole, and a window without a live cell where there are three."""
    v = rng.integers(least, T + 1, size=B).astype(np.uint32)
    v[0] = T
    if B > 2:
        v[B // 2] = 0
    return v


def _u32(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _filled(shape):
    """A host output that holds the fill pattern, for the simulator to write."""
    return np.full(shape, NAN_FILL, dtype=np.uint32).view(np.float32)


class _Norm:
    """clx_norm_windows, in place, with var; `stats` in some calls."""
    norm = cx.Norm(True, True, 0, 1e-7, -1.0)

    @staticmethod
    def case(rng, B, rows, T, layout, stats, sim):
        c = dict(B=B, rows=rows, T=T, layout=layout, stats=stats, sim=sim)
        c["valid"] = _valid(rng, B, T)
        c["x"] = _batch(rng, c)
        return c

    @staticmethod
    def make(c):
        flat, body = device_out(c["x"].size)
        body.copy_(torch.from_numpy(c["x"].reshape(-1)))
        return dict(flat=flat, body=body, stats=device_out(c["B"] * c["rows"] * 2) if c["stats"] else None)

    @classmethod
    def queue(cls, ctx, c, b, stream):
        ctx.norm_windows(b["body"].view(_shape(c)), c["valid"], c["layout"], cls.norm,
                         stats=b["stats"][1].view(c["B"], c["rows"], 2) if c["stats"] else None, stream=stream)

    @staticmethod
    def words(c, b, what):
        out = [written(b["flat"], c["x"].size, what + ("cells",))]
        return out + ([written(b["stats"][0], c["B"] * c["rows"] * 2, what + ("stats",))] if c["stats"] else [])

    @classmethod
    def sim(cls, c):
        a, st = c["x"].copy(), _filled((c["B"], c["rows"], 2))
        sn.norm_windows(a, c["valid"], c["layout"], sn.of_norm(cls.norm), st)
        return [_u32(a)] + ([_u32(st)] if c["stats"] else [])


class _Add:
    """clx_add_windows, in place; every call reads the one noise tensor (NOISE windows of ROWS x T cells, taken in the call's
    layout), some windows have no noise, `gains` in some calls."""
    ROWS, T, NOISE = 2, 100, 5
    noise_valid = np.array([100, 0, 30, 100, 77], dtype=np.uint32)
    noise = np.random.default_rng(59).standard_normal((NOISE, ROWS * T), dtype=np.float32)
    d_noise = None                       # the test's device copy

    @classmethod
    def case(cls, rng, B, layout, gains, sim):
        c = dict(B=B, rows=cls.ROWS, T=cls.T, layout=layout, gains=gains, sim=sim)
        c["valid"] = _valid(rng, B, cls.T)
        c["index"] = rng.integers(-1, cls.NOISE, size=B).astype(np.int32)
        c["index"][0], c["index"][1::7] = 0, -1               # (the first window has a noise, so every call has work; some have none)
        c["snr"] = rng.uniform(-5.0, 20.0, size=B).astype(np.float32)
        c["x"] = _batch(rng, c)
        return c

    @staticmethod
    def make(c):
        flat, body = device_out(c["x"].size)
        body.copy_(torch.from_numpy(c["x"].reshape(-1)))
        return dict(flat=flat, body=body, gains=device_out(c["B"]) if c["gains"] else None)

    @classmethod
    def queue(cls, ctx, c, b, stream):
        ctx.add_windows(b["body"].view(_shape(c)), c["valid"], cls.d_noise.view((cls.NOISE,) + _shape(c)[1:]), cls.noise_valid, c["index"],
                        c["snr"], c["layout"], gains=b["gains"][1] if c["gains"] else None, stream=stream)

    @staticmethod
    def words(c, b, what):
        out = [written(b["flat"], c["x"].size, what + ("cells",))]
        return out + ([written(b["gains"][0], c["B"], what + ("gains",))] if c["gains"] else [])

    @classmethod
    def sim(cls, c):
        a, g = c["x"].copy(), _filled((c["B"],))
        assert sa.add_windows(a, c["valid"], cls.noise.reshape((cls.NOISE,) + _shape(c)[1:]), cls.noise_valid, c["index"], c["snr"], c["layout"], g)
        return [_u32(a)] + ([_u32(g)] if c["gains"] else [])


class _Reverb:
    """clx_reverb_windows and clx_reverb_windows_fft (c["fft"]), out of place: the data and the responses keep their words; some
    windows have no response, `gains` in some calls."""

    @staticmethod
    def case(rng, B, rows, T, layout, keep, gains, sim, ir, lens, fft=False):
        c = dict(B=B, rows=rows, T=T, layout=layout, keep=keep, gains=gains, sim=sim, ir=ir, lens=np.array(lens, dtype=np.uint32), fft=fft)
        c["valid"] = _valid(rng, B, T)
        c["index"] = rng.integers(-1, len(lens), size=B).astype(np.int32)
        c["index"][0] = 0                                    # (the whole window with the longest response: there is work, and power to keep)
        c["x"] = _batch(rng, c) * np.float32(0.25)
        return c

    @staticmethod
    def make(c):
        return dict(data=torch.from_numpy(c["x"]).to(DEV), ir=torch.from_numpy(c["ir"]).to(DEV), out=device_out(c["x"].size),
                    gains=device_out(c["B"]) if c["gains"] else None)

    @staticmethod
    def queue(ctx, c, b, stream):
        ctx.reverb_windows(b["data"], c["valid"], b["ir"], c["lens"], c["index"], c["layout"], out=b["out"][1].view(_shape(c)), keep_power=c["keep"],
                           gains=b["gains"][1] if c["gains"] else None, stream=stream, method="fft" if c["fft"] else "direct")

    @staticmethod
    def words(c, b, what):
        assert np.array_equal(_u32(b["data"].cpu().numpy()), _u32(c["x"])), what + ("the data was written",)
        assert np.array_equal(_u32(b["ir"].cpu().numpy()), _u32(c["ir"])), what + ("the responses were written",)
        out = [written(b["out"][0], c["x"].size, what + ("cells",))]
        return out + ([written(b["gains"][0], c["B"], what + ("gains",))] if c["gains"] else [])

    @staticmethod
    def sim(c):
        o, g = _filled(c["x"].shape), _filled((c["B"],))
        assert (sf if c["fft"] else sr).reverb_windows(c["x"], c["valid"], c["ir"], c["lens"], c["index"], c["layout"], o, int(c["keep"]), g)
        return [_u32(o)] + ([_u32(g)] if c["gains"] else [])

    @staticmethod
    def partials(c):
        """The doubles the call reserves: [B][2][rows][chunks] with keep_power, 0 without."""
        return c["B"] * 2 * c["rows"] * -(-c["T"] // CHUNK) if c["keep"] else 0

    @staticmethod
    def fft_bytes(c):
        """(the table's bytes, the workspace's) of an FFT call, as clx_rvfft_plan_call lays them out: 40 bytes a window and 12 a
        partition job; a spectrum of 1040 complex words for every segment (the ceil(T / 1024) blocks of every row) and every job.
        The jobs are every response's whole partitions (as many as the longest min(ir_len, valid) that reads it holds) and one
        ragged partition for every distinct (response, live taps)."""
        whole, ragged = {}, set()
        for v, j in zip(c["valid"].tolist(), c["index"].tolist()):
            if j >= 0:
                lv = min(int(c["lens"][j]), v)
                whole[j] = max(whole.get(j, 0), lv // 1024)
                if lv % 1024:
                    ragged.add((j, lv))
        jobs = sum(whole.values()) + len(ragged)
        return 40 * c["B"] + 12 * jobs, (c["B"] * c["rows"] * -(-c["T"] // 1024) + jobs) * 1040 * 8


class _SpecAug:
    """clx_specaug_windows, out of place: the input keeps its words; warps, F frequency and M time masks a window, `fills` always."""

    @staticmethod
    def case(rng, B, rows, T, layout, fill, sim, F=2, M=2, offset=0.0, width=(3, 6), least=0):
        c = dict(B=B, rows=rows, T=T, layout=layout, fill=fill, sim=sim, F=F, M=M)
        c["valid"] = v = _valid(rng, B, T, least)
        c["warp"] = np.zeros((B, 2), dtype=np.int64)
        for k in np.nonzero(v >= 6)[0]:
            cc = int(rng.integers(1, v[k]))
            c["warp"][k] = (cc, min(max(cc + int(rng.integers(-3, 4)), 1), int(v[k]) - 1))
        c["fm"] = np.stack([rng.integers(0, rows, (B, F)), rng.integers(0, width[0] + 1, (B, F))], axis=-1)
        c["tm"] = np.stack([rng.integers(0, T, (B, M)), rng.integers(0, width[1] + 1, (B, M))], axis=-1)
        c["x"] = _batch(rng, c, offset)
        return c

    @staticmethod
    def make(c):
        return dict(data=torch.from_numpy(c["x"]).to(DEV), out=device_out(c["x"].size), fills=device_out(c["B"]))

    @staticmethod
    def queue(ctx, c, b, stream):
        ctx.specaug_windows(b["data"], c["valid"], c["layout"], c["warp"], c["fm"], c["tm"], c["fill"], out=b["out"][1].view(_shape(c)),
                            fills=b["fills"][1], stream=stream)

    @staticmethod
    def words(c, b, what):
        assert np.array_equal(_u32(b["data"].cpu().numpy()), _u32(c["x"])), what + ("the input was written",)
        return [written(b["out"][0], c["x"].size, what + ("cells",)), written(b["fills"][0], c["B"], what + ("fills",))]

    @staticmethod
    def sim(c):
        o, f = _filled(c["x"].shape), _filled((c["B"],))
        ss.specaug_windows(c["x"], o, c["valid"], c["layout"], c["warp"], c["fm"], c["tm"], c["fill"], f)
        return [_u32(o), _u32(f)]

    @staticmethod
    def table(c):
        """The table's words on the device: V, the warp pair and the masks' ranges of every window, and its fill behind them."""
        return c["B"] * (3 + 2 * c["F"] + 2 * c["M"]) + c["B"]

    @staticmethod
    def partials(c):
        """The doubles a mean call reserves, clx_norm's [B][rows][2][chunks]; a constant fill needs none."""
        return c["B"] * c["rows"] * 2 * -(-c["T"] // CHUNK) if c["fill"] == "mean" else 0


def _alone(op, c, what):
    """The call's output words when a context that has made no other makes it by itself."""
    alone = cx.Context(0)
    b = op.make(c)
    torch.cuda.synchronize()
    op.queue(alone, c, b, None)
    torch.cuda.synchronize()
    got = [w.copy() for w in op.words(c, b, what + ("alone",))]
    alone.close()
    return got


def _expected(op, calls, name):
    return [op.sim(c) if c["sim"] else _alone(op, c, (name, i)) for i, c in enumerate(calls)]


def _same(op, calls, bufs, want, name):
    """Every output word of every call against `want`; returns how many there were."""
    words = 0
    for i, (c, b, w) in enumerate(zip(calls, bufs, want)):
        what = (name, "call", i, c["B"], c["rows"], c["T"], c["layout"])
        got = op.words(c, b, what)
        assert len(got) == len(w)
        for part, (g, e) in enumerate(zip(got, w)):
            bad = np.nonzero(g != e)[0]
            assert bad.size == 0, what + ("output %d" % part, "%d words differ from the %s; the first is word %d"
                                          % (bad.size, "simulator" if c["sim"] else "call alone", bad[0]))
            words += e.size
    return words


def _queued(ctx, op, calls, name, outside=0):
    """The calls on ctx: the first `outside` before the work in front, the others behind it with nothing waited for, the current
    stream and a second one in turn.  Returns (whether the work in front was pending at each call, the words compared)."""
    want = _expected(op, calls, name)
    bufs = [op.make(c) for c in calls]
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    for c, b in zip(calls[:outside], bufs):
        op.queue(ctx, c, b, None)
    done, _ = _work_in_front(side)                           # (its own size, four products of 8192 x 8192 floats: see the module's text)
    pending = []
    for i, (c, b) in enumerate(zip(calls[outside:], bufs[outside:])):
        op.queue(ctx, c, b, side if i % 2 else None)
        pending.append(not done.query())
    torch.cuda.synchronize()
    return pending, _same(op, calls, bufs, want, name)


def _summary(name, calls, pending, made, words):
    print("%s queued: %d calls (%d simulated, %d alone on a fresh context); buffers made or replaced: %s; the work in front was pending "
          "at the calls: %r; %d words compared, 0 differ" % (name, len(calls), sum(c["sim"] for c in calls), sum(not c["sim"] for c in calls),
                                                              made, pending, words))


def test_norm_windows_queued_across_two_streams(ctx):
    """B = 1, 70, 200: the table (a word a window, slack 64) and the partial sums ([B][rows][2][chunks]) are made for the first and
    both replaced for the other two with launches pending on what they replace.  Then 2 windows of 160 rows over two chunks: the
    table fits and the sums do not, so only the sums are replaced and the stream must still wait for the last launch before the
    upload rewrites the table.  Then B = 50 twice, on what is there."""
    rng = np.random.default_rng(61)
    calls = [_Norm.case(rng, *a) for a in ((1, 3, 70, TC, True, True), (70, 2, 100, CT, False, True), (200, 2, 70, CT, True, False),
                                           (2, 160, CHUNK + 4, CT, True, True), (50, 4, 64, TC, True, True), (50, 2, 300, CT, False, True))]
    tables, cap = _made([c["B"] for c in calls], 64)
    sums, pcap = _made([c["B"] * c["rows"] * 2 * -(-c["T"] // CHUNK) for c in calls], 64)
    assert (tables, sums) == (3, 4) and calls[3]["B"] <= cap and cap >= 50 and pcap >= 50 * 4 * 2
    pending, words = _queued(ctx, _Norm, calls, "norm")
    _summary("norm", calls, pending, dict(table=tables, sums=sums), words)


def test_add_windows_queued_across_two_streams(ctx):
    """The ladder of the norm test over one noise tensor: the table (a window a unit, slack 64; the gains lie behind the call's own
    entries, so a call on a larger table than it needs writes them elsewhere than the call before it) and the partial sums
    ([B][2][rows][chunks]) are made for B = 1 and replaced for 70 and 200; B = 50 twice reuses both."""
    rng = np.random.default_rng(67)
    calls = [_Add.case(rng, *a) for a in ((1, CT, True, True), (70, TC, False, True), (200, CT, True, False), (50, TC, True, True),
                                          (50, CT, False, True), (50, TC, True, True))]
    tables, cap = _made([c["B"] for c in calls], 64)
    sums, pcap = _made([c["B"] * 2 * c["rows"] for c in calls], 64)
    assert (tables, sums) == (3, 3) and cap >= 50 and pcap >= 50 * 2 * 2
    assert all(np.any(c["index"] < 0) for c in calls[1:]) and all(np.any(c["index"] > 0) for c in calls[1:])
    _Add.d_noise = torch.from_numpy(_Add.noise).to(DEV)
    try:
        pending, words = _queued(ctx, _Add, calls, "add")
        assert np.array_equal(_u32(_Add.d_noise.cpu().numpy()), _u32(_Add.noise)), "the noise was written"
    finally:
        _Add.d_noise = None
    _summary("add", calls, pending, dict(table=tables, sums=sums), words)


def test_reverb_windows_queued_across_two_streams(ctx):
    """keep_power on and off in turn, responses of 300 taps (one chunk of 256 and a ragged one) and shorter.  With keep_power, B = 40
    makes the table and the sums; without, B = 150 replaces the table and reserves 0 sums (they count as kept: the stream waits);
    with, B = 20 finds room in both; without, B = 10 likewise."""
    rng = np.random.default_rng(71)
    ir = (rng.standard_normal((4, 300)) * np.exp(-np.arange(300) / 80.0)).astype(np.float32)
    lens = (300, 256, 7, 0)
    calls = [_Reverb.case(rng, *a, ir, lens) for a in ((40, 2, 333, CT, True, True, True), (150, 2, 333, TC, False, True, False),
                                                       (20, 3, 333, TC, True, False, True), (10, 1, 333, CT, False, True, True))]
    tables, cap = _made([c["B"] for c in calls], 64)
    sums, pcap = _made([_Reverb.partials(c) for c in calls], 64)
    assert (tables, sums) == (2, 1) and cap >= 20 and pcap >= _Reverb.partials(calls[2]) > 0 == _Reverb.partials(calls[1])
    pending, words = _queued(ctx, _Reverb, calls, "reverb")
    _summary("reverb", calls, pending, dict(table=tables, sums=sums), words)


def test_reverb_windows_fft_queued_across_two_streams(ctx):
    """A first call of one window meets the twiddles (their upload is a blocking copy, which would wait for the work in front) and
    makes the table (in bytes, slack 4096), the sums and the workspace.  Then, behind the work: 6 windows of two blocks (the
    workspace is replaced, the table and the sums are kept); 120 windows with keep_power (all three are replaced); 8 windows of
    three blocks (all three are kept); 40 windows of four rows (the workspace is replaced again, the table kept)."""
    rng = np.random.default_rng(73)
    tiny = rng.standard_normal((1, 8)).astype(np.float32)
    ir1 = (rng.standard_normal((3, 1100)) * np.exp(-np.arange(1100) / 300.0)).astype(np.float32)
    ir2 = (rng.standard_normal((3, 2100)) * np.exp(-np.arange(2100) / 500.0)).astype(np.float32)
    l1, l2 = (1100, 1030, 5), (2100, 1500, 1024)
    calls = [_Reverb.case(rng, *a, fft=True) for a in ((1, 1, 100, CT, True, True, True, tiny, (8,)), (6, 2, 1030, TC, False, True, True, ir1, l1),
                                                       (120, 1, 1030, CT, True, True, False, ir1, l1), (8, 2, 2100, TC, True, False, True, ir2, l2),
                                                       (40, 4, 2100, CT, False, True, False, ir2, l2))]
    nbytes = [_Reverb.fft_bytes(c) for c in calls]
    tables, _ = _made([t for t, w in nbytes], 4096)
    spectra, _ = _made([w for t, w in nbytes], 0)
    sums, _ = _made([_Reverb.partials(c) for c in calls], 64)
    assert (tables, spectra, sums) == (2, 4, 2)
    assert _made([t for t, w in nbytes[:2]], 4096)[0] == 1 and _made([w for t, w in nbytes[:2]], 0)[0] == 2       # (call 1: the workspace alone)
    assert _made([t for t, w in nbytes[:3]], 4096)[0] == 2 and _made([_Reverb.partials(c) for c in calls[:3]], 64)[0] == 2   # (call 2: all three)
    assert _made([w for t, w in nbytes[:4]], 0)[0] == 3                                                             # (call 3: nothing)
    pending, words = _queued(ctx, _Reverb, calls, "reverb fft", outside=1)
    _summary("reverb fft", calls, pending, dict(table=tables, spectra=spectra, sums=sums), words)


def test_specaug_windows_queued_across_two_streams(ctx):
    """The mean and a constant as the fill in turn, warps and masks everywhere.  B = 1 (mean) makes the table (in words, slack 64)
    and the sums; 70 (constant) replaces the table; 200 (mean) replaces both; 3 windows of 110 rows over two chunks (mean) find
    room in the table and replace the sums alone; B = 50 twice, a constant and the mean, on what is there."""
    rng = np.random.default_rng(79)
    calls = [_SpecAug.case(rng, *a) for a in ((1, 3, 70, TC, "mean", True), (70, 4, 40, CT, 0.5, True), (200, 2, 70, CT, "mean", False),
                                              (3, 110, CHUNK + 4, CT, "mean", False), (50, 8, 64, TC, -1.25, True), (50, 8, 64, CT, "mean", True))]
    tables, cap = _made([_SpecAug.table(c) for c in calls], 64)
    sums, pcap = _made([_SpecAug.partials(c) for c in calls], 64)      # (0 and not reserved come to the same count: neither is ever replaced)
    assert (tables, sums) == (3, 3) and _SpecAug.table(calls[3]) <= _made([_SpecAug.table(c) for c in calls[:3]], 64)[1]
    assert cap >= _SpecAug.table(calls[5]) and pcap >= _SpecAug.partials(calls[5])
    pending, words = _queued(ctx, _SpecAug, calls, "specaug")
    _summary("specaug", calls, pending, dict(table=tables, sums=sums), words)


def test_specaug_mean_after_a_constant_call_that_grew_the_table():
    """Three calls of one context.  A: the mean as the fill on the current stream, 32 windows of 80 rows and 3000 frames: clx_k_norm_sum
    writes the partial sums and clx_k_specaug_fill reads them.  B: a constant fill on a second stream, 8 windows with 32 + 32 masks
    each, so that its table is larger than A's: B replaces the one buffer it needs.  C: the mean again, on the second stream, 4
    windows of 80 rows whose cells lie 100 higher; its table and its sums fit what A and B left, and its sums are written to the
    head of the buffer A's kernels use.  C is ordered behind A only through B, so B has to wait for the last launch although it
    replaced its table: the sums it does not use are still another call's.  (A constant fill used to reserve no sums at all and to
    wait only when its table was kept; C then waited for B alone, and A's fills could come from C's sums or C's from A's.  Whether
    a machine shows that is a matter of timing: this test passing on such a library does not show that the order was right.)
    Four contexts get the triple behind the same work in front, the second stream put behind each A, so that every B and C is
    free to start where its A does; the expected words are each call's alone on a fresh context."""
    rng = np.random.default_rng(83)
    A = _SpecAug.case(rng, 32, 80, 3000, CT, "mean", False, least=2900)
    B = _SpecAug.case(rng, 8, 4, 8, CT, 0.5, False, F=32, M=32)
    C = _SpecAug.case(rng, 4, 80, 200, CT, "mean", False, offset=100.0)
    calls = [A, B, C]
    _, cap_a = _made([_SpecAug.table(A)], 64)
    _, pcap_a = _made([_SpecAug.partials(A)], 64)
    tables, cap_b = _made([_SpecAug.table(c) for c in (A, B)], 64)
    assert _SpecAug.table(B) > cap_a and tables == 2                  # B replaces the table ...
    assert _SpecAug.partials(B) == 0                                  # ... and has no use for the sums;
    assert _SpecAug.table(C) <= cap_b and 0 < _SpecAug.partials(C) <= pcap_a      # C keeps both
    want = _expected(_SpecAug, calls, "specaug a/b/c")
    assert float(want[2][1].view(np.float32)[0]) - float(want[0][1].view(np.float32)[0]) > 90      # (the first windows' means lie far apart)
    ctxs = [cx.Context(0, wait_s=120) for _ in range(4)]
    try:
        bufs = [[_SpecAug.make(c) for c in calls] for _ in ctxs]
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        done, _ = _work_in_front(side)                       # (its own size, four products of 8192 x 8192 floats: see the module's text)
        pending = []
        for c, b in zip(ctxs, bufs):
            for call, buf, stream in zip(calls, b, (None, side, side)):
                _SpecAug.queue(c, call, buf, stream)
                pending.append(not done.query())
            side.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        words = sum(_same(_SpecAug, calls, b, want, "specaug a/b/c, context %d" % i) for i, b in enumerate(bufs))
    finally:
        for c in ctxs:
            c.close()
    print("specaug a/b/c queued: 4 contexts x 3 calls (each alone on a fresh context for the expected words); per context the table is "
          "made by A and replaced by B, the sums are made by A and kept; the work in front was pending at the calls: %r; %d words "
          "compared, 0 differ" % (pending, words))
