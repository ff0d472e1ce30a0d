"""One-second crops at 16 kHz from a resident shard of 44.1 kHz streams: StreamSet.read(..., sample_rate=16000) against reading at the
native rate and resampling with a torch strided conv1d, and clx_resample_windows alone.  Workload: tools/window_probe.py's with the
streams at 44.1 kHz -- 256 synthetic FLAC streams of 15 s, stereo, 16 bits, blocks of 4096; one window of 1 s (16 000 outputs) per
stream at a seeded random start.  All figures come from one process on one device, host clocks around calls that end in
torch.cuda.synchronize() (device events for the launches alone); each is the median (and the fastest) of --repeats repeats after
--warmup warm-ups.

  (a) read() of the covering 44.1 kHz samples, then conv1d(stride 441) with the same [160, 34] table     the route without the feature
  (b) read(sample_rate=16000)
  (c) clx_resample_windows alone on (b)'s shapes, in microseconds and in GB/s of bytes read plus bytes written, next to
      clx_gather_windows writing the same number of floats
  (d) read(sample_rate=44100) against read(): the same windows, as copies

Writes one JSON line per figure to --out (default profiles/resample_probe.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
FS, R, BS, SECONDS, N_STREAMS, WINDOW = 44100, 16000, 4096, 15, 256, 16000


def flac_stream(k):
    import synth
    n_frames = (SECONDS * FS) // BS
    rng = np.random.default_rng(4000 + k)
    t = np.arange(n_frames * BS)
    x = np.stack([np.clip(np.round(9000 * np.sin(2 * np.pi * (80 + k + 7 * c) * t / FS) + rng.normal(0, 300, t.size)), -32768, 32767)
                  for c in range(2)]).astype(np.int32)
    fp = [synth.FrameParams() for _ in range(n_frames)]
    for i, f in enumerate(fp):
        f.number = i
        for c in range(2):
            f.sf[c] = synth.sf(synth.SF_LPC, order=8, precision=12, partition_order=4)
    w = synth.encode_frames("probe", x.reshape(2, n_frames, BS).transpose(1, 0, 2), 2, BS, 16, fp, sample_rate=FS)
    si = bytearray(34)                                       # (no MD5, no sample count: neither is looked at here)
    si[0:2] = BS.to_bytes(2, "big"); si[2:4] = BS.to_bytes(2, "big")
    si[10:14] = ((FS << 12) | (1 << 9) | (15 << 4)).to_bytes(4, "big")
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + bytes(si) + w.arena[:w.arena_len].tobytes()


def table(o, n, W):
    """The [n, 2W] coefficients of the definition (claxon_hip.h), float64."""
    base = min(o, n) * 0.99
    i = np.arange(n)[:, None]
    d = (np.arange(2 * W)[None, :] - W + 1) - ((i * o) % n) / n
    t = d * base / o
    return np.where(np.abs(t) < 6, np.sinc(t) * np.cos(np.pi * t / 12) ** 2 * base / o, 0.0)


def times(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_probe.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=N_STREAMS)
    args = ap.parse_args()
    import torch
    import claxon_amd as cx
    import synth
    synth.build()
    n_streams = args.streams
    streams = [flac_stream(k) for k in range(n_streams)]
    ctx = cx.Context(0, wait_s=120)
    sset = cx.open_streams(ctx, streams)
    o, n, W = cx.resample_pair(FS, R)
    T = int(sset.lengths[0])
    T_R = int(sset.lengths_at(R)[0])
    rng = np.random.default_rng(1)
    sid = np.arange(n_streams)
    # whole periods of the phase (160 outputs = 441 source samples), so that route (a) is one strided convolution for every window
    starts = rng.integers(1, (T_R - WINDOW) // n - 1, size=n_streams) * n
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), streams=n_streams, seconds=SECONDS, rate=FS, to_rate=R, channels=2, bits=16,
         block=BS, window=WINDOW, o=o, n=n, W=W, repeats=args.repeats, warmup=args.warmup)

    # (a): the covering source run of a window is the same length for every start that is a multiple of n
    src_starts = starts // n * o - W + 1
    src_len = (WINDOW // n - 1) * o + (n - 1) * o // n + 2 * W
    kernel = torch.from_numpy(table(o, n, W).astype(np.float32)).to("cuda:0")      # [n, 2W]
    offs = torch.from_numpy(np.arange(n) * o // n).to("cuda:0")

    def route_a():
        x, _ = sset.read(sid, src_starts, src_len, layout="ct")                   # [B, 2, src_len] at 44.1 kHz
        x = x.reshape(n_streams * 2, 1, src_len)
        # phase i of every period: taps from floor(i o / n) of the period's source run on; one conv1d per distinct offset would be n
        # launches, so the kernel is laid out over the period's whole support instead: [n, 1, (n-1) o // n + 2W], stride o
        return torch.nn.functional.conv1d(x, wide, stride=o).reshape(n_streams, 2, n, WINDOW // n)
    support = (n - 1) * o // n + 2 * W
    wide = torch.zeros((n, 1, support), device="cuda:0")
    for i in range(n):
        wide[i, 0, int(offs[i]):int(offs[i]) + 2 * W] = kernel[i]

    def route_a_ct():
        y = route_a()                                                             # [B, 2, n, periods] -> [B, 2, WINDOW]
        return y.permute(0, 1, 3, 2).reshape(n_streams, 2, WINDOW)
    want = route_a_ct()
    got, valid = sset.read(sid, starts, WINDOW, layout="ct", sample_rate=R)
    assert valid.tolist() == [WINDOW] * n_streams
    emit(what="(a) against (b): largest difference of the two routes' outputs (float32 sums in different orders)",
         max_abs_diff=float((got - want).abs().max()), max_abs=float(want.abs().max()))
    emit(what="(a) read() at 44.1 kHz + conv1d(stride %d) with the [%d, %d] table, ct" % (o, n, 2 * W), source_samples_per_window=src_len,
         **times(route_a_ct, args.repeats, args.warmup))
    for layout in ("tc", "ct"):
        n0 = sset.frames_decoded
        t = times(lambda: sset.read(sid, starts, WINDOW, layout=layout, sample_rate=R), args.repeats, args.warmup)
        emit(what="(b) read(sample_rate=%d), %s" % (R, layout), frames_per_read=(sset.frames_decoded - n0) // (args.repeats + args.warmup), **t)

    # (c) the launch alone: the source spans back to back in one buffer
    lo = np.maximum(starts * o // n - W + 1, 0)
    hi = np.minimum((starts + WINDOW - 1) * o // n + W + 1, T)
    span = hi - lo
    room = (span * 2 + 7) // 8 * 8
    first = (np.cumsum(room) - room).astype(np.uint64)
    scratch = torch.randn(int(room.sum()), device="cuda:0")
    out = torch.empty((n_streams, WINDOW, 2), dtype=torch.float32, device="cuda:0")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def device_ms(fn, inner=20):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.repeats):
            ev0.record()
            for _ in range(inner):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            ts.append(ev0.elapsed_time(ev1) / inner)
        return float(np.median(ts)), min(ts)
    valid32 = np.full(n_streams, WINDOW, dtype=np.uint32)
    rates = np.full(n_streams, FS, dtype=np.uint32)
    moved = int(span.sum()) * 2 * 4 + out.numel() * 4        # bytes of the spans read once plus bytes written
    flops = 2 * out.numel() * 2 * W
    for layout, name in ((cx.WINDOW_TC, "tc"), (cx.WINDOW_CT, "ct")):
        ov = out if name == "tc" else out.view(n_streams, 2, WINDOW)
        med, best = device_ms(lambda: ctx.resample_windows(scratch, first, lo, span, starts, valid32, rates, R, WINDOW, 2, layout, ov))
        emit(what="(c) clx_resample_windows alone, %s (back to back: the table upload of each call included)" % name, median_us=round(med * 1e3, 2),
             min_us=round(best * 1e3, 2), mb_moved=round(moved / 1e6, 2), gb_per_s=round(moved / med / 1e6, 1), gflop_per_s=round(flops / med / 1e6, 1))
    gfirst = first
    gmoved = 2 * out.numel() * 4
    for layout, name in ((cx.WINDOW_TC, "tc"), (cx.WINDOW_CT, "ct")):
        ov = out if name == "tc" else out.view(n_streams, 2, WINDOW)
        med, best = device_ms(lambda: ctx.gather_windows(scratch, gfirst, valid32, WINDOW, 2, layout, ov))
        emit(what="(c) clx_gather_windows alone on the same output size, %s" % name, median_us=round(med * 1e3, 2), min_us=round(best * 1e3, 2),
             mb_moved=round(gmoved / 1e6, 2), gb_per_s=round(gmoved / med / 1e6, 1))

    # (d) the native rate asked for by name: copies through clx_k_resample against the gather
    nat_starts = rng.integers(0, T - FS, size=n_streams)
    a, _ = sset.read(sid, nat_starts, FS)
    b, _ = sset.read(sid, nat_starts, FS, sample_rate=FS)
    assert torch.equal(a, b)
    for _ in range(2):                                       # (alternating: twice each)
        emit(what="(d) read() of 1 s at the native rate, tc", **times(lambda: sset.read(sid, nat_starts, FS), args.repeats, args.warmup))
        emit(what="(d) read(sample_rate=%d) of the same windows, tc" % FS,
             **times(lambda: sset.read(sid, nat_starts, FS, sample_rate=FS), args.repeats, args.warmup))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
