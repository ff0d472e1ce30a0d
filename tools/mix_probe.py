"""One-second mono crops at 16 kHz from a resident shard that is half mono and half stereo: StreamSet.read(..., sample_rate=16000,
channels=1) against the route without it, and clx_mix_windows alone.  Workload: tools/resample_probe.py's with every second stream
mono -- 256 synthetic FLAC streams of 15 s at 44.1 kHz, 16 bits, blocks of 4096, 128 mono and 128 stereo; one window of 1 s (16 000
outputs) per stream at a seeded random start.  All figures come from one process on one device, host clocks around calls that end in
torch.cuda.synchronize() (device events for the launches alone); each is the median (and the fastest) of --repeats repeats after
--warmup warm-ups.

  (a) the framework route (the baseline: without channels= there is no single call): read(sample_rate=16000) per channel-count
      group, mean(-1, keepdim=True) of each, cat
  (b) one read(sample_rate=16000, channels=1)
  (c) clx_mix_windows alone on the stereo half (2 -> 1), in microseconds and GB/s of bytes read plus bytes written, next to
      clx_resample_windows on the same spans (2 -> 2)

Writes one JSON line per figure to --out (default profiles/mix_probe.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
FS, R, BS, SECONDS, N_STREAMS, WINDOW = 44100, 16000, 4096, 15, 256, 16000


def flac_stream(k, ch):
    import synth
    n_frames = (SECONDS * FS) // BS
    rng = np.random.default_rng(5000 + k)
    t = np.arange(n_frames * BS)
    x = np.stack([np.clip(np.round(9000 * np.sin(2 * np.pi * (80 + k + 7 * c) * t / FS) + rng.normal(0, 300, t.size)), -32768, 32767)
                  for c in range(ch)]).astype(np.int32)
    fp = [synth.FrameParams() for _ in range(n_frames)]
    for i, f in enumerate(fp):
        f.number = i
        for c in range(ch):
            f.sf[c] = synth.sf(synth.SF_LPC, order=8, precision=12, partition_order=4)
    w = synth.encode_frames("probe", x.reshape(ch, n_frames, BS).transpose(1, 0, 2), ch, BS, 16, fp, sample_rate=FS)
    si = bytearray(34)                                       # (no MD5, no sample count: neither is looked at here)
    si[0:2] = BS.to_bytes(2, "big"); si[2:4] = BS.to_bytes(2, "big")
    si[10:14] = ((FS << 12) | ((ch - 1) << 9) | (15 << 4)).to_bytes(4, "big")
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + bytes(si) + w.arena[:w.arena_len].tobytes()


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_probe.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=N_STREAMS)
    args = ap.parse_args()
    import torch
    import claxon_amd as cx
    import synth
    synth.build()
    n_streams = args.streams
    half = n_streams // 2
    chans = [1] * half + [2] * (n_streams - half)
    streams = [flac_stream(k, ch) for k, ch in enumerate(chans)]
    ctx = cx.Context(0, wait_s=120)
    sset = cx.open_streams(ctx, streams)
    assert sset.channels == chans
    o, n, W = cx.resample_pair(FS, R)
    T = int(sset.lengths[0])
    T_R = int(sset.lengths_at(R)[0])
    rng = np.random.default_rng(1)
    sid = np.arange(n_streams)
    starts = rng.integers(0, T_R - WINDOW, size=n_streams)
    groups = [sid[:half], sid[half:]]                        # (by channel count; in stream order, so (a)'s cat is (b)'s order)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), streams=n_streams, mono=half, stereo=n_streams - half, seconds=SECONDS, rate=FS,
         to_rate=R, bits=16, block=BS, window=WINDOW, o=o, n=n, W=W, repeats=args.repeats, warmup=args.warmup)

    def route_a():
        return torch.cat([sset.read(g, starts[g], WINDOW, sample_rate=R)[0].mean(-1, keepdim=True) for g in groups])

    def route_b():
        return sset.read(sid, starts, WINDOW, sample_rate=R, channels=1)[0]
    want, got = route_a(), route_b()
    assert got.shape == want.shape == (n_streams, WINDOW, 1)
    assert torch.equal(got[:half], want[:half])              # (the mono half: the same resampler on the same samples)
    emit(what="(a) against (b), stereo half: largest difference (the mean before the filter against the mean behind it)",
         max_abs_diff=float((got - want).abs().max()), max_abs=float(want.abs().max()))
    for _ in range(2):                                       # (alternating: twice each)
        n0 = sset.frames_decoded
        t = times(route_a, args.repeats, args.warmup)
        emit(what="(a) read(sample_rate=%d) per channel-count group + mean + cat, tc" % R,
             frames_per_batch=(sset.frames_decoded - n0) // (args.repeats + args.warmup), **t)
        n0 = sset.frames_decoded
        t = times(route_b, args.repeats, args.warmup)
        emit(what="(b) read(sample_rate=%d, channels=1), tc" % R, frames_per_batch=(sset.frames_decoded - n0) // (args.repeats + args.warmup), **t)

    # (c) the launches alone on the stereo half: the source spans back to back in one buffer
    st = starts[half:]
    B = st.size
    lo = np.maximum(st * o // n - W + 1, 0)
    hi = np.minimum((st + WINDOW - 1) * o // n + W + 1, T)
    span = hi - lo
    room = (span * 2 + 7) // 8 * 8
    first = (np.cumsum(room) - room).astype(np.uint64)
    scratch = torch.randn(int(room.sum()), device="cuda:0")
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
    valid32 = np.full(B, WINDOW, dtype=np.uint32)
    rates = np.full(B, FS, dtype=np.uint32)
    two = np.full(B, 2, dtype=np.uint8)
    out1 = torch.empty((B, WINDOW, 1), dtype=torch.float32, device="cuda:0")
    out2 = torch.empty((B, WINDOW, 2), dtype=torch.float32, device="cuda:0")
    read_bytes = int(span.sum()) * 2 * 4
    for name, fn, out, filters in (
            ("clx_mix_windows alone, 2 -> 1", lambda: ctx.mix_windows(scratch, first, lo, span, st, valid32, rates, two, R, WINDOW, 1, cx.WINDOW_TC, out1),
             out1, 1),
            ("clx_resample_windows alone, 2 -> 2", lambda: ctx.resample_windows(scratch, first, lo, span, st, valid32, rates, R, WINDOW, 2, cx.WINDOW_TC, out2),
             out2, 2)):
        med, best = device_ms(fn)
        moved = read_bytes + out.numel() * 4                 # bytes of the spans read once plus bytes written
        emit(what="(c) %s, tc, the stereo half (back to back: the table upload of each call included)" % name, median_us=round(med * 1e3, 2),
             min_us=round(best * 1e3, 2), mb_moved=round(moved / 1e6, 2), gb_per_s=round(moved / med / 1e6, 1),
             gflop_per_s=round(2 * B * WINDOW * filters * 2 * W / med / 1e6, 1))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
