"""One-second crops from a resident shard: StreamSet.read against load_batch followed by a slice, and clx_gather_windows alone.
Workload: 256 synthetic FLAC streams of 15 s, 16 kHz stereo, 16 bits, blocks of 4096 (58 frames each); one window of 16 000 samples
per stream at a seeded random start.  All figures come from one process on one device, host clocks around calls that end in
torch.cuda.synchronize(); each is the median (and the fastest) of --repeats repeats after --warmup warm-ups.

  (a) load_batch of the 256 streams, then one 1 s slice of each        the route without a resident set
  (b) open_streams, once                                                 upload + index
  (c) StreamSet.read of the 256 windows, "tc" and "ct"                   with its host-side steps timed apart
  (d) clx_gather_windows alone on (c)'s shapes, in GB/s of bytes read plus bytes written, next to a torch device-to-device copy of
      the same number of bytes

Writes one JSON line per figure to --out (default profiles/window_probe.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
RATE, BS, SECONDS, N_STREAMS, WINDOW = 16000, 4096, 15, 256, 16000


def flac_stream(k):
    import synth
    n_frames = (SECONDS * RATE) // BS
    rng = np.random.default_rng(4000 + k)
    t = np.arange(n_frames * BS)
    x = np.stack([np.clip(np.round(9000 * np.sin(2 * np.pi * (80 + k + 7 * c) * t / RATE) + rng.normal(0, 300, t.size)), -32768, 32767)
                  for c in range(2)]).astype(np.int32)
    fp = [synth.FrameParams() for _ in range(n_frames)]
    for i, f in enumerate(fp):
        f.number = i
        for c in range(2):
            f.sf[c] = synth.sf(synth.SF_LPC, order=8, precision=12, partition_order=4)
    w = synth.encode_frames("probe", x.reshape(2, n_frames, BS).transpose(1, 0, 2), 2, BS, 16, fp, sample_rate=RATE)
    si = bytearray(34)                                       # (no MD5, no sample count: neither is looked at here)
    si[0:2] = BS.to_bytes(2, "big"); si[2:4] = BS.to_bytes(2, "big")
    si[10:14] = ((RATE << 12) | (1 << 9) | (15 << 4)).to_bytes(4, "big")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_probe.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import claxon_amd as cx
    import synth
    synth.build()
    streams = [flac_stream(k) for k in range(N_STREAMS)]
    ctx = cx.Context(0, wait_s=120)
    rng = np.random.default_rng(1)
    sid = np.arange(N_STREAMS)
    starts = rng.integers(0, (SECONDS * RATE) // BS * BS - WINDOW, size=N_STREAMS)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), streams=N_STREAMS, seconds=SECONDS, rate=RATE, channels=2, bits=16, block=BS,
         window=WINDOW, compressed_mb=round(sum(len(s) for s in streams) / 1e6, 2), repeats=args.repeats, warmup=args.warmup)

    def route_a():
        x, _, _ = cx.load_batch(ctx, streams)
        return torch.stack([x[k, s:s + WINDOW] for k, s in enumerate(starts.tolist())])
    want = route_a()
    emit(what="(a) load_batch + one slice per stream", **times(route_a, max(3, args.repeats // 4), 1))
    emit(what="(b) open_streams", **times(lambda: cx.open_streams(ctx, streams), max(3, args.repeats // 4), 1))
    sset = cx.open_streams(ctx, streams)
    for layout in ("tc", "ct"):
        got, valid = sset.read(sid, starts, WINDOW, layout=layout)
        assert torch.equal(got if layout == "tc" else got.transpose(1, 2), want) and valid.tolist() == [WINDOW] * N_STREAMS
        n0 = sset.frames_decoded
        t = times(lambda: sset.read(sid, starts, WINDOW, layout=layout), args.repeats, args.warmup)
        emit(what="(c) read, %s" % layout, frames_per_read=(sset.frames_decoded - n0) // (args.repeats + args.warmup),
             frames_in_the_set=int(sset._descs.size), **t)

    # (c) cut into its steps: the plan and the decode through a Batch kept open, the gather alone
    f0 = np.searchsorted(sset._start, sset._base[sid] + starts, side="right") - 1
    f1 = np.searchsorted(sset._start, sset._base[sid] + starts + WINDOW - 1, side="right") - 1
    rows = np.concatenate([np.arange(a, b + 1) for a, b in zip(f0, f1)])
    descs = sset._descs[rows]
    sizes = descs["block_size"].astype(np.uint64) * 2
    out_offs = (np.cumsum(sizes) - sizes).astype(np.uint64)
    scratch = torch.empty(int(sizes.sum()), dtype=torch.float32, device="cuda:0")

    def plan():
        cx.Batch(ctx, descs, out_offs, True, cx.OUT_F32).close()
    emit(what="(c) step: plan (clx_batch_create + destroy) of the covering frames", frames=int(rows.size), **times(plan, args.repeats, args.warmup))
    batch = cx.Batch(ctx, descs, out_offs, True, cx.OUT_F32)

    def decode():
        batch.run(sset._arena.data_ptr(), int(sset._arena_len), scratch.data_ptr())
        batch.results()
    emit(what="(c) step: run + results of the planned frames", **times(decode, args.repeats, args.warmup))
    batch.close()

    per = np.cumsum(f1 - f0 + 1) - (f1 - f0 + 1)
    first = (out_offs[per] + (starts - sset._local[f0]).astype(np.uint64) * 2).astype(np.uint64)
    valid = np.full(N_STREAMS, WINDOW, dtype=np.uint32)
    out = torch.empty((N_STREAMS, WINDOW, 2), dtype=torch.float32, device="cuda:0")
    moved = 2 * out.numel() * 4                              # bytes read plus bytes written
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
    other = torch.empty_like(out)
    med, best = device_ms(lambda: other.copy_(out))
    copy_gbs = moved / med / 1e6
    emit(what="(d) torch device-to-device copy of the same bytes", mb_moved=round(moved / 1e6, 2), median_us=round(med * 1e3, 2), min_us=round(best * 1e3, 2),
         gb_per_s=round(copy_gbs, 1))
    for layout, name in ((cx.WINDOW_TC, "tc"), (cx.WINDOW_CT, "ct")):
        o = out if name == "tc" else out.view(N_STREAMS, 2, WINDOW)
        med, best = device_ms(lambda: ctx.gather_windows(scratch, first, valid, WINDOW, 2, layout, o))
        emit(what="(d) clx_gather_windows alone, %s (back to back: the table upload of each call included)" % name, median_us=round(med * 1e3, 2),
             min_us=round(best * 1e3, 2), gb_per_s=round(moved / med / 1e6, 1), of_the_copy=round(moved / med / 1e6 / copy_gbs, 3))
        assert torch.equal(o if name == "tc" else o.transpose(1, 2), want)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
