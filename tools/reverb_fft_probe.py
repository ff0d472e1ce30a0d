"""The partitioned FFT form of reverb= against the direct form and against the framework route, on reverb_probe.py's workload: 32
synthetic mono FLAC streams of 32 s at 16 kHz as speech and 32 decaying-noise responses; one window of 30 s per stream, every fourth
two thirds padding; responses truncated to 800, 4 000 and 16 000 taps; keep_power on.  All figures come from one process on one
device.  Per tap count the three routes

  (f) read(.., "ct", reverb=Reverb(.., taps=K, method="fft"))
  (d) read(.., "ct", reverb=Reverb(.., taps=K))                               the direct form
  (t) read, source.read, then torch rfft / irfft (reverb_probe.py's route (b))

run in turn inside every repeat -- f, d, t, f, d, t, .. -- behind --warmup rounds of all three, host clocks around calls that end
in torch.cuda.synchronize(); each figure is the median (with the fastest and the slowest: the run-to-run spread) of --repeats.  Then
the launches alone with keep_power off, on (t)'s batches, between device events: clx_reverb_windows_fft (its forward and its
multiply-accumulate kernel) against clx_reverb_windows (clx_k_reverb), alternating likewise.  And the largest difference between the
two methods' batches.  Writes one JSON line per figure to --out (default profiles/reverb_fft_probe.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from norm_probe import BS, FS, N_STREAMS, WINDOW_S, flac_stream  # noqa: E402
from reverb_probe import TAPS, rir_stream, torch_reverb  # noqa: E402


def _stat(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reverb_fft_probe.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=N_STREAMS)
    args = ap.parse_args()
    import torch
    import claxon_amd as cx
    import synth
    synth.build()
    B = args.streams
    ctx = cx.Context(0, wait_s=120)
    speech = cx.open_streams(ctx, [flac_stream(k) for k in range(B)])
    rirs = cx.open_streams(ctx, [rir_stream(k) for k in range(B)])
    assert speech.problems == [None] * B and rirs.problems == [None] * B
    T = int(speech.lengths[0])
    L = WINDOW_S * FS
    sid = np.arange(B)
    starts = np.where(sid % 4 == 3, T - 10 * FS, 0)
    dev = "cuda:%d" % ctx.device
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), windows=B, seconds=WINDOW_S, rate=FS, short_windows=int((sid % 4 == 3).sum()),
         block=BS, taps=list(TAPS), repeats=args.repeats, warmup=args.warmup, order="fft, direct, torch in turn inside every repeat")
    side = torch.cuda.Stream(device=dev)
    for K in TAPS:
        def fft():
            return speech.read(sid, starts, L, "ct", reverb=cx.Reverb(sid, rirs, taps=K, keep_power=True, method="fft"))

        def direct():
            return speech.read(sid, starts, L, "ct", reverb=cx.Reverb(sid, rirs, taps=K, keep_power=True))

        def framework():
            x, v = speech.read(sid, starts, L, "ct")
            h, _ = rirs.read(sid, np.zeros(B, dtype=np.int64), K, "ct")
            y, g = torch_reverb(x, v.to(dev), h)
            return y, v, g

        routes = (("fft", fft), ("direct", direct), ("torch", framework))
        a, b, c = fft(), direct(), framework()
        torch.cuda.synchronize()
        emit(what="agreement", taps=K, max_abs_fft_minus_direct=float((a[0] - b[0]).abs().max()), max_abs_fft_minus_torch=float((a[0] - c[0]).abs().max()),
             max_abs=float(b[0].abs().max()))
        del a, b, c
        ts = {name: [] for name, _ in routes}
        for i in range(args.warmup + args.repeats):
            for name, fn in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ts[name].append((time.perf_counter() - t0) * 1e3)
        st = {name: _stat(v) for name, v in ts.items()}
        emit(what="read(reverb=, method='fft') (f)", taps=K, **st["fft"])
        emit(what="read(reverb=) direct (d)", taps=K, **st["direct"])
        emit(what="read, read, then torch rfft / irfft (t)", taps=K, **st["torch"])
        emit(what="ratio", taps=K, f_over_d=round(st["fft"]["median_ms"] / st["direct"]["median_ms"], 3),
             f_over_t=round(st["fft"]["median_ms"] / st["torch"]["median_ms"], 3),
             fft_faster_than_direct_beyond_spread=bool(st["fft"]["max_ms"] < st["direct"]["min_ms"]))

        x, v = speech.read(sid, starts, L, "ct")
        h, hl = rirs.read(sid, np.zeros(B, dtype=np.int64), K, "ct")
        v, hl = v.numpy(), hl.numpy()
        outs = {m: torch.empty_like(x) for m in ("fft", "direct")}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ls = {m: [] for m in outs}
        for i in range(args.warmup + args.repeats):
            for m in ("fft", "direct"):
                torch.cuda.synchronize()
                ev0.record(side)
                ctx.reverb_windows(x, v, h.view(B, K), hl, sid, cx.WINDOW_CT, out=outs[m], keep_power=False, stream=side, method=m)
                ev1.record(side)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ls[m].append(ev0.elapsed_time(ev1))
        emit(what="clx_reverb_windows_fft alone, keep_power off", taps=K, **_stat(ls["fft"]))
        emit(what="clx_reverb_windows alone, keep_power off", taps=K, **_stat(ls["direct"]))
        emit(what="unscaled agreement", taps=K, max_abs_fft_minus_direct=float((outs["fft"] - outs["direct"]).abs().max()),
             max_abs=float(outs["direct"].abs().max()))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
