"""Noise mixed into the windows inside the read against the framework route behind two reads.  Workload: 32 synthetic mono FLAC
streams of 32 s at 16 kHz, 16 bits, blocks of 4096, as speech, and 32 more as noise; one window of 30 s per stream, every fourth
speech window starting 10 s before its stream's end (two thirds padding) and every eighth noise window starting 20 s before its
stream's end (the noise ends inside the window).  All figures come from one process on one device, host clocks around calls that
end in torch.cuda.synchronize(); each is the median (and the fastest) of --repeats repeats after --warmup warm-ups.

  (a) read(.., "ct", add=Add(.., source=noise set))                      against
  (b) read(.., "ct") on both sets followed by torch: masks from valid, the two masked square-sums, the divide, pow, sqrt and the
      masked addcmul
  (c) clx_add_windows alone on (b)'s batches (device events), in microseconds and GB/s of the bytes it moves: the live samples of
      both batches read twice and those of one written (padding and the cells behind a noise's end are not touched)

Writes one JSON line per figure to --out (default profiles/add_probe.txt)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from norm_probe import BS, FS, N_STREAMS, WINDOW_S, flac_stream, times  # noqa: E402


def torch_add(x, v, n, nv, snr_db):
    """The framework route: x, n [B, 1, L]; v, nv [B] on the device.  Mean-power SNR over each side's live samples, the noise added
    where both are live."""
    import torch
    L = x.shape[-1]
    t = torch.arange(L, device=x.device).view(1, 1, L)
    vn = torch.minimum(v, nv)
    ls, ln = t < v.view(-1, 1, 1), t < vn.view(-1, 1, 1)
    es = (x.double() ** 2 * ls).sum((1, 2))
    en = (n.double() ** 2 * ln).sum((1, 2))
    q = torch.pow(torch.tensor(10.0, dtype=torch.float64, device=x.device), -snr_db.double() / 10.0)
    g = torch.sqrt(es * vn * q / (en * v).clamp(min=1e-300))
    g = torch.where((es > 0) & (en > 0) & (vn > 0), g, torch.zeros_like(g)).float()
    return torch.addcmul(x, n * ln, g.view(-1, 1, 1)), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "add_probe.txt"))
    ap.add_argument("--repeats", type=int, default=10)
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
    noise = cx.open_streams(ctx, [flac_stream(100 + k) for k in range(B)])
    assert speech.problems == [None] * B and noise.problems == [None] * B
    T = int(speech.lengths[0])
    L = WINDOW_S * FS
    sid = np.arange(B)
    starts = np.where(sid % 4 == 3, T - 10 * FS, 0)
    nstarts = np.where(sid % 8 == 5, T - 20 * FS, 0)
    snr = np.linspace(0.0, 20.0, B).astype(np.float32)
    dev = "cuda:%d" % ctx.device
    snr_dev = torch.from_numpy(snr).to(dev)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), windows=B, seconds=WINDOW_S, rate=FS, short_windows=int((sid % 4 == 3).sum()),
         short_noises=int((sid % 8 == 5).sum()), block=BS, repeats=args.repeats, warmup=args.warmup)

    def fused():
        return speech.read(sid, starts, L, "ct", add=cx.Add(sid, nstarts, snr, source=noise), return_gains=True)

    def framework():
        x, v = speech.read(sid, starts, L, "ct")
        n, nv = noise.read(sid, nstarts, L, "ct")
        y, g = torch_add(x, v.to(dev), n, nv.to(dev), snr_dev)
        return y, v, g

    a, b = fused(), framework()
    torch.cuda.synchronize()
    emit(what="agreement", max_abs_diff=float((a[0] - b[0]).abs().max()), max_rel_gain_diff=float(((a[2] - b[2]).abs() / b[2].clamp(min=1e-30)).max()))
    ta, tb = times(fused, args.repeats, args.warmup), times(framework, args.repeats, args.warmup)
    emit(what="read(add=) (a)", **ta)
    emit(what="read, read, then torch (b)", **tb)
    emit(what="ratio", a_over_b=round(ta["median_ms"] / tb["median_ms"], 3), b_over_a=round(tb["median_ms"] / ta["median_ms"], 3))

    x, v = speech.read(sid, starts, L, "ct")
    n, nv = noise.read(sid, nstarts, L, "ct")
    v, nv = v.numpy(), nv.numpy()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    side = torch.cuda.Stream(device=dev)                     # (a stream of torch's own: on the default one the launches would go to the
    for i in range(args.warmup + args.repeats):              # context's stream, and the events would not bracket them)
        y = x.clone()
        torch.cuda.synchronize()
        ev0.record(side)
        ctx.add_windows(y, v, n, nv, sid, snr, cx.WINDOW_CT, stream=side)
        ev1.record(side)
        torch.cuda.synchronize()
        if i >= args.warmup:
            ts.append(ev0.elapsed_time(ev1) * 1e3)
    us = float(np.median(ts))
    # what the kernels touch: the sum pass reads the signal's Vs and the noise's Vn live samples, the apply pass reads Vn of each
    # and writes Vn; padding and the cells behind a noise's end are neither loaded nor stored
    vn = np.minimum(v, nv)
    moved = int(4 * (v.astype(np.int64).sum() + 4 * vn.astype(np.int64).sum()))
    emit(what="clx_add_windows alone (c): waveform [B, 1, L] twice", median_us=round(us, 1), min_us=round(min(ts), 1),
         bytes_moved=moved, bytes_of_whole_batches=5 * x.numel() * 4, gb_per_s=round(moved / us / 1e3, 1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
