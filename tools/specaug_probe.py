"""SpecAugment inside the read against the framework route behind it.  Workload: 32 synthetic mono FLAC streams of 32 s at 16 kHz,
16 bits, blocks of 4096; one window of 3000 Kaldi fbank frames by 80 bands per stream, every fourth one starting 10 s before its
stream's end, so that it is two thirds padding; the default policy SpecAugment(seed=1), one plan drawn once and used by every route.
All figures come from one process on one device, host clocks around calls that end in torch.cuda.synchronize(); each is the median
(and the fastest) of --repeats repeats after --warmup warm-ups.

  (a) read_mel(.., MelSpec.kaldi, "ct") followed by torch: per window the mean of the live cells, torch.nn.functional.interpolate(
      mode="bicubic") of the two segments, masked_fill of the masks' rows and frames
  (b) read_mel(.., MelSpec.kaldi, "ct", augment=plan)
  (c) clx_specaug_windows alone on (a)'s batch (device events), in microseconds and TB/s of the batch read once and written once (the
      mean's sum pass reads it a second time and is inside the figure), beside a torch device-to-device copy of the same bytes

Writes one JSON line per figure to --out (default profiles/specaug_probe.txt)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from norm_probe import FS, N_STREAMS, flac_stream, times  # noqa: E402

FRAMES = 3000


def torch_specaug(x, vf, plan):
    """The framework route on x [B, rows, T] (a new tensor): what clx_specaug_windows defines, by torch's own operations."""
    import torch
    y = x.clone()
    rows = x.shape[1]
    for k, V in enumerate(vf):
        live = x[k, :, :V]
        fill = live.mean() if plan.fill == "mean" and V else torch.zeros((), device=x.device) + (0.0 if plan.fill == "mean" else plan.fill)
        c, w = (int(v) for v in plan.warp[k])
        if c != w:
            for b, I, ob, O in ((0, c, 0, w), (c, V - c, w, V - w)):
                seg = live[:, b:b + I].reshape(1, rows, 1, I)
                y[k, :, ob:ob + O] = torch.nn.functional.interpolate(seg, size=(1, O), mode="bicubic", align_corners=False).view(rows, O)
        for first, width in plan.freq_masks[k]:
            y[k, int(first):int(first) + int(width), :V] = fill
        for first, width in plan.time_masks[k]:
            y[k, :, int(first):min(int(first) + int(width), V)] = fill
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specaug_probe.txt"))
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
    sset = cx.open_streams(ctx, [flac_stream(k) for k in range(B)])
    assert sset.problems == [None] * B
    T = int(sset.lengths[0])
    sid = np.arange(B)
    starts = np.where(sid % 4 == 3, T - 10 * FS, 0)
    spec = cx.MelSpec.kaldi(ctx)
    x, vf = sset.read_mel(sid, starts, FRAMES, spec, layout="ct")
    vf = vf.numpy()
    plan = cx.SpecAugment(seed=1).draw(vf, spec.n_out)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), windows=B, frames=FRAMES, n_mels=spec.n_out, short_windows=int((sid % 4 == 3).sum()),
         warped=int((plan.warp[:, 0] != plan.warp[:, 1]).sum()), masked_frames=int(plan.time_masks[..., 1].sum()), repeats=args.repeats,
         warmup=args.warmup)

    def route_a():
        y, v = sset.read_mel(sid, starts, FRAMES, spec, layout="ct")
        return torch_specaug(y, vf, plan), v

    def route_b():
        return sset.read_mel(sid, starts, FRAMES, spec, layout="ct", augment=plan)

    torch.cuda.synchronize()
    a = torch_specaug(x, vf, plan)                           # (on a batch that is complete: every step waited for)
    torch.cuda.synchronize()
    b = route_b()[0]
    torch.cuda.synchronize()
    emit(what="agreement", max_abs_diff=float((a - b).abs().max()), max_abs_cell=float(b.abs().max()))
    ta, tb = times(route_a, args.repeats, args.warmup), times(route_b, args.repeats, args.warmup)
    emit(what="read_mel kaldi, then torch (a)", **ta)
    emit(what="read_mel kaldi, augment= (b)", **tb)
    emit(what="ratio", a_over_b=round(ta["median_ms"] / tb["median_ms"], 3))

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = torch.empty_like(x)

    def alone(fn):
        ts = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            ev0.record()
            fn()
            ev1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(ev0.elapsed_time(ev1) * 1e3)
        us = float(np.median(ts))
        return dict(median_us=round(us, 1), min_us=round(min(ts), 1), tb_per_s=round(2 * x.numel() * 4 / us / 1e6, 3))

    for layout, name in ((cx.WINDOW_CT, "[B, 80, F]"), (cx.WINDOW_TC, "[B, F, 80] (the same bytes taken as TC)")):
        for fill in ("mean", 0.0):
            emit(what="clx_specaug_windows alone (c): %s, fill=%r" % (name, fill),
                 **alone(lambda: ctx.specaug_windows((x.data_ptr(), B, spec.n_out, FRAMES), vf, layout, plan.warp, plan.freq_masks, plan.time_masks,
                                                     fill, out=out.data_ptr(), stream=torch.cuda.current_stream())))
    emit(what="torch device-to-device copy of the same bytes", **alone(lambda: out.copy_(x)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
