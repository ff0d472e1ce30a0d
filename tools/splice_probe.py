"""Frame splicing inside the read against the framework route behind it.  Workload: 32 synthetic mono FLAC streams of 32 s at 16 kHz,
16 bits, blocks of 4096; one window of 3000 frames per stream, every fourth one starting 10 s before its stream's end, so that it is
two thirds padding.  All figures come from one process on one device, host clocks around calls that end in
torch.cuda.synchronize(); each is the median (and the fastest) of --repeats repeats after --warmup warm-ups.

  lfr     80-band Kaldi fbank, Splice.lfr(): seven frames stacked at a stride of six, [32, 560, 500]
  deltas  13-row Kaldi MFCC, Splice.deltas(): the features and their first and second deltas, [32, 39, 3000]
  (a) read_mel(.., "ct") followed by torch: per window, at its own valid_frames, replicate padding, unfold (LFR) or conv1d with the
      combined filters (deltas), cat
  (b) read_mel(.., "ct", splice=)
  (c) clx_splice_windows alone on (a)'s batch (device events), in microseconds and TB/s of the bytes it reads once and writes once,
      beside a torch device-to-device copy of as many bytes

Writes one JSON line per figure to --out (default profiles/splice_probe.txt)."""
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


def torch_splice(x, vf, splice):
    """The framework route on x [B, rows, T] (a new tensor): what clx_splice_windows defines, by torch's own operations."""
    import torch
    F = torch.nn.functional
    B, rows, T = x.shape
    s = splice.stride
    H = max(abs(o) + (0 if c is None else len(c) // 2) for o, c in splice.blocks)
    y = torch.full((B, splice.n_out(rows), splice.frames_out(T)), splice.pad, dtype=x.dtype, device=x.device)
    for k, V in enumerate(vf):
        if V == 0:
            continue
        Vo = splice.frames_out(V)
        p = F.pad(x[k:k + 1, :, :V], (H, H + s), mode="replicate")[0]          # frame t of the window is p[:, t + H]
        parts = []
        for o, c in splice.blocks:
            if c is None:
                parts.append(p[:, H + o:H + o + (Vo - 1) * s + 1:s])
            else:
                m = len(c) // 2
                w = torch.tensor(c, dtype=x.dtype, device=x.device).view(1, 1, -1)
                parts.append(F.conv1d(p[:, None, H + o - m:H + o + m + (Vo - 1) * s + 1], w, stride=s)[:, 0])
        y[k, :, :Vo] = torch.cat(parts, dim=0)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_probe.txt"))
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
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), windows=B, frames=FRAMES, short_windows=int((sid % 4 == 3).sum()),
         repeats=args.repeats, warmup=args.warmup)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def alone(fn, nbytes):
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
        return dict(median_us=round(us, 1), min_us=round(min(ts), 1), tb_per_s=round(nbytes / us / 1e6, 3))

    for name, spec, splice in (("lfr", cx.MelSpec.kaldi(ctx), cx.Splice.lfr()), ("deltas", cx.MelSpec.mfcc(ctx), cx.Splice.deltas())):
        x, vf = sset.read_mel(sid, starts, FRAMES, spec, layout="ct")
        vf = vf.numpy()
        torch.cuda.synchronize()

        def route_a():
            y, v = sset.read_mel(sid, starts, FRAMES, spec, layout="ct")
            return torch_splice(y, vf, splice), v

        def route_b():
            return sset.read_mel(sid, starts, FRAMES, spec, layout="ct", splice=splice)

        a = torch_splice(x, vf, splice)                      # (on a batch that is complete: every step waited for)
        torch.cuda.synchronize()
        b = route_b()[0]
        torch.cuda.synchronize()
        emit(what="%s: agreement" % name, shape=list(b.shape), max_abs_diff=float((a - b).abs().max()), max_abs_cell=float(b.abs().max()),
             words_that_differ=int((a.view(torch.int32) != b.view(torch.int32)).sum()))
        ta, tb = times(route_a, args.repeats, args.warmup), times(route_b, args.repeats, args.warmup)
        emit(what="%s: read_mel, then torch (a)" % name, **ta)
        emit(what="%s: read_mel, splice= (b)" % name, **tb)
        emit(what="%s: ratio" % name, a_over_b=round(ta["median_ms"] / tb["median_ms"], 3))
        out = torch.empty_like(b)
        nbytes = 4 * (int(vf.sum()) * spec.n_out + out.numel())                 # the live input cells once, every output cell once
        xt = x.transpose(1, 2).contiguous()
        for layout, src, what in ((cx.WINDOW_CT, x, "CT"), (cx.WINDOW_TC, xt, "TC")):
            emit(what="%s: clx_splice_windows alone (c), %s" % (name, what),
                 **alone(lambda: ctx.splice_windows((src.data_ptr(), B, spec.n_out, FRAMES), vf, layout, splice, out=out.data_ptr(),
                                                    stream=torch.cuda.current_stream()), nbytes))
        n = nbytes // 8
        c0, c1 = torch.empty(n, dtype=torch.float32, device=x.device), torch.empty(n, dtype=torch.float32, device=x.device)
        emit(what="%s: torch device-to-device copy of as many bytes" % name, **alone(lambda: c1.copy_(c0), 8 * n))
        spec.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
