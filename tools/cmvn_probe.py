"""Global and sliding-window CMVN inside the read against the framework route behind it.  Workload: 32 synthetic mono FLAC streams of
32 s at 16 kHz, 16 bits, blocks of 4096; one window of 3000 frames per stream, every fourth one starting 10 s before its stream's
end, so that it is two thirds padding.  All figures come from one process on one device, host clocks around calls that end in
torch.cuda.synchronize(); each is the median (and the fastest) of --repeats repeats after --warmup warm-ups.

  global   80-band Kaldi fbank, Splice.lfr(), a global Cmvn of 560 rows: [32, 560, 500]
  sliding  13-row Kaldi MFCC, Cmvn.xvector() (a centred window of 300 frames, means only): [32, 13, 3000]
  (a) read_mel(.., "ct"[, splice=]) followed by torch: global -- the broadcast (x + shift) * scale and the padding mask; sliding --
      per window, at its own valid_frames, a float64 cumsum and the window's ends by index
  (b) read_mel(.., "ct"[, splice=], cmvn=)
  (c) the launch alone on (a)'s batch (device events), in microseconds and TB/s of the bytes it reads once and writes once, beside a
      torch device-to-device copy of as many bytes

Writes one JSON line per figure to --out (default profiles/cmvn_probe.txt)."""
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


def torch_global(x, vf, shift, scale, pad):
    """The framework route on x [B, rows, T] (a new tensor): the broadcast expression, then the padding mask."""
    import torch
    y = (x + shift[None, :, None]) * scale[None, :, None]
    live = torch.arange(x.shape[2], device=x.device)[None, None, :] < torch.as_tensor(vf.astype(np.int64), device=x.device)[:, None, None]
    return torch.where(live, y, torch.full_like(y, pad))


def torch_sliding(x, vf, cmvn):
    """The framework route on x [B, rows, T] (a new tensor): per window a float64 cumsum, the statistics window's ends by index
    (centred, means only: what Cmvn.xvector() asks for)."""
    import torch
    N = cmvn.window
    y = torch.full_like(x, cmvn.pad)
    for k, V in enumerate(vf):
        V = int(V)
        if V == 0:
            continue
        t = torch.arange(V, device=x.device)
        a = (t - N // 2).clamp(min=0)
        b = a + N
        over = (b - V).clamp(min=0)
        a, b = (a - over).clamp(min=0), b.clamp(max=V)
        cs = torch.nn.functional.pad(x[k, :, :V].double().cumsum(dim=1), (1, 0))
        m = (cs[:, b] - cs[:, a]) / (b - a).double()
        y[k, :, :V] = (x[k, :, :V].double() - m).float()
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmvn_probe.txt"))
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

    rng = np.random.default_rng(3)
    glob = cx.Cmvn.global_(rng.uniform(3, 9, 560), rng.uniform(0.1, 0.5, 560))
    for name, spec, splice, cmvn in (("global", cx.MelSpec.kaldi(ctx), cx.Splice.lfr(), glob), ("sliding", cx.MelSpec.mfcc(ctx), None, cx.Cmvn.xvector())):
        x, vf = sset.read_mel(sid, starts, FRAMES, spec, layout="ct", splice=splice)
        vf = vf.numpy()
        torch.cuda.synchronize()
        rows, frames = int(x.shape[1]), int(x.shape[2])
        if cmvn.rows is not None:
            d_shift, d_scale = torch.from_numpy(cmvn.shift).to(x.device), torch.from_numpy(cmvn.scale).to(x.device)
            route = lambda y: torch_global(y, vf, d_shift, d_scale, cmvn.pad)   # noqa: E731
        else:
            route = lambda y: torch_sliding(y, vf, cmvn)                        # noqa: E731

        def route_a():
            y, v = sset.read_mel(sid, starts, FRAMES, spec, layout="ct", splice=splice)
            return route(y), v

        def route_b():
            return sset.read_mel(sid, starts, FRAMES, spec, layout="ct", splice=splice, cmvn=cmvn)

        a = route(x)                                         # (on a batch that is complete: every step waited for)
        torch.cuda.synchronize()
        b = route_b()[0]
        torch.cuda.synchronize()
        emit(what="%s: agreement" % name, shape=list(b.shape), max_abs_diff=float((a - b).abs().max()), max_abs_cell=float(b.abs().max()),
             words_that_differ=int((a.view(torch.int32) != b.view(torch.int32)).sum()))
        ta, tb = times(route_a, args.repeats, args.warmup), times(route_b, args.repeats, args.warmup)
        emit(what="%s: read_mel, then torch (a)" % name, **ta)
        emit(what="%s: read_mel, cmvn= (b)" % name, **tb)
        emit(what="%s: ratio" % name, a_over_b=round(ta["median_ms"] / tb["median_ms"], 3))
        nbytes = 4 * (int(vf.sum()) * rows + x.numel())                         # the live input cells once, every output cell once
        xt = x.transpose(1, 2).contiguous()
        out = torch.empty_like(x)
        for layout, src, what in ((cx.WINDOW_CT, x, "CT"), (cx.WINDOW_TC, xt, "TC")):
            work = src.clone()                               # (the global step is in place: it runs again and again on its own output)
            o_ptr = None if cmvn.rows is not None else out.data_ptr()
            emit(what="%s: the launch alone (c), %s" % (name, what),
                 **alone(lambda: ctx.cmvn_windows((work.data_ptr(), B, rows, frames), vf, layout, cmvn, out=o_ptr,
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
