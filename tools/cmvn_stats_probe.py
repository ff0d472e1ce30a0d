"""CMVN statistics accumulated inside the read, and the per-speaker normalisation, against the framework routes behind it.  Workload:
32 synthetic mono FLAC streams of 32 s at 16 kHz, 16 bits, blocks of 4096; one window of 3000 frames per stream, every fourth one
starting 10 s before its stream's end, so that it is two thirds padding.  All figures come from one process on one device, host
clocks around calls that end in torch.cuda.synchronize(); each is the median (and the fastest) of --repeats repeats after --warmup
warm-ups.  Routes (a) and (b) of a pair are timed alternately in one loop, a, b, a, b, .., so that a drift of the device's clocks
or of the host falls on both alike.

  fbank  80-band Kaldi fbank: [32, 80, 3000]
  lfr    the same behind Splice.lfr(): [32, 560, 500]
  stats    (a) read_mel(.., "ct"[, splice=]) followed by torch: the padding mask, then float64 sums of x and of x * x over batch and
               time, and the count
           (b) read_mel(.., "ct"[, splice=], stats=CmvnStats)
  grouped  8 speakers, window k speaker k mod 8, a CmvnStats of 8 groups filled beforehand:
           (a) read_mel followed by a per-speaker torch loop: (x[speaker's windows] + shift) * scale, then the padding mask
           (b) read_mel(.., cmvn=Cmvn.grouped(stats), groups=)
  (c) the launches alone on (a)'s batch (device events), in microseconds and TB/s of the bytes they read once (and, the apply, write
      once), beside a torch device-to-device copy of as many bytes

Writes one JSON line per figure to --out (default profiles/cmvn_stats_probe.txt)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from norm_probe import FS, N_STREAMS, flac_stream  # noqa: E402

FRAMES, SPEAKERS = 3000, 8


def times_pair(fa, fb, reps, warmup):
    """Host milliseconds of fa and fb, each call ended by a synchronise, the two alternated in one loop: (a's, b's) figures."""
    import time
    import torch
    ts = ([], [])
    for i in range(warmup + reps):
        for j, fn in enumerate((fa, fb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                ts[j].append((time.perf_counter() - t0) * 1e3)
    return tuple({"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)} for t in ts)


def torch_stats(x, vf):
    """The framework route on x [B, rows, T]: float64 [2, rows + 1] in Kaldi's layout."""
    import torch
    live = torch.arange(x.shape[2], device=x.device)[None, None, :] < torch.as_tensor(vf.astype(np.int64), device=x.device)[:, None, None]
    xd = torch.where(live, x.double(), torch.zeros((), dtype=torch.float64, device=x.device))
    out = torch.zeros((2, x.shape[1] + 1), dtype=torch.float64, device=x.device)
    out[0, :-1] = xd.sum(dim=(0, 2))
    out[1, :-1] = (xd * xd).sum(dim=(0, 2))
    out[0, -1] = float(vf.sum())
    return out


def torch_grouped(x, vf, groups, shift, scale, pad):
    """The framework route on x [B, rows, T] (a new tensor): a loop over the speakers, then the padding mask."""
    import torch
    y = torch.empty_like(x)
    for g in range(shift.shape[0]):
        ks = torch.as_tensor(np.nonzero(groups == g)[0], device=x.device)
        y[ks] = (x[ks] + shift[g][None, :, None]) * scale[g][None, :, None]
    live = torch.arange(x.shape[2], device=x.device)[None, None, :] < torch.as_tensor(vf.astype(np.int64), device=x.device)[:, None, None]
    return torch.where(live, y, torch.full_like(y, pad))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmvn_stats_probe.txt"))
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
    groups = (sid % SPEAKERS).astype(np.int32)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), windows=B, frames=FRAMES, short_windows=int((sid % 4 == 3).sum()),
         speakers=SPEAKERS, repeats=args.repeats, warmup=args.warmup)
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
        return dict(median_us=round(us, 1), min_us=round(min(ts), 1), max_us=round(max(ts), 1), tb_per_s=round(nbytes / us / 1e6, 3))

    spec = cx.MelSpec.kaldi(ctx)
    for name, splice in (("fbank", None), ("lfr", cx.Splice.lfr())):
        x, vf = sset.read_mel(sid, starts, FRAMES, spec, layout="ct", splice=splice)
        vf = vf.numpy()
        torch.cuda.synchronize()
        rows, frames = int(x.shape[1]), int(x.shape[2])
        one, per = cx.CmvnStats(ctx, rows), cx.CmvnStats(ctx, rows, SPEAKERS)

        # ---- the statistics
        def stats_a():
            y, v = sset.read_mel(sid, starts, FRAMES, spec, layout="ct", splice=splice)
            return torch_stats(y, v.numpy())

        def stats_b():
            one.reset()
            return sset.read_mel(sid, starts, FRAMES, spec, layout="ct", splice=splice, stats=one)

        a = torch_stats(x, vf).cpu().numpy()
        stats_b()
        b = one.numpy()
        rel = np.abs(a - b)[:, :-1] / np.maximum(np.abs(b)[:, :-1], 1e-300)
        emit(what="%s stats: agreement" % name, shape=list(b.shape), count=float(b[0, -1]), count_equal=bool(a[0, -1] == b[0, -1]),
             max_rel_diff=float(rel.max()))
        ta, tb = times_pair(stats_a, stats_b, args.repeats, args.warmup)
        # (every timed (b) was a reset followed at once by the read: the accumulator holds one batch's sums, not twelve)
        emit(what="%s stats: after the timed loop" % name, words_that_differ_from_one_pass=int((one.numpy().view(np.uint64) != b.view(np.uint64)).sum()))
        emit(what="%s stats: read_mel, then torch (a)" % name, **ta)
        emit(what="%s stats: read_mel, stats= (b)" % name, **tb)
        emit(what="%s stats: ratio" % name, a_over_b=round(ta["median_ms"] / tb["median_ms"], 3))

        # ---- the per-speaker normalisation
        per.accumulate(x, vf, cx.WINDOW_CT, groups)
        st = per.numpy()
        cmvn = cx.Cmvn.grouped(per)
        sh = np.stack([cx.Cmvn.from_kaldi_stats(st[g]).shift for g in range(SPEAKERS)])
        sc = np.stack([cx.Cmvn.from_kaldi_stats(st[g]).scale for g in range(SPEAKERS)])
        d_sh, d_sc = torch.from_numpy(sh).to(x.device), torch.from_numpy(sc).to(x.device)

        def grouped_a():
            y, v = sset.read_mel(sid, starts, FRAMES, spec, layout="ct", splice=splice)
            return torch_grouped(y, v.numpy(), groups, d_sh, d_sc, 0.0), v

        def grouped_b():
            return sset.read_mel(sid, starts, FRAMES, spec, layout="ct", splice=splice, cmvn=cmvn, groups=groups)

        a = torch_grouped(x, vf, groups, d_sh, d_sc, 0.0)
        torch.cuda.synchronize()
        b = grouped_b()[0]
        torch.cuda.synchronize()
        emit(what="%s grouped: agreement" % name, shape=list(b.shape), max_abs_diff=float((a - b).abs().max()), max_abs_cell=float(b.abs().max()),
             words_that_differ=int((a.view(torch.int32) != b.view(torch.int32)).sum()))
        ta, tb = times_pair(grouped_a, grouped_b, args.repeats, args.warmup)
        emit(what="%s grouped: read_mel, then torch (a)" % name, **ta)
        emit(what="%s grouped: read_mel, cmvn=grouped, groups= (b)" % name, **tb)
        emit(what="%s grouped: ratio" % name, a_over_b=round(ta["median_ms"] / tb["median_ms"], 3))

        # ---- the launches alone
        live = 4 * int(vf.sum()) * rows
        xt = x.transpose(1, 2).contiguous()
        cur = torch.cuda.current_stream()
        for layout, src, what in ((cx.WINDOW_CT, x, "CT"), (cx.WINDOW_TC, xt, "TC")):
            emit(what="%s stats: the launches alone (c), %s" % (name, what),
                 **alone(lambda: per.accumulate((src.data_ptr(), B, rows, frames), vf, layout, groups, stream=cur), live))
            work = src.clone()                               # (in place: it runs again and again on its own output)
            emit(what="%s grouped: the launches alone (c), %s" % (name, what),
                 **alone(lambda: ctx.cmvn_windows((work.data_ptr(), B, rows, frames), vf, layout, cmvn, stream=cur, groups=groups), live + 4 * x.numel()))
        for label, nbytes in (("stats", live), ("grouped", live + 4 * x.numel())):
            n = nbytes // 8
            c0, c1 = torch.empty(n, dtype=torch.float32, device=x.device), torch.empty(n, dtype=torch.float32, device=x.device)
            emit(what="%s %s: torch device-to-device copy of as many bytes" % (name, label), **alone(lambda: c1.copy_(c0), 8 * n))
        one.close()
        per.close()
    spec.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
