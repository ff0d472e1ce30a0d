"""Per-utterance normalisation inside the read against the framework route behind it.  Workload: 32 synthetic mono FLAC streams of
32 s at 16 kHz, 16 bits, blocks of 4096; one window of 30 s per stream, every fourth one starting 10 s before its stream's end, so
that it is two thirds padding.  All figures come from one process on one device, host clocks around calls that end in
torch.cuda.synchronize(); each is the median (and the fastest) of --repeats repeats after --warmup warm-ups.

  (a) read_mel(.., MelSpec.kaldi, "tc", normalize=Norm.cmvn())           against
  (b) read_mel(.., MelSpec.kaldi, "tc") followed by torch: a mask from valid_frames, the masked mean and variance over the frames,
      subtract, divide, fill
  (c) read(.., "ct", normalize=Norm.wav2vec2())                          against
  (d) read(.., "ct") followed by the same torch ops over the samples
  (e) clx_norm_windows alone on (b)'s and (d)'s batches (device events), in microseconds and GB/s of the batch read three times and
      written once

Writes one JSON line per figure to --out (default profiles/norm_probe.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
FS, BS, SECONDS, N_STREAMS, WINDOW_S = 16000, 4096, 32, 32, 30


def flac_stream(k):
    import synth
    n_frames = (SECONDS * FS) // BS
    rng = np.random.default_rng(7000 + k)
    t = np.arange(n_frames * BS)
    x = np.clip(np.round(200 + 9000 * np.sin(2 * np.pi * (80 + k) * t / FS) + rng.normal(0, 300, t.size)), -32768, 32767).astype(np.int32)[None]
    fp = [synth.FrameParams() for _ in range(n_frames)]
    for i, f in enumerate(fp):
        f.number = i
        f.sf[0] = synth.sf(synth.SF_LPC, order=8, precision=12, partition_order=4)
    w = synth.encode_frames("probe", x.reshape(1, n_frames, BS).transpose(1, 0, 2), 1, BS, 16, fp, sample_rate=FS)
    si = bytearray(34)                                       # (no MD5, no sample count: neither is looked at here)
    si[0:2] = BS.to_bytes(2, "big"); si[2:4] = BS.to_bytes(2, "big")
    si[10:14] = ((FS << 12) | (15 << 4)).to_bytes(4, "big")
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


def torch_norm(x, valid, axis, eps, ddof=0):
    """The framework route: x [B, ...] normalised over `axis` (the time axis) up to valid[k], padding 0."""
    import torch
    T = x.shape[axis]
    shape = [1] * x.dim()
    shape[axis] = T
    live = torch.arange(T, device=x.device).view(shape) < valid.view([-1] + [1] * (x.dim() - 1))
    n = valid.clamp(min=1).view([-1] + [1] * (x.dim() - 1)).to(x.dtype)
    mean = (x * live).sum(axis, keepdim=True) / n
    d = (x - mean) * live
    var = (d * d).sum(axis, keepdim=True) / (n - ddof).clamp(min=1)
    return torch.where(live, d / torch.sqrt(var + eps), torch.zeros((), device=x.device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_probe.txt"))
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
    L = WINDOW_S * FS
    sid = np.arange(B)
    starts = np.where(sid % 4 == 3, T - 10 * FS, 0)
    spec = cx.MelSpec.kaldi(ctx)
    F = 1 + (L - spec.win_length) // spec.hop
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), windows=B, seconds=WINDOW_S, rate=FS, frames=F, n_mels=spec.n_out,
         short_windows=int((sid % 4 == 3).sum()), repeats=args.repeats, warmup=args.warmup)

    def mel_a():
        return sset.read_mel(sid, starts, F, spec, layout="tc", normalize=cx.Norm.cmvn())

    def mel_b():
        x, vf = sset.read_mel(sid, starts, F, spec, layout="tc")
        return torch_norm(x, vf.to(x.device), 1, 0.0), vf

    def wav_c():
        return sset.read(sid, starts, L, "ct", normalize=cx.Norm.wav2vec2())

    def wav_d():
        x, v = sset.read(sid, starts, L, "ct")
        return torch_norm(x, v.to(x.device), 2, 1e-7), v

    a, b = mel_a()[0], mel_b()[0]
    c, d = wav_c()[0], wav_d()[0]
    torch.cuda.synchronize()
    emit(what="agreement", mel_max_abs_diff=float((a - b).abs().max()), wav_max_abs_diff=float((c - d).abs().max()))
    ta, tb, tc, td = (times(f, args.repeats, args.warmup) for f in (mel_a, mel_b, wav_c, wav_d))
    emit(what="read_mel kaldi + cmvn: normalize= (a)", **ta)
    emit(what="read_mel kaldi, then torch (b)", **tb)
    emit(what="read + wav2vec2 norm: normalize= (c)", **tc)
    emit(what="read, then torch (d)", **td)
    emit(what="ratio", mel_b_over_a=round(tb["median_ms"] / ta["median_ms"], 3), wav_d_over_c=round(td["median_ms"] / tc["median_ms"], 3))

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, (x, v), layout, N in (("features [B, F, 80]", sset.read_mel(sid, starts, F, spec, layout="tc"), cx.WINDOW_TC, cx.Norm.cmvn()),
                                    ("waveform [B, 1, L]", sset.read(sid, starts, L, "ct"), cx.WINDOW_CT, cx.Norm.wav2vec2())):
        v = v.numpy()
        ts = []
        for i in range(args.warmup + args.repeats):
            y = x.clone()
            torch.cuda.synchronize()
            ev0.record()
            ctx.norm_windows(y, v, layout, N)
            ev1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(ev0.elapsed_time(ev1) * 1e3)
        us = float(np.median(ts))
        emit(what="clx_norm_windows alone (e): " + name, median_us=round(us, 1), min_us=round(min(ts), 1),
             gb_per_s=round(4 * x.numel() * 4 / us / 1e3, 1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
