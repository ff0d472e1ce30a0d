"""Kaldi's MFCC ([B, 13, 2998] of 30 s at 16 kHz: 23 bands, frames of 400 every 160, whole frames only) straight from a resident
shard: StreamSet.read_mel with MelSpec.mfcc against read_mel with the 23-band MelSpec.kaldi followed by the framework's matmul with
the DCT and the lifter product -- what a user could do before cepstral specs; it has no energy row -- and each route's launches
alone.  Workload: 32 synthetic mono FLAC streams of a little over 30 s at 16 kHz, 16 bits, blocks of 4096; one window of 480 000
samples (2998 frames) from the start of each.  All figures come from one process on one device, host clocks around calls that end
in torch.cuda.synchronize() (device events on a stream of their own for the launches alone); each is the median (and the fastest)
of --repeats repeats after --warmup warm-ups, the routes alternating.

  (a) read_mel with MelSpec.kaldi(n_mels=23), then torch.matmul with the DCT and a multiplication by the lifter
  (b) one read_mel with MelSpec.mfcc
  (c) the launches alone on the same audio, in microseconds: clx_mel_windows with the fbank spec (clx_k_mel_f) plus the framework's
      two operations, against clx_mel_windows with the MFCC spec (clx_k_mel_q)

The figure of record is (b) against (a).  Writes one JSON line per figure to --out (default profiles/mfcc_probe.txt)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mel_probe  # noqa: E402  (flac_stream and times: the same synthetic streams, 30 s of them)

R, N_STREAMS, N_FRAMES, SECONDS = 16000, 32, 2998, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mfcc_probe.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=N_STREAMS)
    args = ap.parse_args()
    import torch
    import claxon_amd as cx
    import synth
    synth.build()
    B = args.streams
    mel_probe.SECONDS = SECONDS + 1                          # (whole blocks of 4096: 31 s gives 121 of them, 495 616 samples)
    streams = [mel_probe.flac_stream(k) for k in range(B)]
    ctx = cx.Context(0, wait_s=120)
    sset = cx.open_streams(ctx, streams)
    assert sset.channels == [1] * B and sset.sample_rates == [R] * B
    fbank, mfcc = cx.MelSpec.kaldi(ctx, n_mels=23), cx.MelSpec.mfcc(ctx)
    L = mfcc.window_len(N_FRAMES)
    assert L == fbank.window_len(N_FRAMES) == SECONDS * R - 80 and int(min(sset.lengths)) >= L
    dct_t = torch.from_numpy(mfcc.dct).cuda()                # [n_ceps, n_mels]
    lift_t = torch.from_numpy(mfcc.lifter).cuda()[None, :, None]
    sid, starts = np.arange(B), np.zeros(B, dtype=np.int64)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), streams=B, window_samples=L, frames=N_FRAMES, rate=R, bits=16,
         block=mel_probe.BS, n_fft=mfcc.n_fft, win_length=mfcc.win_length, hop=mfcc.hop, n_mels=mfcc.n_mels, n_ceps=mfcc.n_ceps,
         repeats=args.repeats, warmup=args.warmup)

    def framework(y):                                        # [B, n_mels, T] -> [B, n_ceps, T]
        return torch.matmul(dct_t, y) * lift_t

    def route_a():
        return framework(sset.read_mel(sid, starts, N_FRAMES, fbank)[0])

    def route_b():
        return sset.read_mel(sid, starts, N_FRAMES, mfcc)[0]

    want, got = route_a(), route_b()
    torch.cuda.synchronize()
    assert got.shape == want.shape == (B, mfcc.n_ceps, N_FRAMES)
    emit(what="(a) against (b): largest difference of the outputs", max_abs_diff=float((got - want).abs().max()))
    for _ in range(2):                                       # (alternating: twice each)
        emit(what="(a) read_mel with MelSpec.kaldi(n_mels=23) + matmul with the DCT + the lifter product", **mel_probe.times(route_a, args.repeats, args.warmup))
        emit(what="(b) read_mel with MelSpec.mfcc", **mel_probe.times(route_b, args.repeats, args.warmup))
    audio, valid = sset.read(sid, starts, L, "ct", sample_rate=R, channels=1)
    audio, valid = audio.view(B, L), valid.numpy()
    out_f = torch.empty((B, fbank.n_mels, N_FRAMES), dtype=torch.float32, device="cuda:0")
    out_q = torch.empty((B, mfcc.n_ceps, N_FRAMES), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def launch_a():
        ctx.mel_windows(fbank, audio, valid, N_FRAMES, cx.WINDOW_CT, out_f, stream=side)
        framework(out_f)

    def launch_b():
        ctx.mel_windows(mfcc, audio, valid, N_FRAMES, cx.WINDOW_CT, out_q, stream=side)

    inner = 5
    for _ in range(2):                                       # (alternating: twice each)
        for what, launch in (("(c) (a)'s launches alone: clx_mel_windows (clx_k_mel_f), matmul, mul", launch_a),
                             ("(c) (b)'s launch alone: clx_mel_windows (clx_k_mel_q)", launch_b)):
            ts = []
            with torch.cuda.stream(side):
                for r in range(args.warmup + args.repeats):
                    ev0.record(side)
                    for _ in range(inner):
                        launch()
                    ev1.record(side)
                    torch.cuda.synchronize()
                    if r >= args.warmup:
                        ts.append(ev0.elapsed_time(ev1) / inner)
            emit(what=what + " (back to back: the table's upload of each call included)", median_us=round(float(np.median(ts)) * 1e3, 2),
                 min_us=round(min(ts) * 1e3, 2))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
