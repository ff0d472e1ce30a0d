"""Kaldi's fbank with snip_edges=false ([B, 80, 3000] of 30 s at 16 kHz: frames of 400 every 160, reflected at the crop's ends)
straight from a resident shard: StreamSet.read_mel with MelSpec.kaldi_reflected against what a user had to do without it -- read(),
a symmetric pad in torch and clx_mel_windows with MelSpec.kaldi -- and the launch of clx_k_mel_fr alone against clx_k_mel_f alone on
the same number of frames.  Workload: 32 synthetic mono FLAC streams of a little over 30 s at 16 kHz, 16 bits, blocks of 4096; one
window of 480 000 samples (3000 frames) from the start of each.  All figures come from one process on one device, host clocks around
calls that end in torch.cuda.synchronize() (device events on a stream of their own for the launches alone); each is the median (and
the fastest) of --repeats repeats after --warmup warm-ups, the routes alternating twice.

  (a) read(..., sample_rate=16000, channels=1), torch.cat of the flipped first 120 and last 120 samples around it, mel_windows with
      MelSpec.kaldi on the padded batch (whole frames: 3000 of them), against one read_mel with MelSpec.kaldi_reflected
  (b) clx_mel_windows alone: clx_k_mel_fr on (a)'s audio against clx_k_mel_f on (a)'s padded audio, in microseconds, twice each in
      turn; the two runs of clx_k_mel_f give its own run-to-run spread

The figure of record is (b).  Writes one JSON line per figure to --out (default profiles/reflected_probe.txt)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mel_probe  # noqa: E402  (flac_stream and times: the same synthetic streams, 30 s of them)

R, N_STREAMS, N_FRAMES, SECONDS = 16000, 32, 3000, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reflected_probe.txt"))
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
    refl, snip = cx.MelSpec.kaldi_reflected(ctx), cx.MelSpec.kaldi(ctx)
    L = SECONDS * R
    left = refl.win_length // 2 - refl.hop // 2              # 120
    Lp = snip.window_len(N_FRAMES)
    right = Lp - L - left                                    # 120
    assert refl.window_len(N_FRAMES) == L and int(min(sset.lengths)) >= L and (L + refl.hop // 2) // refl.hop == N_FRAMES and 0 <= right <= L
    sid, starts = np.arange(B), np.zeros(B, dtype=np.int64)
    full = np.full(B, Lp, dtype=np.uint32)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), streams=B, window_samples=L, frames=N_FRAMES, rate=R, bits=16,
         block=mel_probe.BS, n_fft=refl.n_fft, win_length=refl.win_length, hop=refl.hop, n_mels=refl.n_mels, pad_left=left, pad_right=right,
         repeats=args.repeats, warmup=args.warmup)

    def padded(audio):
        x = audio.view(B, L)
        return torch.cat([x[:, :left].flip(1), x, x[:, L - right:].flip(1)], dim=1).contiguous()

    def route_pad():
        out = torch.empty((B, snip.n_mels, N_FRAMES), dtype=torch.float32, device="cuda:0")
        ctx.mel_windows(snip, padded(sset.read(sid, starts, L, "ct", sample_rate=R, channels=1)[0]), full, N_FRAMES, cx.WINDOW_CT, out)
        return out

    def route_refl():
        return sset.read_mel(sid, starts, N_FRAMES, refl)[0]

    want, got = route_pad(), route_refl()
    torch.cuda.synchronize()
    assert got.shape == want.shape == (B, refl.n_mels, N_FRAMES)
    emit(what="(a) the two routes' outputs are the same words", equal=bool(torch.equal(got.view(torch.int32), want.view(torch.int32))))
    for _ in range(2):                                       # (alternating: twice each)
        emit(what="(a) read + symmetric pad in torch + mel_windows with MelSpec.kaldi", **mel_probe.times(route_pad, args.repeats, args.warmup))
        emit(what="(a) read_mel with MelSpec.kaldi_reflected", **mel_probe.times(route_refl, args.repeats, args.warmup))
    audio, valid = sset.read(sid, starts, L, "ct", sample_rate=R, channels=1)
    audio, valid = audio.view(B, L), valid.numpy()
    wide = padded(audio)
    out = torch.empty((B, refl.n_mels, N_FRAMES), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def launches(spec, a, v):
        inner, ts = 5, []
        with torch.cuda.stream(side):
            for r in range(args.warmup + args.repeats):
                ev0.record(side)
                for _ in range(inner):
                    ctx.mel_windows(spec, a, v, N_FRAMES, cx.WINDOW_CT, out, stream=side)
                ev1.record(side)
                torch.cuda.synchronize()
                if r >= args.warmup:
                    ts.append(ev0.elapsed_time(ev1) / inner)
        return dict(median_us=round(float(np.median(ts)) * 1e3, 2), min_us=round(min(ts) * 1e3, 2))

    f_runs, fr_runs = [], []
    for _ in range(2):
        f_runs.append(launches(snip, wide, full))
        emit(what="(b) clx_mel_windows alone, clx_k_mel_f on the padded batch (back to back: the table's upload of each call included)", **f_runs[-1])
        fr_runs.append(launches(refl, audio, valid))
        emit(what="(b) clx_mel_windows alone, clx_k_mel_fr on the batch as read", **fr_runs[-1])
    f_med, fr_med = [r["median_us"] for r in f_runs], [r["median_us"] for r in fr_runs]
    emit(what="(b) summary: clx_k_mel_fr over clx_k_mel_f (means of the two medians), and clx_k_mel_f's own spread between its two runs",
         ratio=round(sum(fr_med) / sum(f_med), 4), f_spread=round(abs(f_med[0] - f_med[1]) / min(f_med), 4),
         fr_spread=round(abs(fr_med[0] - fr_med[1]) / min(fr_med), 4))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
