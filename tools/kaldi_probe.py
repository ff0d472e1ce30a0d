"""Kaldi's fbank ([B, 80, 2998] of 30 s at 16 kHz: frames of 400 every 160, whole frames only) straight from a resident shard:
StreamSet.read_mel with MelSpec.kaldi against read() followed by the framework's operations, and the launch of clx_mel_windows
alone.  Workload: 32 synthetic mono FLAC streams of a little over 30 s at 16 kHz, 16 bits, blocks of 4096; one window of 480 000
samples (2998 frames) from the start of each.  All figures come from one process on one device, host clocks around calls
that end in torch.cuda.synchronize() (device events on a stream of their own for the launches alone); each is the median (and the
fastest) of --repeats repeats after --warmup warm-ups.

  (a) read(..., sample_rate=16000, channels=1), then unfold into frames, the frame's mean subtracted, the pre-emphasis, the window,
      a pad to 512, rfft, the squared magnitudes of the first 256 bins, a matmul against the spec's filterbank, clamp and log
      (torchaudio.compliance.kaldi.fbank's steps)
  (b) one read_mel
  (c) clx_mel_windows alone on (a)'s audio (clx_k_mel_f), in microseconds

The figure of record is (b) against (a).  Writes one JSON line per figure to --out (default profiles/kaldi_probe.txt)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kaldi_probe.txt"))
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
    spec = cx.MelSpec.kaldi(ctx)
    L = spec.window_len(N_FRAMES)
    assert L == SECONDS * R - 80 and int(min(sset.lengths)) >= L
    win_t = torch.from_numpy(spec.window).cuda()
    fb_t = torch.from_numpy(spec.fbank).cuda()               # [n_mels, n_bins]
    sid, starts = np.arange(B), np.zeros(B, dtype=np.int64)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), streams=B, window_samples=L, frames=N_FRAMES, rate=R, bits=16,
         block=mel_probe.BS, n_fft=spec.n_fft, win_length=spec.win_length, hop=spec.hop, n_mels=spec.n_mels, repeats=args.repeats, warmup=args.warmup)

    def framework(audio):
        x = audio.view(B, L).unfold(1, spec.win_length, spec.hop)                             # [B, T, Nw]
        x = x - x.mean(dim=2, keepdim=True)
        x = x - spec.preemph * torch.nn.functional.pad(x, (1, 0), mode="replicate")[..., :-1]
        st = torch.fft.rfft(torch.nn.functional.pad(x * win_t, (0, spec.n_fft - spec.win_length)), dim=2)[..., :spec.n_bins]
        return torch.log(torch.clamp((st.abs() ** 2) @ fb_t.T, min=spec.floor)).transpose(1, 2)   # [B, n_mels, T]

    def route_a():
        return framework(sset.read(sid, starts, L, "ct", sample_rate=R, channels=1)[0])

    def route_b():
        return sset.read_mel(sid, starts, N_FRAMES, spec)[0]

    want, got = route_a(), route_b()
    torch.cuda.synchronize()
    assert got.shape == want.shape == (B, spec.n_mels, N_FRAMES)
    emit(what="(a) against (b): largest difference of the outputs", max_abs_diff=float((got - want).abs().max()))
    for _ in range(2):                                       # (alternating: twice each)
        emit(what="(a) read + unfold, mean, pre-emphasis, window, pad, rfft, |.|^2, matmul, log", **mel_probe.times(route_a, args.repeats, args.warmup))
        emit(what="(b) read_mel with MelSpec.kaldi", **mel_probe.times(route_b, args.repeats, args.warmup))
    audio, valid = sset.read(sid, starts, L, "ct", sample_rate=R, channels=1)
    audio, valid = audio.view(B, L), valid.numpy()
    out = torch.empty((B, spec.n_mels, N_FRAMES), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    inner, ts = 5, []
    with torch.cuda.stream(side):
        for r in range(args.warmup + args.repeats):
            ev0.record(side)
            for _ in range(inner):
                ctx.mel_windows(spec, audio, valid, N_FRAMES, cx.WINDOW_CT, out, stream=side)
            ev1.record(side)
            torch.cuda.synchronize()
            if r >= args.warmup:
                ts.append(ev0.elapsed_time(ev1) / inner)
    emit(what="(c) clx_mel_windows alone (clx_k_mel_f, back to back: the table's upload of each call included)",
         median_us=round(float(np.median(ts)) * 1e3, 2), min_us=round(min(ts) * 1e3, 2))
    emit(what="(c') the framework's operations alone on the same audio", **mel_probe.times(lambda: framework(audio), args.repeats, args.warmup))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
