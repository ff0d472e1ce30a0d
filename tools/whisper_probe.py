"""Whisper's encoder input (log_mel_spectrogram: [B, 80, 3000] of 30 s at 16 kHz) straight from a resident shard:
StreamSet.read_mel with MelSpec.whisper against read() followed by the framework's operations, and the two launches of
clx_mel_windows alone.  Workload: 32 synthetic mono FLAC streams of a little over 30 s at 16 kHz, 16 bits, blocks of 4096; one window
of 480 000 samples (3000 frames) from the start of each.  All figures come from one process on one device, host clocks around calls
that end in torch.cuda.synchronize() (device events on a stream of their own for the launches alone); each is the median (and the
fastest) of --repeats repeats after --warmup warm-ups.

  (a) read(..., sample_rate=16000, channels=1), then torch.stft(center=True, pad_mode="reflect") with the spec's window, the squared
      magnitudes of the first 3000 frames, a matmul against the spec's filterbank, clamp and log10, amax over each window, maximum
      with amax - 8, (x + 4) / 4
  (b) one read_mel
  (c) clx_mel_windows alone on (a)'s audio (clx_k_mel_c, then clx_k_mel_range), in microseconds

The figure of record is (b) against (a).  Writes one JSON line per figure to --out (default profiles/whisper_probe.txt)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_probe.txt"))
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
    spec = cx.MelSpec.whisper(ctx)
    L = spec.window_len(N_FRAMES)
    assert L == SECONDS * R and int(min(sset.lengths)) >= L
    win_t = torch.from_numpy(spec.window).cuda()
    fb_t = torch.from_numpy(spec.fbank).cuda()               # [n_mels, J]
    sid, starts = np.arange(B), np.zeros(B, dtype=np.int64)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), streams=B, window_samples=L, frames=N_FRAMES, rate=R, bits=16,
         block=mel_probe.BS, n_fft=spec.n_fft, hop=spec.hop, n_mels=spec.n_mels, repeats=args.repeats, warmup=args.warmup)

    def framework(audio):
        st = torch.stft(audio.view(B, L), spec.n_fft, hop_length=spec.hop, window=win_t, center=True, pad_mode="reflect", return_complex=True)
        x = torch.log10(torch.clamp(fb_t @ (st[..., :N_FRAMES].abs() ** 2), min=spec.floor))    # [B, n_mels, T]
        x = torch.maximum(x, x.amax(dim=(1, 2), keepdim=True) - spec.top)
        return (x + spec.shift) * spec.scale

    def route_a():
        return framework(sset.read(sid, starts, L, "ct", sample_rate=R, channels=1)[0])

    def route_b():
        return sset.read_mel(sid, starts, N_FRAMES, spec)[0]

    want, got = route_a(), route_b()
    torch.cuda.synchronize()
    assert got.shape == want.shape == (B, spec.n_mels, N_FRAMES)
    emit(what="(a) against (b): largest difference of the outputs", max_abs_diff=float((got - want).abs().max()))
    for _ in range(2):                                       # (alternating: twice each)
        emit(what="(a) read + stft(center), |.|^2, matmul, log10, amax, maximum, affine", **mel_probe.times(route_a, args.repeats, args.warmup))
        emit(what="(b) read_mel with MelSpec.whisper", **mel_probe.times(route_b, args.repeats, args.warmup))
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
    emit(what="(c) clx_mel_windows alone (clx_k_mel_c + clx_k_mel_range, back to back: the table's upload of each call included)",
         median_us=round(float(np.median(ts)) * 1e3, 2), min_us=round(min(ts) * 1e3, 2))
    emit(what="(c') the framework's operations alone on the same audio", **mel_probe.times(lambda: framework(audio), args.repeats, args.warmup))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
