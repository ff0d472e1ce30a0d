"""Log-mel features (n_fft 400, hop 160, 80 HTK bands, ln) of 1 s and 10 s windows from a resident shard: StreamSet.read_mel against
read() followed by the framework's operations on the same tables, and clx_mel_windows alone.  Workload: 256 synthetic mono FLAC
streams of 15 s at 16 kHz, 16 bits, blocks of 4096; one window per stream at a seeded random start.  All figures come from one
process on one device, host clocks around calls that end in torch.cuda.synchronize() (device events for the launch alone); each is
the median (and the fastest) of --repeats repeats after --warmup warm-ups.

  (a) read(..., sample_rate=16000, channels=1), then unfold, two matmuls against the spec's basis (cos and sin, built here in
      double and rounded once, as the library's), square and add, a matmul against the filterbank, clamp and log
  (b) one read_mel
  (c) clx_mel_windows alone on (a)'s audio, in microseconds and as a share of the fp32 vector peak (157.3 TFLOP/s), counting the
      DFT's and the band sums' multiply-adds of the live frames

The figure of record is (b) against (a).  Writes one JSON line per figure to --out (default profiles/mel_probe.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
R, BS, SECONDS, N_STREAMS = 16000, 4096, 15, 256
N_FFT, HOP, N_MELS, FLOOR = 400, 160, 80, 1e-10
PEAK_FP32 = 157.3e12


def flac_stream(k):
    import synth
    n_frames = (SECONDS * R) // BS
    rng = np.random.default_rng(7000 + k)
    t = np.arange(n_frames * BS)
    x = np.clip(np.round(9000 * np.sin(2 * np.pi * (80 + k) * t / R) + rng.normal(0, 300, t.size)), -32768, 32767).astype(np.int32)
    fp = [synth.FrameParams() for _ in range(n_frames)]
    for i, f in enumerate(fp):
        f.number = i
        f.sf[0] = synth.sf(synth.SF_LPC, order=8, precision=12, partition_order=4)
    w = synth.encode_frames("probe", x.reshape(1, n_frames, BS).transpose(1, 0, 2), 1, BS, 16, fp, sample_rate=R)
    si = bytearray(34)                                       # (no MD5, no sample count: neither is looked at here)
    si[0:2] = BS.to_bytes(2, "big"); si[2:4] = BS.to_bytes(2, "big")
    si[10:14] = ((R << 12) | (15 << 4)).to_bytes(4, "big")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_probe.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=N_STREAMS)
    args = ap.parse_args()
    import torch
    import claxon_amd as cx
    import synth
    synth.build()
    n_streams = args.streams
    streams = [flac_stream(k) for k in range(n_streams)]
    ctx = cx.Context(0, wait_s=120)
    sset = cx.open_streams(ctx, streams)
    assert sset.channels == [1] * n_streams and sset.sample_rates == [R] * n_streams
    spec = cx.MelSpec(ctx, R, n_fft=N_FFT, hop=HOP, n_mels=N_MELS, mode="ln", floor=FLOOR)
    J = N_FFT // 2 + 1
    ang = 2.0 * np.pi * ((np.arange(J)[:, None] * np.arange(N_FFT)[None, :]) % N_FFT) / N_FFT
    w64 = spec.window.astype(np.float64)[None, :]
    cos_t = torch.from_numpy((w64 * np.cos(ang)).astype(np.float32).T.copy()).cuda()          # [N, J]
    sin_t = torch.from_numpy((-w64 * np.sin(ang)).astype(np.float32).T.copy()).cuda()
    fb_t = torch.from_numpy(spec.fbank.T.copy()).cuda()                                        # [J, n_mels]
    T = int(sset.lengths[0])
    sid = np.arange(n_streams)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), streams=n_streams, seconds=SECONDS, rate=R, bits=16, block=BS, n_fft=N_FFT,
         hop=HOP, n_mels=N_MELS, mode="ln", repeats=args.repeats, warmup=args.warmup)
    for seconds in (1, 10):
        n_frames = (seconds * R - N_FFT) // HOP + 1
        L = spec.window_len(n_frames)
        starts = np.random.default_rng(seconds).integers(0, T - L, size=n_streams)

        def framework(audio):
            fr = audio.view(n_streams, L).unfold(1, N_FFT, HOP)                                # [B, T, N]
            p = (fr @ cos_t) ** 2 + (fr @ sin_t) ** 2
            return torch.log(torch.clamp(p @ fb_t, min=FLOOR)).transpose(1, 2)                  # [B, n_mels, T]

        def route_a():
            return framework(sset.read(sid, starts, L, "ct", sample_rate=R, channels=1)[0])

        def route_b():
            return sset.read_mel(sid, starts, n_frames, spec)[0]
        want, got = route_a(), route_b()
        assert got.shape == want.shape == (n_streams, N_MELS, n_frames)
        emit(what="(a) against (b), %d s windows: largest difference of the ln outputs" % seconds, frames=n_frames,
             max_abs_diff=float((got - want).abs().max()))
        for _ in range(2):                                   # (alternating: twice each)
            emit(what="(a) read + unfold, matmuls, square, matmul, log; %d s windows" % seconds, **times(route_a, args.repeats, args.warmup))
            emit(what="(b) read_mel; %d s windows" % seconds, **times(route_b, args.repeats, args.warmup))
        audio, valid = sset.read(sid, starts, L, "ct", sample_rate=R, channels=1)
        audio, valid = audio.view(n_streams, L), valid.numpy()
        out = torch.empty((n_streams, N_MELS, n_frames), dtype=torch.float32, device="cuda:0")
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        inner, ts = 10, []
        for r in range(args.warmup + args.repeats):
            ev0.record()
            for _ in range(inner):
                ctx.mel_windows(spec, audio, valid, n_frames, cx.WINDOW_CT, out)
            ev1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                ts.append(ev0.elapsed_time(ev1) / inner)
        med = float(np.median(ts))
        macs = n_streams * n_frames * (N_FFT * 2 * J + int(np.count_nonzero(spec.fbank)))
        emit(what="(c) clx_mel_windows alone, ct, %d s windows (back to back: the valid table's upload of each call included)" % seconds,
             median_us=round(med * 1e3, 2), min_us=round(min(ts) * 1e3, 2), gmacs=round(macs / 1e9, 3),
             tflop_per_s=round(2 * macs / med / 1e9, 2), share_of_fp32_vector_peak=round(2 * macs / (med * 1e-3) / PEAK_FP32, 4))
        emit(what="(c') the framework's operations alone on the same audio, %d s windows" % seconds,
             **times(lambda: framework(audio), args.repeats, args.warmup))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
