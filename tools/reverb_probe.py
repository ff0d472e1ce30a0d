"""Reverberation inside the read against the framework route behind two reads.  Workload: 32 synthetic mono FLAC streams of 32 s at
16 kHz, 16 bits, blocks of 4096, as speech, and 32 streams of decaying noise behind a direct path as room impulse responses; one
window of 30 s per stream, every fourth starting 10 s before its stream's end (two thirds padding); responses truncated to 800,
4 000 and 16 000 taps (50 ms, 250 ms, 1 s).  All figures come from one process on one device, host clocks around calls that end in
torch.cuda.synchronize(); each is the median (and the fastest) of --repeats repeats after --warmup warm-ups.  Per tap count:

  (a) read(.., "ct", reverb=Reverb(.., taps=K, keep_power=True))              against
  (b) read(.., "ct") and source.read(.., K, "ct") followed by torch: rfft of both at the next power of two above L + K, the
      product, irfft, the crop to L, the mask from valid and the rescale to the dry power
  (c) clx_reverb_windows alone on (b)'s batches with keep_power off -- the FIR launch -- (device events), in milliseconds and in
      FLOP/s of the fused multiply-adds it performs (2 per tap per live sample, the taps that reach before the crop not counted)
      against the fp32 vector peak of the device, 157.3 TFLOP/s

The direct form's work grows with the taps and the FFT's does not: the figures are recorded as measured, also where (a) loses.
Writes one JSON line per figure to --out (default profiles/reverb_probe.txt)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from norm_probe import BS, FS, N_STREAMS, WINDOW_S, flac_stream, times  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12
TAPS = (800, 4000, 16000)


def rir_stream(k, n_frames=4):
    """A mono 16 kHz FLAC stream of n_frames * 4096 samples: a direct path and exponentially decaying noise (T60 about 0.6 s)."""
    import synth
    rng = np.random.default_rng(9000 + k)
    t = np.arange(n_frames * BS)
    h = rng.normal(0, 5000, t.size) * np.exp(-t / (0.087 * FS))
    h[0] = 24000
    x = np.clip(np.round(h), -32768, 32767).astype(np.int32)[None]
    fp = [synth.FrameParams() for _ in range(n_frames)]
    for i, f in enumerate(fp):
        f.number = i
        f.sf[0] = synth.sf(synth.SF_LPC, order=8, precision=12, partition_order=4)
    w = synth.encode_frames("rir", x.reshape(1, n_frames, BS).transpose(1, 0, 2), 1, BS, 16, fp, sample_rate=FS)
    si = bytearray(34)
    si[0:2] = BS.to_bytes(2, "big"); si[2:4] = BS.to_bytes(2, "big")
    si[10:14] = ((FS << 12) | (15 << 4)).to_bytes(4, "big")
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + bytes(si) + w.arena[:w.arena_len].tobytes()


def torch_reverb(x, v, h):
    """The framework route: x [B, 1, L], h [B, 1, K], v [B] on the device.  The causal convolution cropped to L, live samples only,
    rescaled to the dry power."""
    import torch
    L, K = x.shape[-1], h.shape[-1]
    n = 1 << (L + K - 1).bit_length()
    live = torch.arange(L, device=x.device).view(1, 1, L) < v.view(-1, 1, 1)
    xm = x * live
    y = torch.fft.irfft(torch.fft.rfft(xm, n) * torch.fft.rfft(h, n), n)[..., :L] * live
    ex, ey = (xm.double() ** 2).sum((1, 2)), (y.double() ** 2).sum((1, 2))
    g = torch.where((ex > 0) & (ey > 0), torch.sqrt(ex / ey.clamp(min=1e-300)), torch.ones_like(ex)).float()
    return y * g.view(-1, 1, 1), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reverb_probe.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--streams", type=int, default=N_STREAMS)
    args = ap.parse_args()
    import torch
    import claxon_amd as cx
    import synth
    synth.build()
    B = args.streams
    ctx = cx.Context(0, wait_s=120)
    speech = cx.open_streams(ctx, [flac_stream(k) for k in range(B)])
    rirs = cx.open_streams(ctx, [rir_stream(k) for k in range(B)])
    assert speech.problems == [None] * B and rirs.problems == [None] * B
    T = int(speech.lengths[0])
    L = WINDOW_S * FS
    sid = np.arange(B)
    starts = np.where(sid % 4 == 3, T - 10 * FS, 0)
    dev = "cuda:%d" % ctx.device
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), windows=B, seconds=WINDOW_S, rate=FS, short_windows=int((sid % 4 == 3).sum()),
         block=BS, taps=list(TAPS), repeats=args.repeats, warmup=args.warmup)
    side = torch.cuda.Stream(device=dev)                     # (a stream of torch's own: on the default one the launches would go to the
    for K in TAPS:                                           # context's stream, and the events would not bracket them)
        def fused():
            return speech.read(sid, starts, L, "ct", reverb=cx.Reverb(sid, rirs, taps=K, keep_power=True))

        def framework():
            x, v = speech.read(sid, starts, L, "ct")
            h, _ = rirs.read(sid, np.zeros(B, dtype=np.int64), K, "ct")
            y, g = torch_reverb(x, v.to(dev), h)
            return y, v, g

        a, b = fused(), framework()
        torch.cuda.synchronize()
        emit(what="agreement", taps=K, max_abs_diff=float((a[0] - b[0]).abs().max()), max_abs=float(b[0].abs().max()))
        ta, tb = times(fused, args.repeats, args.warmup), times(framework, args.repeats, args.warmup)
        emit(what="read(reverb=) (a)", taps=K, **ta)
        emit(what="read, read, then torch rfft / irfft (b)", taps=K, **tb)
        emit(what="ratio", taps=K, a_over_b=round(ta["median_ms"] / tb["median_ms"], 3), b_over_a=round(tb["median_ms"] / ta["median_ms"], 3))

        x, v = speech.read(sid, starts, L, "ct")
        h, hl = rirs.read(sid, np.zeros(B, dtype=np.int64), K, "ct")
        v, hl = v.numpy(), hl.numpy()
        out = torch.empty_like(x)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            ev0.record(side)
            ctx.reverb_windows(x, v, h.view(B, K), hl, sid, cx.WINDOW_CT, out=out, keep_power=False, stream=side)
            ev1.record(side)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(ev0.elapsed_time(ev1))
        ms = float(np.median(ts))
        n = np.minimum(hl.astype(np.int64), v.astype(np.int64))
        fmas = int((v.astype(np.int64) * n - n * (n - 1) // 2).sum())          # sum over t < v of min(t + 1, len)
        emit(what="clx_reverb_windows alone, keep_power off (c)", taps=K, median_ms=round(ms, 3), min_ms=round(min(ts), 3), gflop=round(2 * fmas / 1e9, 1),
             tflop_per_s=round(2 * fmas / ms / 1e9, 2), of_fp32_vector_peak=round(2 * fmas / (ms * 1e-3) / PEAK_FP32_VECTOR, 3))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
