"""Stream MD5 on the device (clx_md5_streams) against hashlib on the host.  Each part runs in a child process of its own under
`timeout -k`; the first part that fails ends the probe.  Writes profiles/md5_probe.txt (one JSON line per figure):
  a) one stream of 1, 8 and 32 MB of message: device call time, hashlib on one host core, D2H copy + hashlib;
  b) 64, 1024 and 8192 streams of 480 KB each (15 s of 16 kHz mono, 16-bit): aggregate device GB/s, against hashlib on one core;
  c) load_batch of 256 such FLAC streams with and without verify_md5.
Device times are host clocks around calls that end in a synchronise (clx_md5_streams returns with the digests on the host)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
PART_TIMEOUT = {"a": 300, "b": 600, "c": 900}


def _median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def part_a(ctx, emit):
    import torch
    for mb in (1, 8, 32):
        n = mb << 20
        d = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        host = d.cpu().numpy().tobytes()
        want = hashlib.md5(host).digest()
        got = ctx.md5_streams(d, 2, [0], [n // 2], [16])
        assert bytes(got[0]) == want
        t_dev = _median_time(lambda: ctx.md5_streams(d, 2, [0], [n // 2], [16]), 3)
        t_host = _median_time(lambda: hashlib.md5(host).digest(), 3)
        t_copy = _median_time(lambda: hashlib.md5(d.cpu().numpy().tobytes()).digest(), 3)
        emit(part="a", message_mb=mb, device_ms=round(t_dev * 1e3, 3), device_mb_s=round(mb / t_dev, 1), hashlib_ms=round(t_host * 1e3, 3),
             hashlib_mb_s=round(mb / t_host, 1), d2h_plus_hashlib_ms=round(t_copy * 1e3, 3))


def part_b(ctx, emit):
    import torch
    per = 240000                                                  # samples of 15 s at 16 kHz, 2 bytes each
    for n in (64, 1024, 8192):
        d = torch.randint(0, 256, (n * per * 2,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        first = np.arange(n, dtype=np.uint64) * per
        counts = np.full(n, per, dtype=np.uint64)
        bps = np.full(n, 16, dtype=np.uint8)
        got = ctx.md5_streams(d, 2, first, counts, bps)
        chk = d[:min(n, 64) * per * 2].cpu().numpy()
        for k in range(min(n, 64)):
            assert bytes(got[k]) == hashlib.md5(chk[k * per * 2:(k + 1) * per * 2].tobytes()).digest(), k
        t_dev = _median_time(lambda: ctx.md5_streams(d, 2, first, counts, bps), 3)
        t_host = _median_time(lambda: [hashlib.md5(chk[k * per * 2:(k + 1) * per * 2].tobytes()).digest() for k in range(8)], 3) / 8
        gb = n * per * 2 / 1e9
        emit(part="b", streams=n, stream_kb=per * 2 // 1000, device_ms=round(t_dev * 1e3, 3), device_gb_s=round(gb / t_dev, 2),
             hashlib_one_core_ms=round(t_host * n * 1e3, 1), hashlib_one_core_gb_s=round(per * 2 / 1e9 / t_host, 3),
             hashlib_16_cores_gb_s_if_linear=round(16 * per * 2 / 1e9 / t_host, 2))
        del d
        torch.cuda.empty_cache()


def _flac_stream(k, seconds=15, rate=16000, bs=4096):
    import synth
    n_frames = (seconds * rate) // bs
    rng = np.random.default_rng(1000 + k)
    t = np.arange(n_frames * bs)
    x = np.clip(np.round(9000 * np.sin(2 * np.pi * (80 + k) * t / rate) + rng.normal(0, 300, t.size)), -32768, 32767).astype(np.int64)
    fp = [synth.FrameParams() for _ in range(n_frames)]
    for i, f in enumerate(fp):
        f.number = i
        f.sf[0] = synth.sf(synth.SF_LPC, order=8, precision=12, partition_order=4)
    w = synth.encode_frames("probe", x.reshape(n_frames, 1, bs).astype(np.int32), 1, bs, 16, fp, sample_rate=rate)
    b = np.stack([x & 0xff, (x >> 8) & 0xff], axis=1).astype(np.uint8).tobytes()
    si = bytearray(34)
    si[0:2] = bs.to_bytes(2, "big"); si[2:4] = bs.to_bytes(2, "big")
    si[10:14] = ((rate << 12) | (0 << 9) | (15 << 4)).to_bytes(4, "big")
    si[14:18] = int(x.size).to_bytes(4, "big")
    si[18:34] = hashlib.md5(b).digest()
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + bytes(si) + w.arena[:w.arena_len].tobytes()


def part_c(ctx, emit):
    import claxon_amd as cx
    streams = [_flac_stream(k) for k in range(256)]
    for v in (False, True):
        cx.load_batch(ctx, streams, verify_md5=v)                  # (warm-up: code objects, allocations)
    for _ in range(2):
        for v in (False, True):
            t = _median_time(lambda: cx.load_batch(ctx, streams, verify_md5=v), 3)
            emit(part="c", streams=256, seconds_each=15, verify_md5=v, load_batch_ms=round(t * 1e3, 2))
    t = _median_time(lambda: cx.verify(ctx, streams), 3)
    emit(part="c", streams=256, seconds_each=15, call="verify", ms=round(t * 1e3, 2))


def run_part(part, out):
    import claxon_amd as cx
    ctx = cx.Context(0, wait_s=120)

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    {"a": part_a, "b": part_b, "c": part_c}[part](ctx, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c"], default=None, help="run one part in this process (the driver's child)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md5_probe.txt"))
    args = ap.parse_args()
    if args.part:
        run_part(args.part, args.out)
        return
    open(args.out, "w").close()
    for p in ("a", "b", "c"):
        st = subprocess.call(["timeout", "-k", "10", str(PART_TIMEOUT[p]), sys.executable, os.path.abspath(__file__), "--part", p, "--out", args.out])
        if st != 0:
            print("md5_probe: part %s ended with status %d; stopping" % (p, st), flush=True)
            sys.exit(st)


if __name__ == "__main__":
    main()
