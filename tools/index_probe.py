"""The frame index in front of the whole-stream loaders: per-stream clx_index_frames_device calls (the parent commit's route) against one
clx_index_streams_device call.  Workload of profiles/md5_probe.txt part (c): 256 FLAC streams of 15 s, 16 kHz mono, 16 bits.

Every measurement runs in a child process of its own under `timeout -k`; the first child that fails ends the probe.  `--parent-dir DIR`
names a checkout of the parent commit whose claxon_amd/libclaxon_hip.so is built: its children import DIR's claxon_amd and load that
library (CLAXON_HIP_LIB), and parent and new children alternate (`--rounds` times each).  Without it only this tree is measured.
Times are host clocks around calls that end in a synchronise; each figure is the median and the fastest of `--repeats` repeats.

  breakdown  load_batch of the 256 streams cut into its steps (header parse, index, arena build + upload, plan, decode, MD5)
  loaders    load_batch with and without verify_md5, verify, load of one 15 s stream and of one 32 MB stream
  index      the index alone for n = 1, 64 and 1 024 streams and for one 32 MB stream: n calls of Context.index_frames, and (this tree)
             one call of Context.index_streams on a host arena and on a device arena
  calls      (for rocprofv3) one warm-up call and four timed calls of Context.index_streams with --n streams, nothing else

Writes one JSON line per figure to --out (default profiles/index_streams_probe.txt)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
PART_TIMEOUT = {"breakdown": 240, "loaders": 420, "index": 420, "calls": 180}


def _times(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def make_streams(path, n=256):
    """The probe's streams, generated once by the driver (tools/md5_probe.py's generator) and kept in an .npz for the children."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import md5_probe
    streams = [np.frombuffer(md5_probe._flac_stream(k), dtype=np.uint8) for k in range(n)]
    np.savez(path, *streams)


def load_streams(path):
    z = np.load(path)
    return [z["arr_%d" % k].tobytes() for k in range(len(z.files))]


def long_stream(cx, streams, target=32 << 20):
    """One stream of about `target` bytes: the first stream's header, then the frames of the streams over and over (a chain of valid
    frames: the indexer looks at headers and CRCs, not at frame numbers)."""
    parts, size = [], 0
    st, _, _, off = cx.read_stream_header(streams[0])
    parts.append(streams[0][:off])
    k = 0
    while size < target:
        s = streams[k % len(streams)]
        o = cx.read_stream_header(s)[3]
        parts.append(s[o:])
        size += len(s) - o
        k += 1
    return b"".join(parts)


def part_breakdown(cx, ctx, streams, emit, reps):
    import torch
    arrs = [cx._u8(s) for s in streams]
    batched = hasattr(ctx, "index_streams")

    def sync():
        torch.cuda.synchronize()

    def run():
        t = {}
        c0 = time.perf_counter()
        heads = [cx.read_stream_header(a) for a in arrs]
        t["header_parse"] = time.perf_counter() - c0
        offs, base = [], 0
        for a in arrs:
            offs.append(base)
            base = ((base + a.size + 15) // 16) * 16
        if not batched:
            c0 = time.perf_counter()
            idx = [ctx.index_frames(a, start=h[3]) for a, h in zip(arrs, heads)]
            t["index"] = time.perf_counter() - c0
            descs = []
            for (d, _, _), o, a in zip(idx, offs, arrs):
                d = d.copy()
                d["byte_off"] += np.uint64(o)
                descs.append(d)
            descs = np.concatenate(descs)
        c0 = time.perf_counter()
        arena = cx._arena_on_device(ctx, list(zip(offs, arrs)), base)
        sync()
        t["arena_build_upload"] = time.perf_counter() - c0
        if batched:
            c0 = time.perf_counter()
            descs, _, first, stops = ctx.index_streams(arena, offs, [a.size for a in arrs], [h[3] for h in heads])
            t["index"] = time.perf_counter() - c0
        c0 = time.perf_counter()
        bs = descs["block_size"].astype(np.uint64) * descs["n_channels"].astype(np.uint64)
        out_offs = np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64)
        out = torch.zeros(int(bs.sum()), dtype=torch.float32, device="cuda")
        sync()
        t["offsets_and_output_alloc"] = time.perf_counter() - c0
        c0 = time.perf_counter()
        batch = ctx.plan(descs, out_offs, verify_crc=True, path=cx.OUT_F32)
        t["plan"] = time.perf_counter() - c0
        c0 = time.perf_counter()
        batch.run(arena.data_ptr(), base, out.data_ptr())
        res = batch.results()
        t["decode_and_results"] = time.perf_counter() - c0
        assert np.all(res["status"] == 0)
        c0 = time.perf_counter()
        batch.close()
        t["plan_destroy"] = time.perf_counter() - c0
        t["frames"] = int(descs.size)
        return t

    run()
    runs = [run() for _ in range(reps)]
    keys = [k for k in runs[0] if k != "frames"]
    emit(part="breakdown", streams=len(streams), frames=runs[0]["frames"], repeats=reps,
         median_ms={k: round(float(np.median([r[k] for r in runs])) * 1e3, 3) for k in keys},
         sum_of_medians_ms=round(sum(float(np.median([r[k] for r in runs])) for k in keys) * 1e3, 3))


def part_loaders(cx, ctx, streams, emit, reps):
    one, big = streams[0], long_stream(cx, streams)
    for v in (False, True):
        cx.load_batch(ctx, streams, verify_md5=v)                  # (warm-up: code objects, allocations)
    cx.verify(ctx, streams)
    cx.load(ctx, one)
    cx.load(ctx, big)
    for v in (False, True):
        emit(part="loaders", call="load_batch", streams=len(streams), verify_md5=v, repeats=reps,
             **_times(lambda: cx.load_batch(ctx, streams, verify_md5=v), reps))
    emit(part="loaders", call="verify", streams=len(streams), repeats=reps, **_times(lambda: cx.verify(ctx, streams), reps))
    emit(part="loaders", call="load", stream_bytes=len(one), repeats=reps, **_times(lambda: cx.load(ctx, one), reps))
    emit(part="loaders", call="load", stream_bytes=len(big), repeats=reps, **_times(lambda: cx.load(ctx, big), reps))


def _shard(cx, streams):
    arrs = [cx._u8(s) for s in streams]
    starts = [cx.read_stream_header(a)[3] for a in arrs]
    offs, base = [], 0
    for a in arrs:
        offs.append(base)
        base = ((base + a.size + 15) // 16) * 16
    host = np.zeros(base + 32, dtype=np.uint8)
    for o, a in zip(offs, arrs):
        host[o:o + a.size] = a
    return arrs, host, base, offs, [a.size for a in arrs], starts


def part_index(cx, ctx, streams, emit, reps):
    import torch
    sets = [("n=1", streams[:1]), ("n=64", streams[:64]), ("n=1024", streams * 4), ("one 32 MB stream", [long_stream(cx, streams)])]
    for name, ss in sets:
        arrs, host, base, offs, lens, starts = _shard(cx, ss)

        def per_stream():
            return [ctx.index_frames(a, start=s) for a, s in zip(arrs, starts)]
        frames = sum(d.size for d, _, _ in per_stream())
        emit(part="index", case=name, route="index_frames per stream", streams=len(ss), frames=frames, arena_mb=round(base / 1e6, 2),
             repeats=reps, **_times(per_stream, reps))
        if hasattr(ctx, "index_streams"):
            dev = torch.from_numpy(host).cuda()
            got = ctx.index_streams(host[:base], offs, lens, starts)
            assert got[0].size == frames and ctx.index_streams(dev, offs, lens, starts)[0].tobytes() == got[0].tobytes()
            emit(part="index", case=name, route="index_streams, host arena", streams=len(ss), frames=frames, repeats=reps,
                 **_times(lambda: ctx.index_streams(host[:base], offs, lens, starts), reps))
            emit(part="index", case=name, route="index_streams, device arena", streams=len(ss), frames=frames, repeats=reps,
                 **_times(lambda: ctx.index_streams(dev, offs, lens, starts), reps))
            del dev


def part_calls(cx, ctx, streams, emit, n):
    ss = (streams * ((n + len(streams) - 1) // len(streams)))[:n]
    arrs, host, base, offs, lens, starts = _shard(cx, ss)
    for _ in range(5):                                                 # (one warm-up call that sizes the scratch, four more)
        d = ctx.index_streams(host[:base], offs, lens, starts)[0]
    emit(part="calls", streams=n, calls=5, frames=int(d.size))


def child(args):
    if args.kind == "parent":
        sys.path.insert(0, os.path.abspath(args.parent_dir))
    else:
        sys.path.insert(0, ROOT)
    import claxon_amd as cx
    assert os.path.abspath(cx.__file__).startswith(os.path.abspath(args.parent_dir if args.kind == "parent" else ROOT))
    ctx = cx.Context(0, wait_s=120)
    streams = load_streams(args.streams)

    def emit(**kw):
        line = json.dumps(dict(code=args.kind, **kw))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if args.part == "calls":
        part_calls(cx, ctx, streams, emit, args.n)
    else:
        {"breakdown": part_breakdown, "loaders": part_loaders, "index": part_index}[args.part](cx, ctx, streams, emit, args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=list(PART_TIMEOUT), default=None, help="run one part in this process (the driver's child)")
    ap.add_argument("--kind", choices=["new", "parent"], default="new")
    ap.add_argument("--parent-dir", default=None)
    ap.add_argument("--streams", default=None, help="the .npz of the probe's streams (made by the driver)")
    ap.add_argument("--make-streams", default=None, metavar="NPZ", help="only generate the probe's streams into this file")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_streams_probe.txt"))
    args = ap.parse_args()
    if args.make_streams:
        make_streams(args.make_streams)
        return
    if args.part:
        child(args)
        return
    tmp = tempfile.mkdtemp(prefix="index_probe_")
    npz = os.path.join(tmp, "streams.npz")
    make_streams(npz)
    open(args.out, "w").close()
    kinds = (["parent"] if args.parent_dir else []) + ["new"]
    for part in ("breakdown", "loaders", "index"):
        for _ in range(args.rounds if len(kinds) > 1 else 1):
            for kind in kinds:
                env = dict(os.environ)
                cmd = ["timeout", "-k", "10", str(PART_TIMEOUT[part]), sys.executable, os.path.abspath(__file__), "--part", part, "--kind", kind,
                       "--streams", npz, "--out", args.out, "--repeats", str(args.repeats)]
                if kind == "parent":
                    env["CLAXON_HIP_LIB"] = os.path.join(os.path.abspath(args.parent_dir), "claxon_amd", "libclaxon_hip.so")
                    cmd += ["--parent-dir", args.parent_dir]
                st = subprocess.call(cmd, env=env)
                if st != 0:
                    print("index_probe: part %s (%s) ended with status %d; stopping" % (part, kind, st), flush=True)
                    sys.exit(st)


if __name__ == "__main__":
    main()
