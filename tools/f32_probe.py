"""Float output against the routes it replaces, in bench.py's pipelined form: config 3 (and config 4) with 24 distinct copies of the
input on the device, clx_batch_submit rotating over the batch's submit_depth outputs, 20 and 96 steps, the modes alternating in one
process.  Modes: planar i32; CLX_OUT_F32; CLX_OUT_PCM16; planar + clx_batch_interleave(CLX_SAMPLE_F32) (the two-pass route).
Prints one JSON line per (config, mode, steps): the median ms per step over the repeats."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import claxon_amd as cx  # noqa: E402
import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, nargs="+", default=[20, 96])
    ap.add_argument("--configs", nargs="+", default=["config3", "config4"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    ctx = cx.Context(0, wait_s=120)
    lines = []
    for cfg in args.configs:
        w = getattr(synth, cfg)(args.frames)
        descs = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)[0]
        arenas = [torch.from_numpy(w.arena).cuda() for _ in range(24)]
        modes = {"planar": 0, "f32": cx.OUT_F32, "pcm16": cx.OUT_PCM16, "planar+interleave_f32": 0} if cfg == "config3" else \
                {"planar": 0, "f32": cx.OUT_F32}
        batches = {m: ctx.plan(descs, w.out_offs, verify_crc=True, path=f) for m, f in modes.items()}
        depth = max(b.submit_depth for b in batches.values())
        outs = [torch.empty(w.pcm.size, dtype=torch.int32, device="cuda") for _ in range(depth)]
        pcm = [torch.empty(w.pcm.size, dtype=torch.float32, device="cuda") for _ in range(depth)]
        times = {(m, s): [] for m in modes for s in args.steps}

        def steps(m, n):
            b = batches[m]
            for i in range(n):
                b.submit(arenas[i % 24].data_ptr(), w.arena_len, outs[i % depth].data_ptr())
                if m == "planar+interleave_f32":
                    b.interleave(outs[i % depth].data_ptr(), pcm[i % depth].data_ptr(), cx.SAMPLE_F32)
            b.flush()
            torch.cuda.synchronize()

        for m in modes:
            steps(m, 8)                                       # (warm-up: plans, staging, code objects)
            assert np.all(batches[m].results()["status"] == cx.OK), m
        for _ in range(args.repeats):
            for s in args.steps:
                for m in modes:
                    t0 = time.perf_counter()
                    steps(m, s)
                    times[(m, s)].append((time.perf_counter() - t0) * 1e3 / s)
        for (m, s), v in times.items():
            line = {"config": cfg, "mode": m, "steps": s, "ms_per_step": round(float(np.median(v)), 4), "all": [round(x, 4) for x in v]}
            lines.append(line)
            print(json.dumps(line), flush=True)
        for b in batches.values():
            b.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
