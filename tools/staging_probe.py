"""Narrow-output batches whose groups the general kernels decode into staging rows: time per merged submission and the device memory
the plan and its submissions hold (torch.cuda.mem_get_info around them).  One JSON line per case.  CLAXON_HIP_LIB picks the library,
so builds can be compared.  Usage: python tools/staging_probe.py [--subs N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import claxon_amd as cx  # noqa: E402
import synth  # noqa: E402


def unique(n, ch, bs):
    rng = np.random.default_rng(ch * 100000 + bs)
    t = np.arange(bs)
    pcm = np.empty((n, ch, bs), dtype=np.int32)
    fps = []
    for i in range(n):
        for c in range(ch):
            pcm[i, c] = np.clip(np.rint(6000 * np.sin(2 * np.pi * (60 + 7 * i + 13 * c) * t / 44100.0) + rng.normal(0, 20, bs)), -32768, 32767)
        fp = synth.FrameParams(i % 4 if ch == 2 else 0, 0, synth.TILE_NUMBER_BASE + i)
        for c in range(ch):
            fp.sf[c] = synth.sf(synth.SF_FIXED, 2, 0, 0)
        fps.append(fp)
    return synth.encode_frames("u", pcm, ch, bs, 16, fps)


def used():
    import torch
    torch.cuda.synchronize()
    return -int(torch.cuda.mem_get_info(0)[0])


def run(name, w, mode, subs):
    import torch
    descs = cx.descs_from_offsets(w.arena[:w.arena_len], w.offs, w.lens, check_crc=False)[0]
    n_samples = int(w.out_offs[-1]) + int(w.channels[-1]) * int(w.block_sizes[-1])
    nb = 2 if mode == cx.OUT_PCM16 else 4
    ctx = cx.Context(0, wait_s=300)
    d_arena = torch.from_numpy(w.arena).cuda()
    u0 = used()
    batch = ctx.plan(descs, w.out_offs, verify_crc=True, path=mode)
    depth = batch.submit_depth
    outs = [torch.empty(n_samples * nb + 16, dtype=torch.uint8, device="cuda") for _ in range(depth)]
    for k in range(depth):                                   # warm-up: every stream's staging grown
        batch.submit(d_arena.data_ptr(), int(w.arena_len), outs[k].data_ptr())
    batch.flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(subs):
        batch.submit(d_arena.data_ptr(), int(w.arena_len), outs[k % depth].data_ptr())
    batch.flush()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    held = used() - u0 - sum(o.numel() for o in outs)
    ok = bool(np.all(batch.results()["status"] == cx.OK))
    batch.close(); ctx.close()
    print(json.dumps(dict(case=name, mode="pcm16" if mode == cx.OUT_PCM16 else "f32", lib=os.path.basename(cx.LIB_PATH), ok=ok,
                          ms_per_submission=round(1e3 * dt / subs, 3), held_gb=round(held / 1e9, 3),
                          one_output_gb=round(n_samples * nb / 1e9, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subs", type=int, default=48)
    a = ap.parse_args()
    long_ = synth.TiledStream(unique(64, 2, 65535), 2048).slice(0, 2048)
    six = synth.TiledStream(unique(64, 6, 4096), 2000).slice(0, 2000)
    short = synth.config3(1000)
    lone = unique(1, 2, 65535)
    mixed = synth.concat("one long", [short, lone, synth.config3(1000)])
    for name, w, modes in (("2048 x stereo 65535", long_, (cx.OUT_PCM16, cx.OUT_F32)), ("2000 x 6 ch 4096", six, (cx.OUT_PCM16, cx.OUT_F32)),
                           ("2000 x stereo 4096 + one 65535", mixed, (cx.OUT_PCM16,))):
        for m in modes:
            run(name, w, m, a.subs)


if __name__ == "__main__":
    main()
