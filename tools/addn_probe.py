"""Several placed or looped noises mixed inside the read (read(add=[...]), clx_addn_windows), against the framework routes behind the
reads and against clx_add_windows.  Workload: 32 synthetic mono FLAC streams of 32 s at 16 kHz, 16 bits, blocks of 4096; one window
of 30 s per stream.  All figures come from one process on one device; host clocks around calls that end in
torch.cuda.synchronize(), or device events around the launches alone; each is the median (and the fastest and slowest) of --repeats
repeats after --warmup warm-ups.  Routes (a) and (b) of a pair are timed alternately in one loop, a, b, a, b, .., so that a drift
of the device's clocks or of the host falls on both alike.

  loop     one 10 s noise (the last 10 s of the next stream) looped under every window
  babble   five other streams summed into every window, each at its own snr
  read     (a) the reads followed by torch: the noise tiled by an index gather, masked float64 energies, the gains, x + sum g n
           (b) read(.., add=[...])
  alone    clx_addn_windows between two device events on the read's batches, in microseconds and TB/s of the bytes its kernels touch
           (the sums read the signal and what each term hears; the apply pass reads both again and writes the signal), beside a
           torch device-to-device copy of as many bytes
  plain    one term a window, offset 0, no loop: (a) clx_add_windows, (b) clx_addn_windows, on the same batch, between device events

Writes one JSON line per figure to --out (default profiles/addn_probe.txt)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cmvn_stats_probe import times_pair  # noqa: E402
from norm_probe import FS, N_STREAMS, flac_stream  # noqa: E402

SECONDS, NOISE_SECONDS, BABBLE = 30, 10, 5


def torch_mix(x, v, noises, periods, loops, snrs):
    """The framework route on x [B, 1, L] (a new tensor): per term the noise [B, 1, L] heard through an index gather (looped from its
    period on), the masked float64 energies, the gain against the clean signal, and the sum."""
    import torch
    L = x.shape[2]
    t = torch.arange(L, device=x.device)[None, None, :]
    vs = torch.as_tensor(v.astype(np.int64), device=x.device)[:, None, None]
    live = t < vs
    es = torch.where(live, x.double() ** 2, 0.0).sum(dim=(1, 2))
    y = x.clone()
    for noise, P, loop, snr in zip(noises, periods, loops, snrs):
        p = torch.as_tensor(P.astype(np.int64), device=x.device)[:, None, None]
        heard = torch.gather(noise, 2, (t % p.clamp(min=1)).expand(-1, 1, -1)) if loop else noise
        on = live & (t < p) if not loop else live & (p > 0)
        en = torch.where(on, heard.double() ** 2, 0.0).sum(dim=(1, 2))
        nc = on.sum(dim=(1, 2)).double()
        g = torch.sqrt(es * nc * 10.0 ** (-snr / 10.0) / (en * vs[:, 0, 0].double())).float()
        y = y + torch.where(on, g[:, None, None] * heard, 0.0)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "addn_probe.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=N_STREAMS)
    args = ap.parse_args()
    import torch
    import claxon_amd as cx
    import synth
    synth.build()
    B = args.streams
    ctx = cx.Context(0, wait_s=120)
    sset = cx.open_streams(ctx, [flac_stream(k) for k in range(B)])
    assert sset.problems == [None] * B
    T, L = int(sset.lengths[0]), SECONDS * FS
    sid, starts = np.arange(B), np.zeros(B, dtype=np.int64)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), windows=B, samples=L, noise_samples=NOISE_SECONDS * FS, babble_terms=BABBLE,
         repeats=args.repeats, warmup=args.warmup)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    side = torch.cuda.Stream(device="cuda:0")                # (a stream of torch's own: on the default one the launches would go to the
                                                             # context's stream, and the events would not bracket them)

    def alone_pair(fa, fb):
        """Device microseconds of fa and fb between two events on `side`, where both run, alternated in one loop."""
        ts = ([], [])
        for i in range(args.warmup + args.repeats):
            for j, fn in enumerate((fa, fb)):
                torch.cuda.synchronize()
                ev0.record(side)
                with torch.cuda.stream(side):
                    fn()
                ev1.record(side)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ts[j].append(ev0.elapsed_time(ev1) * 1e3)
        return tuple(dict(median_us=round(float(np.median(t)), 1), min_us=round(min(t), 1), max_us=round(max(t), 1)) for t in ts)

    recipes = {
        "loop": [cx.Add((sid + 1) % B, np.full(B, T - NOISE_SECONDS * FS), 10.0, tile=True)],
        "babble": [cx.Add((sid + 1 + i) % B, np.full(B, 1000 * i), 5.0 + 2.0 * i) for i in range(BABBLE)],
    }
    for name, adds in recipes.items():
        S = len(adds)
        loops, snrs = [bool(a.tile[0]) for a in adds], [float(a.snr_db[0]) for a in adds]

        def reads():
            x, v = sset.read(sid, starts, L, "ct")
            ns = [sset.read(a.stream_ids, a.starts, L, "ct") for a in adds]
            return x, v.numpy(), [n for n, _ in ns], [p.numpy() for _, p in ns]

        def route_a():
            x, v, ns, ps = reads()
            return torch_mix(x, v, ns, ps, loops, snrs)

        def route_b():
            return sset.read(sid, starts, L, "ct", add=adds)[0]

        a, b = route_a(), route_b()
        torch.cuda.synchronize()
        emit(what="%s read: agreement" % name, shape=list(b.shape), max_abs_diff=float((a - b).abs().max()), max_abs_cell=float(b.abs().max()))
        ta, tb = times_pair(route_a, route_b, args.repeats, args.warmup)
        emit(what="%s read: the reads, then torch (a)" % name, **ta)
        emit(what="%s read: read(add=[...]) (b)" % name, **tb)
        emit(what="%s read: ratio" % name, a_over_b=round(ta["median_ms"] / tb["median_ms"], 3))

        # ---- the launches alone, on the read's batches stacked as read() stacks them (one source: one batch)
        x, v, ns, ps = reads()
        noise, pv = torch.cat(ns), np.concatenate(ps)
        first = np.arange(B + 1) * S
        index = (np.arange(B)[:, None] + B * np.arange(S)[None, :]).reshape(-1)
        loop = np.tile(np.array(loops, dtype=np.uint32), B)
        snr = np.tile(np.array(snrs, dtype=np.float32), B)
        heard = sum(int(v[k]) if loops[s] else min(int(v[k]), int(ps[s][k])) for k in range(B) for s in range(S))
        nbytes = 4 * (3 * int(v.sum()) + 2 * heard)
        work = x.clone()                                     # (in place: it runs again and again on its own output)
        torch.cuda.synchronize()

        def addn():
            ctx.addn_windows((work.data_ptr(), B, 1, L), v, [(noise.data_ptr(), B * S)], pv, first, 0, index, 0, loop, snr, cx.WINDOW_CT, stream=side)

        n = nbytes // 8
        c0, c1 = torch.empty(n, dtype=torch.float32, device=x.device), torch.empty(n, dtype=torch.float32, device=x.device)
        ta, tb = alone_pair(addn, lambda: c1.copy_(c0))
        emit(what="%s alone: clx_addn_windows" % name, bytes=nbytes, tb_per_s=round(nbytes / ta["median_us"] / 1e6, 3), **ta)
        emit(what="%s alone: torch device-to-device copy of as many bytes" % name, tb_per_s=round(8 * n / tb["median_us"] / 1e6, 3), **tb)

    # ---- one plain term a window: clx_add_windows against clx_addn_windows
    x, v = sset.read(sid, starts, L, "ct")
    noise, pv = sset.read((sid + 1) % B, np.full(B, 2 * FS), L, "ct")       # (the noise ends 2 s before the window does)
    v, pv = v.numpy(), pv.numpy()
    wa, wb = x.clone(), x.clone()
    ga, gb = torch.empty(B, dtype=torch.float32, device=x.device), torch.empty(B, dtype=torch.float32, device=x.device)
    torch.cuda.synchronize()

    def plain_add():
        ctx.add_windows((wa.data_ptr(), B, 1, L), v, (noise.data_ptr(), B), pv, np.arange(B), 10.0, cx.WINDOW_CT, gains=ga.data_ptr(), stream=side)

    def plain_addn():
        ctx.addn_windows((wb.data_ptr(), B, 1, L), v, [(noise.data_ptr(), B)], pv, np.arange(B + 1), 0, np.arange(B), 0, 0, 10.0, cx.WINDOW_CT,
                         gains=gb.data_ptr(), stream=side)

    plain_add()
    plain_addn()
    torch.cuda.synchronize()
    emit(what="plain: agreement after one call each", words_that_differ=int((wa.view(torch.int32) != wb.view(torch.int32)).sum()),
         gains_that_differ=int((ga.view(torch.int32) != gb.view(torch.int32)).sum()))
    ta, tb = alone_pair(plain_add, plain_addn)
    emit(what="plain: clx_add_windows (a)", **ta)
    emit(what="plain: clx_addn_windows, one term a window (b)", **tb)
    emit(what="plain: ratio", b_over_a=round(tb["median_us"] / ta["median_us"], 3),
         a_spread=round((ta["max_us"] - ta["min_us"]) / ta["median_us"], 3), b_spread=round((tb["max_us"] - tb["min_us"]) / tb["median_us"], 3))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
