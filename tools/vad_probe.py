"""The energy VAD and the selection of the voiced frames inside the read against the framework route behind it.  Workload: 32
synthetic mono FLAC streams of 32 s at 16 kHz, 16 bits, blocks of 4096; one window of 3000 frames of 30-row Kaldi MFCC per stream,
every fourth one starting 10 s before its stream's end, so that it is two thirds padding: [32, 30, 3000].  All figures come from
one process on one device, host clocks around calls that end in torch.cuda.synchronize(); each is the median (and the fastest) of
--repeats repeats after --warmup warm-ups.

  (a) the x-vector front end with the VAD in torch: read_mel(.., "ct"), Context.cmvn_windows(Cmvn.xvector()) -- the two are
      read_mel(cmvn=Cmvn.xvector()) bit for bit, kept apart here because the decision needs the raw C0, which cmvn= releases --
      then per window, at its own valid_frames: the threshold from a float64 mean, a cumsum count over the context, the compare,
      boolean indexing, and pad_sequence over the batch.  The parent of this feature has no call for it: this is the baseline
  (b) read_mel(.., "ct", cmvn=Cmvn.xvector(), vad=Vad.voxceleb())
  (c) the launches alone on (a)'s batch (device events), in microseconds: the decision in both layouts; the selection in both
      layouts without its copy of the counts, with the bytes it reads and writes (the selected cells once, every output cell once,
      the mask twice) in TB/s, beside a torch device-to-device copy of as many bytes

Writes one JSON line per figure to --out (default profiles/vad_probe.txt)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from norm_probe import FS, N_STREAMS, flac_stream, times  # noqa: E402

FRAMES, CEPS = 3000, 30


def torch_vad_select(raw, normed, vf, vad):
    """The framework route: the decision on raw [B, rows, T], the selection on normed [B, rows, T] (a new tensor, and the counts)."""
    import torch
    E, s, c = vad.energy_threshold, vad.energy_mean_scale, vad.frames_context
    p = torch.tensor(vad.proportion_threshold, dtype=torch.float32, device=raw.device)
    T = raw.shape[2]
    kept, counts = [], []
    for k, V in enumerate(vf):
        V = int(V)
        e = raw[k, vad.row, :V]
        if V == 0:
            kept.append(normed[k, :, :0].T)
            counts.append(0)
            continue
        thr = (E + s * e.double().mean()).float() if s != 0 else torch.tensor(E, dtype=torch.float32, device=raw.device)
        cs = torch.nn.functional.pad((e > thr).to(torch.int32).cumsum(dim=0), (1, 0))
        t = torch.arange(V, device=raw.device)
        lo, hi = (t - c).clamp(min=0), (t + c).clamp(max=V - 1)
        voiced = (cs[hi + 1] - cs[lo]).float() >= (hi - lo + 1).float() * p
        kept.append(normed[k, :, :V][:, voiced].T)
        counts.append(int(kept[-1].shape[0]))                # (a wait a window: the ragged length is on the host)
    y = torch.nn.utils.rnn.pad_sequence(kept, batch_first=True, padding_value=vad.pad)
    y = torch.nn.functional.pad(y, (0, 0, 0, T - y.shape[1]), value=vad.pad)
    return y.transpose(1, 2).contiguous(), np.asarray(counts, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_probe.txt"))
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
    T = int(sset.lengths[0])
    sid = np.arange(B)
    starts = np.where(sid % 4 == 3, T - 10 * FS, 0)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    emit(what="workload", device=torch.cuda.get_device_name(0), windows=B, frames=FRAMES, rows=CEPS, short_windows=int((sid % 4 == 3).sum()),
         repeats=args.repeats, warmup=args.warmup)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def alone(fn, nbytes=None):
        ts = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            ev0.record()
            fn()
            ev1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(ev0.elapsed_time(ev1) * 1e3)
        us = float(np.median(ts))
        d = dict(median_us=round(us, 1), min_us=round(min(ts), 1))
        if nbytes is not None:
            d.update(bytes=int(nbytes), tb_per_s=round(nbytes / us / 1e6, 3))
        return d

    spec, cmvn, vad = cx.MelSpec.mfcc(ctx, n_ceps=CEPS, n_mels=CEPS), cx.Cmvn.xvector(), cx.Vad.voxceleb()
    raw, vf = sset.read_mel(sid, starts, FRAMES, spec, layout="ct")
    vf = vf.numpy()
    torch.cuda.synchronize()
    rows, frames = int(raw.shape[1]), int(raw.shape[2])
    assert rows == CEPS and frames == FRAMES

    def route_a():
        x, v = sset.read_mel(sid, starts, FRAMES, spec, layout="ct")
        normed = ctx.cmvn_windows(x, v.numpy(), cx.WINDOW_CT, cmvn)
        torch.cuda.synchronize()                             # (torch's stream is not ordered behind the context's)
        return torch_vad_select(x, normed, v.numpy(), vad)

    def route_b():
        return sset.read_mel(sid, starts, FRAMES, spec, layout="ct", cmvn=cmvn, vad=vad)

    a, ca = route_a()
    torch.cuda.synchronize()
    b, cb = route_b()
    torch.cuda.synchronize()
    emit(what="agreement", shape=list(b.shape), words_that_differ=int((a.view(torch.int32) != b.view(torch.int32)).sum()),
         counts_equal=bool(np.array_equal(ca, cb.numpy())), live_frames=int(vf.sum()), voiced_frames=int(cb.sum()))
    ta, tb = times(route_a, args.repeats, args.warmup), times(route_b, args.repeats, args.warmup)
    tc = times(lambda: sset.read_mel(sid, starts, FRAMES, spec, layout="ct", cmvn=cmvn), args.repeats, args.warmup)
    emit(what="read_mel, cmvn_windows, then torch (a)", **ta)
    emit(what="read_mel, cmvn=, vad= (b)", **tb)
    emit(what="read_mel, cmvn= alone (neither route's VAD)", **tc)
    emit(what="ratio", a_over_b=round(ta["median_ms"] / tb["median_ms"], 3))
    normed = ctx.cmvn_windows(raw, vf, cx.WINDOW_CT, cmvn)
    torch.cuda.synchronize()
    mask = torch.empty((B, frames), dtype=torch.uint8, device=raw.device)
    out = torch.empty_like(normed)
    st = torch.cuda.current_stream()
    valid = np.ascontiguousarray(vf, dtype=np.uint32)
    opts = cx._SelectOpts(0.0, (C.c_uint32 * 3)(0, 0, 0))
    moved = 4 * (int(cb.sum()) * rows + normed.numel()) + 2 * int(vf.sum())
    for layout, rw, nm, what in ((cx.WINDOW_CT, raw, normed, "CT"), (cx.WINDOW_TC, raw.transpose(1, 2).contiguous(), normed.transpose(1, 2).contiguous(), "TC")):
        emit(what="the decision alone (c), %s: clx_k_vad_sum, clx_k_vad_decide" % what,
             **alone(lambda: ctx.vad_windows((rw.data_ptr(), B, rows, frames), vf, layout, vad, mask=mask.data_ptr(), stream=st)))

        def select():
            rc = cx.lib().clx_select_windows(ctx._h, nm.data_ptr(), out.data_ptr(), B, rows, frames, valid.ctypes.data, mask.data_ptr(), layout,
                                             C.byref(opts), None, None, C.c_void_p(st.cuda_stream))
            assert rc == cx.OK
        emit(what="the selection alone (c), %s: clx_k_select_rank, _scan, _move, no copy of the counts" % what, **alone(select, moved))
    n = moved // 8
    c0, c1 = torch.empty(n, dtype=torch.float32, device=raw.device), torch.empty(n, dtype=torch.float32, device=raw.device)
    emit(what="torch device-to-device copy of as many bytes", **alone(lambda: c1.copy_(c0), 8 * n))
    spec.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
