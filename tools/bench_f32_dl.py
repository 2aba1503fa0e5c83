#!/usr/bin/env python3
"""The three-stage decode on float32 rows against its float64 form on the same frames.

The shape of tools/bench_f32.py: B = 10^6 distinct device-resident frames per step from
channel_device, rounded to float32 once; the float64 form takes those rows widened once beforehand
(the same values), the step's batch rotated over nbuf buffers, W warm-up steps and K >= 20 timed
steps between two HIP events, the final join and synchronisation inside the timed region.  On a
plain and on a pipelined handle (depth 2, outputs alternating two sets) two variants alternate in
one run, --reps rounds each:

  f64      pscl_adaptive_dlscl_device on the widened rows.  Its kernels are the parent's: this is
           the yardstick, and its min .. max spread over the rounds is the noise margin
  f32      pscl_adaptive_dlscl_device_f32 on the float32 rows

One JSON line per variant, then a table.
python tools/bench_f32_dl.py [--frames N] [--steps K] [--reps R] [--ebno dB] [--L 8]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

POLY = "0x1864CFB"


def timed(torch, dev, fn, steps, tail):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for i in range(steps):
        fn(i)
    tail()
    e1.record()
    torch.cuda.synchronize(dev)  # (the events' stream: everything the steps queued has ended)
    return e0.elapsed_time(e1) / steps  # ms per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ebno", type=float, default=5.0)
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--retries", type=int, default=8)
    ap.add_argument("--nbuf", type=int, default=4)
    ap.add_argument("--seed", type=int, default=11)
    args = ap.parse_args()

    import torch

    from polar_code_amd import _native
    from polar_code_amd.polar.polar import construct_info_set

    dev = torch.device("cuda", 0)
    N, K, L, B, R = 128, 64, args.L, args.frames, args.retries
    beta = np.load(ROOT / "tests" / "golden" / f"beta_M{L}.npy")
    res = {}
    for pipelined in (False, True):
        dec = _native.Decoder(N, construct_info_set(N, K), L, POLY)
        if not dec.f32_available():
            raise SystemExit("no float32 kernels on this handle")
        dec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dec.set_beta(beta)
        kp, W = K - 24, dec.W
        llr32 = []
        for i in range(args.nbuf):
            x = torch.empty((B, N), dtype=torch.float64, device=dev)
            dec.channel_device(args.seed, int(round(args.ebno * 10)), args.ebno, K / N, kp, i * B, B, x.data_ptr(), 0)
            dec.sync()
            llr32.append(x.float())
            del x
        llr64 = [x.double() for x in llr32]  # (widened once beforehand: the same values)
        outs = [dict(d_best=torch.empty((B, W), dtype=torch.int64, device=dev), d_flags=torch.empty((B,), dtype=torch.uint8, device=dev),
                     d_stage=torch.empty((B,), dtype=torch.uint8, device=dev), d_attempts=torch.empty((B,), dtype=torch.int32, device=dev),
                     d_tried=torch.empty((B, R), dtype=torch.int32, device=dev), d_n_escalated=torch.zeros(1, dtype=torch.int32, device=dev))
                for _ in range(2)]
        ptrs = [{k: v.data_ptr() for k, v in o.items()} for o in outs]
        torch.cuda.synchronize(dev)
        if pipelined:
            dec.set_pipelined(True, depth=2)
        variants = {"f64": (dec.adaptive_dlscl_device, llr64), "f32": (dec.adaptive_dlscl_device_f32, llr32)}

        def step(name):
            call, rows = variants[name]
            return lambda i: call(rows[i % args.nbuf].data_ptr(), B, R, beta=beta, tried_stride=R, **ptrs[i & 1])

        tail = (lambda: (dec.join(), None)[1]) if pipelined else (lambda: None)
        for name in variants:
            timed(torch, dev, step(name), args.warmup, tail)
        ms = {name: [] for name in variants}
        for _ in range(args.reps):  # (interleaved rounds: f64, f32, f64, f32, ..)
            for name in variants:
                ms[name].append(timed(torch, dev, step(name), args.steps, tail))
        esc = int(outs[0]["d_n_escalated"].cpu()[0])
        ent = int((outs[0]["d_stage"] == 3).sum().cpu())
        for name, v in ms.items():
            res[(pipelined, name)] = v
            print(json.dumps({"call": "adaptive_dlscl", "rows": name, "pipelined": pipelined, "L": L, "ebno_db": args.ebno,
                              "frames": B, "steps": args.steps, "ms_per_step": [round(x, 4) for x in v], "escalated": esc,
                              "chain_entries": ent}), flush=True)
        dec.set_pipelined(False)
        dec.set_stream(None)
        dec.close()
        del llr32, llr64, outs
        torch.cuda.empty_cache()
    print(f"\n{B} frames per step, {args.ebno} dB, L = {L}, beta_M{L}, {args.steps} steps, {args.reps} rounds; ms per step, min .. max")
    print("| handle | f64 on widened rows | f32 rows | f32 / f64 (minima) | every f32 round below every f64 round |")
    print("|---|---|---|---|---|")
    for pipelined in (False, True):
        a, b = res[(pipelined, "f64")], res[(pipelined, "f32")]
        print(f"| {'pipelined' if pipelined else 'stream-ordered'} | {min(a):.3f} .. {max(a):.3f} | {min(b):.3f} .. {max(b):.3f} | "
              f"{min(b) / min(a):.3f} | {'yes' if max(b) < min(a) else 'no'} |")


if __name__ == "__main__":
    main()
