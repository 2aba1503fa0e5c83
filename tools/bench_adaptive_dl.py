#!/usr/bin/env python3
"""DL-SCL retries on an adaptive baseline (pscl_adaptive_dlscl_device) against pscl_dlscl_device on
the same frames.

The headline shape: B = 10^6 distinct device-resident frames per step from channel_device, the
step's batch rotated over nbuf buffers as bench.py does, W warm-up steps and K >= 20 timed steps
between two HIP events, the final join inside the timed region.  In one process, for the (128,64)
code at 4 / 5 / 6 dB with L = 8 / beta_M8 and L = 4 / beta_M4 (retries 8), and for one
polarization-weight (256,128) point:

  dlscl        ms per step of Decoder.dlscl_device (the reference: its code is unchanged), on a plain
               handle and on a pipelined one, each timed --reps times; the spread is the margin
  three-stage  ms per step of Decoder.adaptive_dlscl_device, same rows, same run, both handles
  escalated    share of frames SC fails;  entries: frames per step that enter a retry chain
  main ms      kernel time on the handle's stream per step (pscl_timing_read_split), both calls
  host         pscl_host_stats of the pipelined runs: call and wait ms per call

One JSON line per point, then a table.  python tools/bench_adaptive_dl.py [--frames N] [--steps K]
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
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps  # ms per step


def pw_info_set(N, K):
    """The K positions of LARGEST polarization weight (sum of 2^(j / 4) over the set bits j of the
    index; ties to the larger index), ascending.  Not construct_info_set(method="polarization"): as
    the reference does, that one keeps the K smallest weights -- positions 0 .. -- on which no decoder
    passes a frame, so every frame would run all eight retry rounds."""
    i = np.arange(N)
    w = sum(((i >> j) & 1) * 2.0 ** (j / 4) for j in range(N.bit_length() - 1))
    return np.sort(np.argsort(w, kind="stable")[N - K:]).astype(np.int32)


def run_point(torch, dev, N, K, L, method, beta, ebno, B, steps, warmup, seed, reps, retries):
    from polar_code_amd import _native
    from polar_code_amd.polar.polar import construct_info_set

    info = pw_info_set(N, K) if method else construct_info_set(N, K)
    dec = _native.Decoder(N, info, L, POLY)
    dec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    W, kp = dec.W, K - 24
    nbuf = max(1, min(steps, int(48e9 // (B * N * 8))))
    llr = [torch.empty((B, N), dtype=torch.float64, device=dev) for _ in range(nbuf)]
    best = [torch.empty((B, W), dtype=torch.int64, device=dev) for _ in range(2)]
    flags = [torch.empty((B,), dtype=torch.uint8, device=dev) for _ in range(2)]
    att = [torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(2)]
    stage = torch.zeros((B,), dtype=torch.uint8, device=dev)
    for i in range(nbuf):
        dec.channel_device(seed, int(round(ebno * 10)), ebno, K / N, kp, i * B, B, llr[i].data_ptr(), 0)
    torch.cuda.synchronize(dev)

    def dlscl(i):
        dec.dlscl_device(llr[i % nbuf].data_ptr(), B, retries, beta=beta, d_best=best[i & 1].data_ptr(),
                         d_flags=flags[i & 1].data_ptr(), d_attempts=att[i & 1].data_ptr())

    def three(i, d_stage=0):
        dec.adaptive_dlscl_device(llr[i % nbuf].data_ptr(), B, retries, beta=beta, d_best=best[i & 1].data_ptr(),
                                  d_flags=flags[i & 1].data_ptr(), d_attempts=att[i & 1].data_ptr(), d_stage=d_stage)

    def nothing():
        pass

    # the shares, from one call's stages
    three(0, stage.data_ptr())
    dec.sync()
    escalated = int((stage >= 2).sum().item()) / B
    entries = int((stage == 3).sum().item())
    print(f"({N},{K}) L={L} {ebno} dB: {100 * escalated:.1f} % escalated, {entries} entries per step", file=sys.stderr, flush=True)
    out = {"code": f"({N},{K})" + (" pw" if method else ""), "L": L, "ebno_db": ebno, "frames_per_step": B, "steps": steps,
           "retries": retries, "escalated_share": escalated, "entries_per_step": entries, "build_hash": _native.build_hash()}
    for pipe in (False, True):
        tag = "pipelined" if pipe else "plain"
        dec.set_pipelined(pipe)
        tail = dec.join if pipe else nothing
        for name, fn in (("dlscl", dlscl), ("three_stage", three)):
            for i in range(warmup):
                fn(i)
            dec.join()
        ms = {"dlscl": [], "three_stage": []}
        for _ in range(reps):  # the reference and the new call alternate
            for name, fn in (("dlscl", dlscl), ("three_stage", three)):
                ms[name].append(timed(torch, dev, fn, steps, tail))
                print(f"  {tag} {name}: {ms[name][-1]:.3f} ms per step", file=sys.stderr, flush=True)
        for name, fn in (("dlscl", dlscl), ("three_stage", three)):
            out[f"{name}_{tag}_ms"] = ms[name]
            out[f"{name}_{tag}_fps"] = B / min(ms[name]) * 1e3
            # kernel time on the handle's stream, and the host's share (a pass of their own: the timing
            # events stay out of the wall measurement)
            dec.host_stats(reset=True)
            dec.timing_enable(True)
            for i in range(steps):
                fn(i)
            dec.join()
            (n_main, main_ms), (n_side, side_ms) = dec.timing_read_split()
            dec.timing_enable(False)
            call_ms, wait_ms, calls = dec.host_stats(reset=True)
            out[f"{name}_{tag}_main_ms"] = main_ms / steps
            out[f"{name}_{tag}_side_ms"] = side_ms / steps
            out[f"{name}_{tag}_host_call_ms"] = call_ms / max(calls, 1)
            out[f"{name}_{tag}_host_wait_ms"] = wait_ms / max(calls, 1)
    dec.set_pipelined(False)
    dec.sync()
    del llr, best, flags, att, stage
    dec.close()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=3, help="timed repeats of the reference and of the three-stage call")
    ap.add_argument("--retries", type=int, default=8)
    ap.add_argument("--pw-ebno", type=float, default=2.5, help="Eb/N0 of the polarization-weight (256,128) point")
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    betas = {L: np.load(ROOT / "tests" / "golden" / f"beta_M{L}.npy") for L in (8, 4)}
    points = [(128, 64, L, None, betas[L], ebno) for L in (8, 4) for ebno in (4.0, 5.0, 6.0)]
    points.append((256, 128, 8, "polarization", None, args.pw_ebno))
    rows = []
    stream = torch.cuda.Stream(dev)  # (the handle runs on it and the events bracket exactly its work)
    with torch.cuda.stream(stream):
        for N, K, L, method, beta, ebno in points:
            r = run_point(torch, dev, N, K, L, method, beta, ebno, args.frames, max(args.steps, 1), args.warmup, args.seed,
                          max(args.reps, 1), args.retries)
            rows.append(r)
            print(json.dumps(r), flush=True)

    def span(v):
        return f"{min(v):.3f} .. {max(v):.3f}"

    print()
    print("| code | dB | escalated | entries | dlscl ms | three-stage ms | dlscl pipelined ms | three-stage pipelined ms | "
          "three-stage Mf/s (plain, pipelined) | main-stream ms (dlscl, three-stage; pipelined) | host call / wait ms per "
          "pipelined call (dlscl; three-stage) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['code']} L={r['L']} | {r['ebno_db']:.1f} | {100 * r['escalated_share']:.1f} % | {r['entries_per_step']} | "
              f"{span(r['dlscl_plain_ms'])} | {span(r['three_stage_plain_ms'])} | {span(r['dlscl_pipelined_ms'])} | "
              f"{span(r['three_stage_pipelined_ms'])} | {r['three_stage_plain_fps'] / 1e6:.0f}, "
              f"{r['three_stage_pipelined_fps'] / 1e6:.0f} | {r['dlscl_pipelined_main_ms']:.3f}, "
              f"{r['three_stage_pipelined_main_ms']:.3f} | {r['dlscl_pipelined_host_call_ms']:.3f} / "
              f"{r['dlscl_pipelined_host_wait_ms']:.3f}; {r['three_stage_pipelined_host_call_ms']:.3f} / "
              f"{r['three_stage_pipelined_host_wait_ms']:.3f} |")


if __name__ == "__main__":
    main()
