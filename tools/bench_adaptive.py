#!/usr/bin/env python3
"""Adaptive decoding (pscl_adaptive_device) against the plain list decode on the same frames.

The headline shape: B = 10^6 distinct device-resident frames per step from channel_device, the
step's batch rotated over nbuf buffers as bench.py does (no batch is decoded twice in a row from
a warm cache), W warm-up steps and K >= 20 timed steps between two HIP events, the final
synchronisation inside the timed region.  In one process, for the (128,64) code at L = 8 and
4.0 / 5.0 / 6.0 dB and for the NR (128,88) code with E = 256 at 5 dB:

  adaptive   frames/s of Decoder.adaptive_device (SC on every frame, L = 8 on the rest)
  plain      frames/s of Decoder.decode_device, stream-ordered, and pipelined as bench.py runs it
             (the unchanged baseline path)
  share      escalated frames / frames
  t_sc       the SC kernel's own time per step (pscl_timing_*: a pass at 20 dB, where no frame
             escalates, so the SC launch is the call's only timed launch; the kernel's work does
             not depend on the data)
  t_stage2   the timed stage-2 decode launches per step (total timed launches minus t_sc)
  floor      the SC kernel's HBM floor: row bytes per frame at 6.29 TB/s
  model      t_sc + share * t_plain (the cost model of DESIGN.md section 5.9), beside the measured step
  async      frames/s of Decoder.adaptive_async_device (no host wait, stage 2 a row-list launch) on the
             same rows in the same run, on a plain handle and on a pipelined one (stage 2 on the side
             stream); the synchronous call is the reference, timed --reps times, and its spread over
             those repeats is the noise margin.  --grids: the async call again per workgroup cap of
             the row-list launch (PSCL_TUNE_ADAPT_GRID; 1048576 = a grid sized for B)

One JSON line per point, then a table.  python tools/bench_adaptive.py [--frames N] [--steps K]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

POLY = "0x1864CFB"
HBM_BPS = 6.29e12


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


def run_point(torch, dev, N, K, L, E, ebno, B, steps, warmup, seed, reps=3, grids=()):
    from polar_code_amd import _native
    from polar_code_amd.polar.polar import construct_info_set

    info = construct_info_set(N, K)
    dec = _native.Decoder(N, info, L, POLY)
    if E:
        dec.set_rate_match(E)
    dec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    n_in, W, kp = E or N, dec.W, K - 24
    rate = kp / E if E else K / N
    nbuf = max(1, min(steps, int(48e9 // (B * n_in * 8))))
    llr = [torch.empty((B, n_in), dtype=torch.float64, device=dev) for _ in range(nbuf)]
    hot = torch.empty((B, n_in), dtype=torch.float64, device=dev)  # 20 dB: no frame escalates
    best = [torch.empty((B, W), dtype=torch.int64, device=dev) for _ in range(2)]
    flags = [torch.empty((B,), dtype=torch.uint8, device=dev) for _ in range(2)]
    for i in range(nbuf):
        dec.channel_device(seed, int(round(ebno * 10)), ebno, rate, kp, i * B, B, llr[i].data_ptr(), 0)
    dec.channel_device(seed, 200, 20.0, rate, kp, 0, B, hot.data_ptr(), 0)
    torch.cuda.synchronize(dev)
    esc = [0]

    def adaptive(i, rows=None):
        esc[0] += dec.adaptive_device((rows if rows is not None else llr[i % nbuf]).data_ptr(), B,
                                      d_best=best[i & 1].data_ptr(), d_flags=flags[i & 1].data_ptr())

    def plain(i):
        dec.decode_device(llr[i % nbuf].data_ptr(), B, d_best=best[i & 1].data_ptr(), d_flags=flags[i & 1].data_ptr())

    def nothing():
        pass

    for i in range(warmup):
        adaptive(i)
        plain(i)
    # the SC kernel alone (timing events around its launch)
    dec.timing_enable(True)
    esc[0] = 0
    for i in range(steps):
        adaptive(i, hot)
    n_sc, sc_ms = dec.timing_read()
    assert esc[0] == 0 and n_sc == steps, (esc[0], n_sc)
    dec.timing_enable(False)
    t_sc = sc_ms / steps
    # adaptive, untimed kernels (the events of pscl_timing_* stay out of the wall measurement)
    esc[0] = 0
    t_adaptive = timed(torch, dev, adaptive, steps, nothing)
    share = esc[0] / (steps * B)
    # the call without the host wait, same rows, same run: reference and new call alternate
    n_dev = torch.zeros(1, dtype=torch.int32, device=dev)

    def adaptive_async(i):
        dec.adaptive_async_device(llr[i % nbuf].data_ptr(), B, d_best=best[i & 1].data_ptr(), d_flags=flags[i & 1].data_ptr(),
                                  d_n_escalated=n_dev.data_ptr())

    for i in range(warmup):
        adaptive_async(i)
    ref_ms, async_ms, async_pipe_ms = [t_adaptive], [], []
    for r in range(reps):
        if r:
            ref_ms.append(timed(torch, dev, adaptive, steps, nothing))
        async_ms.append(timed(torch, dev, adaptive_async, steps, nothing))
    assert int(n_dev.cpu()[0]) > 0 or share == 0
    dec.set_pipelined(True)
    for i in range(warmup):
        adaptive_async(i)
    dec.join()
    for r in range(reps):
        async_pipe_ms.append(timed(torch, dev, adaptive_async, steps, dec.join))
    dec.set_pipelined(False)
    grid_ms = {}
    for g in grids:
        dec.set_tuning(adapt_grid=g)
        adaptive_async(0)
        grid_ms[str(g)] = min(timed(torch, dev, adaptive_async, steps, nothing) for _ in range(2))
    dec.set_tuning(adapt_grid=0)
    waits = dec.adaptive_stats()["host_waits"]
    # its timed launches: SC + the stage-2 decode
    dec.timing_enable(True)
    for i in range(steps):
        adaptive(i)
    n_l, tot_ms = dec.timing_read()
    dec.timing_enable(False)
    t_stage2 = tot_ms / steps - t_sc
    # the plain list decode of the same frames: stream-ordered, then pipelined as bench.py runs it
    t_plain = timed(torch, dev, plain, steps, nothing)
    dec.set_pipelined(True)
    for i in range(warmup):
        plain(i)
    dec.join()
    t_plain_pipe = timed(torch, dev, plain, steps, dec.join)
    dec.set_pipelined(False)
    dec.sync()
    del llr, hot, best, flags
    dec.close()
    torch.cuda.empty_cache()
    floor_ms = B * n_in * 8 / HBM_BPS * 1e3
    return {
        "code": f"({N},{K})" + (f" E={E}" if E else ""), "L": L, "ebno_db": ebno, "frames_per_step": B, "steps": steps,
        "adaptive_ms": t_adaptive, "adaptive_fps": B / t_adaptive * 1e3,
        "plain_ms": t_plain, "plain_fps": B / t_plain * 1e3,
        "plain_pipelined_ms": t_plain_pipe, "plain_pipelined_fps": B / t_plain_pipe * 1e3,
        "escalated_share": share, "t_sc_ms": t_sc, "t_stage2_kernels_ms": t_stage2, "timed_launches_per_step": n_l / steps,
        "sc_hbm_floor_ms": floor_ms, "sc_over_floor": t_sc / floor_ms,
        "model_ms": t_sc + share * t_plain, "build_hash": _native.build_hash(),
        "adaptive_ref_ms": ref_ms, "async_ms": async_ms, "async_pipelined_ms": async_pipe_ms, "async_grid_ms": grid_ms,
        "async_fps": B / min(async_ms) * 1e3, "async_pipelined_fps": B / min(async_pipe_ms) * 1e3, "async_host_waits": waits,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=3, help="timed repeats of the synchronous reference and the async call")
    ap.add_argument("--grids", type=str, default="", help="comma-separated workgroup caps of the row-list launch to time")
    args = ap.parse_args()
    grids = [int(g) for g in args.grids.split(",") if g]
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    points = [(128, 64, 8, 0, 4.0), (128, 64, 8, 0, 5.0), (128, 64, 8, 0, 6.0), (128, 88, 8, 256, 5.0)]
    rows = []
    # a stream of its own: the handle runs on it and the events bracket exactly its work (the default
    # stream's handle of 0 would select the decoder's own stream instead)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        for N, K, L, E, ebno in points:
            r = run_point(torch, dev, N, K, L, E, ebno, args.frames, max(args.steps, 1), args.warmup, args.seed,
                          max(args.reps, 1), grids)
            rows.append(r)
            print(json.dumps(r), flush=True)
    print()
    print("| code | dB | escalated | adaptive Mf/s | plain Mf/s | plain pipelined Mf/s | step ms | t_sc ms | floor ms | "
          "t_sc/floor | stage-2 kernels ms | model ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['code']} L={r['L']} | {r['ebno_db']:.1f} | {100 * r['escalated_share']:.1f} % | "
              f"{r['adaptive_fps'] / 1e6:.0f} | {r['plain_fps'] / 1e6:.0f} | {r['plain_pipelined_fps'] / 1e6:.0f} | "
              f"{r['adaptive_ms']:.3f} | {r['t_sc_ms']:.3f} | {r['sc_hbm_floor_ms']:.3f} | {r['sc_over_floor']:.2f} | "
              f"{r['t_stage2_kernels_ms']:.3f} | {r['model_ms']:.3f} |")
    print()
    print("| code | dB | sync adaptive ms (min .. max of the repeats) | async ms | async pipelined ms | async Mf/s | "
          "async pipelined Mf/s | host waits |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['code']} L={r['L']} | {r['ebno_db']:.1f} | {min(r['adaptive_ref_ms']):.3f} .. {max(r['adaptive_ref_ms']):.3f} | "
              f"{min(r['async_ms']):.3f} .. {max(r['async_ms']):.3f} | {min(r['async_pipelined_ms']):.3f} .. "
              f"{max(r['async_pipelined_ms']):.3f} | {r['async_fps'] / 1e6:.0f} | {r['async_pipelined_fps'] / 1e6:.0f} | "
              f"{r['async_host_waits']} |")
        if r["async_grid_ms"]:
            print("|  | row-list grid cap: " + ", ".join(f"{g}: {ms:.3f} ms" for g, ms in r["async_grid_ms"].items()) + " |")


if __name__ == "__main__":
    main()
