#!/usr/bin/env python3
"""Staged decoding (pscl_sc_device + pscl_escalate_device) of the long codes against the plain
pipelined list decode of the same frames.

B distinct device-resident frames per step from channel_device (1 GiB of rows by default), the
step's batch rotated over nbuf buffers as bench.py does, W warm-up steps and K timed steps between
two HIP events, the final synchronisation inside the timed region.  In one process, at L = 8, for
the polarization-weight sets (256,128) and (512,256) at 2.5 dB and (1024,512) at 2.0 and 2.5 dB
(information sets a caller supplies), and for the reference's constructed sets (256,128) at 4 dB
and (1024,512) at 6 dB:

  share        escalated frames / frames
  t_sc         the SC kernel's own time per step (pscl_timing_*)
  floor        the SC kernel's HBM floor: row bytes per frame at 6.29 TB/s
  staged       frames/s of sc_device then escalate_device, batch after batch
  staged ahead frames/s with batch i + 1's sc_device enqueued before batch i's escalate_device
  two handles  the same order with the batches alternating between two handles on two streams: the
               host wait of one batch's escalation then leaves the other batch's SC stage running
  plain        frames/s of the pipelined Decoder.decode_device (the unchanged baseline path)
  async        frames/s of Decoder.adaptive_async_device (no host wait, stage 2 a row-list launch) on
               the same rows in the same run, on a plain handle and on a pipelined one (stage 2 on the
               side stream); `staged` is the reference, timed --reps times: its spread is the margin

One JSON line per point, then a table.  python tools/bench_staged.py [--bytes N] [--steps K]
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


def pw_info_set(N, K):
    """The K positions of largest polarization weight sum 2^(j / 4), ascending."""
    i = np.arange(N)
    w = sum(((i >> j) & 1) * 2.0 ** (j / 4) for j in range(N.bit_length() - 1))
    return np.sort(np.argsort(w, kind="stable")[N - K:]).astype(np.int32)


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


def run_point(torch, dev, kind, N, K, L, ebno, B, steps, warmup, seed, reps=3):
    from polar_code_amd import _native
    from polar_code_amd.polar.polar import construct_info_set

    info = pw_info_set(N, K) if kind == "pw" else construct_info_set(N, K)
    dec = _native.Decoder(N, info, L, POLY)
    dec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    side = torch.cuda.Stream(dev)
    decs = [dec, _native.Decoder(N, info, L, POLY)]
    decs[1].set_stream(side.cuda_stream)
    W, kp = dec.W, K - 24
    nbuf = max(2, min(steps, int(24e9 // (B * N * 8))))
    llr = [torch.empty((B, N), dtype=torch.float64, device=dev) for _ in range(nbuf)]
    out = [dict(d_best=torch.empty((B, W), dtype=torch.int64, device=dev),
                d_flags=torch.empty((B,), dtype=torch.uint8, device=dev),
                d_stage=torch.empty((B,), dtype=torch.uint8, device=dev)) for _ in range(2)]
    ptr = [{k: v.data_ptr() for k, v in o.items()} for o in out]
    for i in range(nbuf):
        dec.channel_device(seed, int(round(ebno * 10)), ebno, K / N, kp, i * B, B, llr[i].data_ptr(), 0)
    torch.cuda.synchronize(dev)
    esc = [0]

    def sc(i):
        dec.sc_device(llr[i % nbuf].data_ptr(), B, **ptr[i & 1])

    def escalate(i):
        esc[0] += dec.escalate_device(llr[i % nbuf].data_ptr(), B, **ptr[i & 1])

    def staged(i):
        sc(i)
        escalate(i)

    def staged_ahead(i):  # (batch 0's SC stage is queued before the loop)
        sc(i + 1)
        escalate(i)

    def two_handles(i):  # (batch 0's SC stage is queued before the loop; batch i runs on handle i & 1)
        decs[(i + 1) & 1].sc_device(llr[(i + 1) % nbuf].data_ptr(), B, **ptr[(i + 1) & 1])
        esc[0] += decs[i & 1].escalate_device(llr[i % nbuf].data_ptr(), B, **ptr[i & 1])

    def join_side():
        torch.cuda.current_stream(dev).wait_stream(side)

    def plain(i):
        dec.decode_device(llr[i % nbuf].data_ptr(), B, d_best=ptr[i & 1]["d_best"], d_flags=ptr[i & 1]["d_flags"])

    def nothing():
        pass

    for i in range(warmup):
        staged(i)
    dec.timing_enable(True)
    for i in range(steps):
        sc(i)
    n_sc, sc_ms = dec.timing_read()
    assert n_sc == steps, n_sc
    dec.timing_enable(False)
    esc[0] = 0
    t_staged = timed(torch, dev, staged, steps, nothing)
    share = esc[0] / (steps * B)
    n_dev = torch.zeros(1, dtype=torch.int32, device=dev)

    def fused(i):
        dec.adaptive_async_device(llr[i % nbuf].data_ptr(), B, **ptr[i & 1], d_n_escalated=n_dev.data_ptr())

    for i in range(warmup):
        fused(i)
    ref_ms, async_ms, async_pipe_ms = [t_staged], [], []
    for r in range(reps):
        if r:
            ref_ms.append(timed(torch, dev, staged, steps, nothing))
        async_ms.append(timed(torch, dev, fused, steps, nothing))
    dec.set_pipelined(True)
    for i in range(warmup):
        fused(i)
    dec.join()
    for r in range(reps):
        async_pipe_ms.append(timed(torch, dev, fused, steps, dec.join))
    dec.set_pipelined(False)
    waits = dec.adaptive_stats()["host_waits"]
    sc(0)
    t_ahead = timed(torch, dev, staged_ahead, steps, nothing)
    for i in range(warmup):
        two_handles(i)
    torch.cuda.synchronize(dev)
    sc(0)
    t_two = timed(torch, dev, two_handles, steps, join_side)
    dec.set_pipelined(True)
    for i in range(warmup):
        plain(i)
    dec.join()
    t_plain = timed(torch, dev, plain, steps, dec.join)
    dec.set_pipelined(False)
    dec.sync()
    del llr, out
    for d in decs:
        d.close()
    torch.cuda.empty_cache()
    floor_ms = B * N * 8 / HBM_BPS * 1e3
    return {
        "code": f"({N},{K})", "set": "polarization weight" if kind == "pw" else "constructed", "L": L, "ebno_db": ebno,
        "frames_per_step": B, "steps": steps, "escalated_share": share, "t_sc_ms": sc_ms / steps,
        "sc_fps": B / (sc_ms / steps) * 1e3, "sc_hbm_floor_ms": floor_ms, "sc_over_floor": sc_ms / steps / floor_ms,
        "staged_ms": t_staged, "staged_fps": B / t_staged * 1e3, "staged_ahead_ms": t_ahead,
        "staged_ahead_fps": B / t_ahead * 1e3, "two_handles_ms": t_two, "two_handles_fps": B / t_two * 1e3,
        "plain_pipelined_ms": t_plain, "plain_pipelined_fps": B / t_plain * 1e3,
        "build_hash": _native.build_hash(),
        "staged_ref_ms": ref_ms, "async_ms": async_ms, "async_pipelined_ms": async_pipe_ms,
        "async_fps": B / min(async_ms) * 1e3, "async_pipelined_fps": B / min(async_pipe_ms) * 1e3, "async_host_waits": waits,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bytes", type=float, default=2.0 ** 30, help="row bytes per step")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--only", type=int, default=0, help="only the rows of this code length")
    ap.add_argument("--reps", type=int, default=3, help="timed repeats of the staged reference and the async call")
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    points = [("pw", 256, 128, 2.5), ("pw", 512, 256, 2.5), ("pw", 1024, 512, 2.0), ("pw", 1024, 512, 2.5),
              ("constructed", 256, 128, 4.0), ("constructed", 1024, 512, 6.0)]
    rows = []
    stream = torch.cuda.Stream(dev)  # (a stream of its own: the events bracket exactly the handle's work)
    with torch.cuda.stream(stream):
        for kind, N, K, ebno in points:
            if args.only and N != args.only:
                continue
            B = max(1024, int(args.bytes // (N * 8)))
            r = run_point(torch, dev, kind, N, K, 8, ebno, B, max(args.steps, 1), args.warmup, args.seed, max(args.reps, 1))
            rows.append(r)
            print(json.dumps(r), flush=True)
    print()
    print("| code | set | dB | escalated | t_sc ms | floor ms | t_sc/floor | SC Mf/s | staged Mf/s | staged ahead Mf/s | "
          "two handles Mf/s | plain pipelined Mf/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['code']} L={r['L']} | {r['set']} | {r['ebno_db']:.1f} | {100 * r['escalated_share']:.2f} % | "
              f"{r['t_sc_ms']:.3f} | {r['sc_hbm_floor_ms']:.3f} | {r['sc_over_floor']:.1f} | {r['sc_fps'] / 1e6:.1f} | "
              f"{r['staged_fps'] / 1e6:.1f} | {r['staged_ahead_fps'] / 1e6:.1f} | {r['two_handles_fps'] / 1e6:.1f} | "
              f"{r['plain_pipelined_fps'] / 1e6:.1f} |")
    print()
    print("| code | set | dB | staged ms (min .. max of the repeats) | async ms | async pipelined ms | async Mf/s | "
          "async pipelined Mf/s | two handles Mf/s | host waits |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['code']} L={r['L']} | {r['set']} | {r['ebno_db']:.1f} | {min(r['staged_ref_ms']):.3f} .. "
              f"{max(r['staged_ref_ms']):.3f} | {min(r['async_ms']):.3f} .. {max(r['async_ms']):.3f} | "
              f"{min(r['async_pipelined_ms']):.3f} .. {max(r['async_pipelined_ms']):.3f} | {r['async_fps'] / 1e6:.1f} | "
              f"{r['async_pipelined_fps'] / 1e6:.1f} | {r['two_handles_fps'] / 1e6:.1f} | {r['async_host_waits']} |")


if __name__ == "__main__":
    main()
