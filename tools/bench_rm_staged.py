#!/usr/bin/env python3
"""Staged de-rate-matching (pscl_set_rate_match_staged) against the mode-off call on the same
rate-matched rows, and against the rate-matching-free twin on rows de-rate-matched beforehand.

The shape of tools/bench_f32.py: distinct device-resident frames from channel_device, the step's
batch rotated over nbuf buffers, W warm-up steps and K >= 20 timed steps between two HIP events,
the final synchronisation (and, pipelined, the join) inside the timed region.  For decode_device and
adaptive_async_device, on a stream-ordered and on a pipelined handle, three variants alternate in
one run, --reps rounds each:

  a  off    the mode-off call on the [B, E] rows: the parent's path and the yardstick; its min .. max
            over the rounds is the noise margin.  Where the parent refuses the call (the adaptive
            call on a rate-matched handle at N != 128) there is no figure
  b  on     the mode-on call on the same rows: the pass, the twin's kernels on its rows, the exact
            re-decode on the caller's rows
  c  twin   a plain handle of the same code on rows de-rate-matched before the timed region: the
            floor; b - c is what the pass costs in place

and  p  the pass alone (derate_match_device) against a device-to-device copy of B (E + N) 8 bytes
(the bytes the pass reads plus the bytes it writes) in the same run, alternating.

One JSON line per point, then tables.  python tools/bench_rm_staged.py [--points 0,1,..] [--steps K]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

POLY = "0x1864CFB"
# (N, K, set, E, L, dB, frames per step)
POINTS = [(128, 64, "c", 100, 8, 5.0, 1_000_000), (128, 100, "c", 256, 8, 4.5, 1_000_000),
          (256, 128, "pw", 300, 8, 4.0, 200_000), (256, 128, "pw", 300, 16, 4.0, 200_000),
          (1024, 512, "pw", 1100, 8, 6.0, 50_000), (1024, 512, "pw", 1100, 32, 6.0, 50_000)]


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


def run_point(torch, dev, N, K, kind, E, L, ebno, B, steps, warmup, seed, reps, nbuf):
    from polar_code_amd import _native
    from polar_code_amd.polar.polar import construct_info_set

    info = pw_info_set(N, K) if kind == "pw" else construct_info_set(N, K)
    stream = torch.cuda.current_stream(dev).cuda_stream
    dec = {}
    for k in ("off", "on", "twin"):
        dec[k] = _native.Decoder(N, info, L, POLY)
        dec[k].set_stream(stream)
        if k != "twin":
            dec[k].set_rate_match(E)
    dec["on"].set_rate_match_staged(True)
    W, kp = dec["on"].W, K - 24
    nbuf = max(3, min(steps, nbuf))  # (a pipelined call's rows stay in use for two more calls)
    llr = [torch.empty((B, E), dtype=torch.float64, device=dev) for _ in range(nbuf)]
    for i in range(nbuf):
        dec["on"].channel_device(seed, int(round(ebno * 10)), ebno, kp / E, kp, i * B, B, llr[i].data_ptr(), 0)
    plain = [torch.empty((B, N), dtype=torch.float64, device=dev) for _ in range(nbuf)]
    for i in range(nbuf):
        dec["on"].derate_match_device(llr[i].data_ptr(), B, plain[i].data_ptr())
    best = [torch.empty((B, W), dtype=torch.int64, device=dev) for _ in range(2)]
    flags = [torch.empty((B,), dtype=torch.uint8, device=dev) for _ in range(2)]
    stage = [torch.empty((B,), dtype=torch.uint8, device=dev) for _ in range(2)]
    n_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)

    def out(i):
        return dict(d_best=best[i & 1].data_ptr(), d_flags=flags[i & 1].data_ptr())

    def call(name, d, rows):
        if name == "decode":
            return lambda i: d.decode_device(rows[i % nbuf].data_ptr(), B, **out(i))
        return lambda i: d.adaptive_async_device(rows[i % nbuf].data_ptr(), B, d_stage=stage[i & 1].data_ptr(),
                                                 d_n_escalated=n_dev.data_ptr(), **out(i))

    res, refused = {}, {}
    for name in ("decode", "adaptive"):
        for pipe in (False, True):
            v = {"off": call(name, dec["off"], llr), "on": call(name, dec["on"], llr), "twin": call(name, dec["twin"], plain)}
            for d in dec.values():
                d.set_pipelined(pipe)

            def tail():
                for d in dec.values():
                    d.join()

            for k in list(v):
                try:
                    for i in range(warmup):
                        v[k](i)
                except NotImplementedError as e:  # (the parent's refusal: no yardstick for this call)
                    refused[name] = str(e)
                    del v[k]
            tail()
            ms = {k: [] for k in v}
            for _ in range(reps):  # the variants alternate
                for k, fn in v.items():
                    ms[k].append(timed(torch, dev, fn, steps, tail))
            for d in dec.values():
                d.set_pipelined(False)
            res[name + ("_pipelined" if pipe else "")] = ms
    # the pass alone against a copy of the bytes it moves
    nbytes = B * (E + N) * 8
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    src.zero_()
    p = {"pass": lambda i: dec["on"].derate_match_device(llr[i % nbuf].data_ptr(), B, plain[i % nbuf].data_ptr()),
         "copy": lambda i: dst.copy_(src)}
    for fn in p.values():
        for i in range(warmup):
            fn(i)
    pms = {k: [] for k in p}
    for _ in range(reps):
        for k, fn in p.items():
            pms[k].append(timed(torch, dev, fn, steps, lambda: None))
    # mode on, mode off and the twin gave the same outputs (the last batch, through the plain decode)
    outs = []
    for k, rows in (("on", llr), ("off", llr), ("twin", plain)):
        dec[k].decode_device(rows[0].data_ptr(), B, **out(0))
        dec[k].sync()
        outs.append((best[0].clone(), flags[0].clone()))
    same = all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])
    deferred = dec["on"].screening_count()
    stats = dec["on"].rm_staged_stats()
    for d in dec.values():
        d.sync()
        d.close()
    del llr, plain, best, flags, stage, src, dst
    torch.cuda.empty_cache()
    return {"code": f"({N},{K})", "set": "polarization weight" if kind == "pw" else "constructed", "E": E, "L": L,
            "ebno_db": ebno, "frames_per_step": B, "steps": steps, "nbuf": nbuf, "ms": res, "refused": refused,
            "pass_ms": pms, "pass_bytes": nbytes, "outputs_equal": bool(same), "deferred_last_batch": deferred,
            "staged_passes": stats["passes"], "build_hash": _native.build_hash()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nbuf", type=int, default=4, help="batches the steps rotate over")
    ap.add_argument("--frames_scale", type=float, default=1.0, help="scale every point's frames per step (smoke runs)")
    ap.add_argument("--points", type=str, default="", help="indices into the point list, e.g. 0,2")
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    points = [POINTS[int(i)] for i in args.points.split(",")] if args.points else POINTS
    rows = []
    stream = torch.cuda.Stream(dev)  # (the handles run on it and the events bracket exactly their work)
    with torch.cuda.stream(stream):
        for N, K, kind, E, L, ebno, B in points:
            r = run_point(torch, dev, N, K, kind, E, L, ebno, max(64, int(B * args.frames_scale)), max(args.steps, 1),
                          args.warmup, args.seed, max(args.reps, 3), args.nbuf)
            rows.append(r)
            print(json.dumps(r), flush=True)

    def span(v):
        return f"{min(v):.3f} .. {max(v):.3f}" if v else "refused"

    print()
    print("| code | E | L | dB | call | a: off ms (min .. max) | b: on ms | c: twin ms | b / a | b / c | b - c ms | M frames/s on | verdict |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        for name, ms in r["ms"].items():
            a, b, c = ms.get("off", []), ms["on"], ms["twin"]
            if not a:
                verdict = "the parent refuses this call"
            elif max(b) < min(a):
                verdict = "below every off round"
            elif min(b) < min(a):
                verdict = "NOT below every off round (overlapping spreads)"
            else:
                verdict = "NOT below off"
            ba = f"{min(b) / min(a):.3f}" if a else "-"
            print(f"| {r['code']} | {r['E']} | {r['L']} | {r['ebno_db']:.1f} | {name} | {span(a)} | {span(b)} | {span(c)} | {ba} | "
                  f"{min(b) / min(c):.3f} | {min(b) - min(c):.3f} | {r['frames_per_step'] / min(b) / 1e3:.2f} | {verdict} |")
    print()
    print("| code | E | frames | pass ms (min .. max) | copy of B (E + N) 8 bytes ms | pass / copy | pass GB/s (read + written) |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        a, b = r["pass_ms"]["pass"], r["pass_ms"]["copy"]
        print(f"| {r['code']} | {r['E']} | {r['frames_per_step']} | {span(a)} | {span(b)} | {min(a) / min(b):.2f} | "
              f"{r['pass_bytes'] / min(a) / 1e6:.0f} |")
    if any(not r["outputs_equal"] for r in rows):
        raise SystemExit("mode-on, mode-off and twin outputs differ")


if __name__ == "__main__":
    main()
