#!/usr/bin/env python3
"""The float32-row calls against their float64 forms on the same frames.

The shape of tools/bench_adaptive.py: B = 10^6 distinct device-resident frames per step from
channel_device, the step's batch rotated over nbuf buffers (no batch is decoded twice in a row from a
warm cache), W warm-up steps and K >= 20 timed steps between two HIP events, the final
synchronisation inside the timed region.  For sc_device, decode_device and adaptive_async_device, on
a plain and on a pipelined handle, three variants alternate in one run, --reps times each:

  f64      the float64 call on float64 rows.  Its code is the parent's: this is the reference, and
           its min .. max spread over the repeats is the noise margin
  f32      the float32 call on the same rows rounded to float32
  widen    llr32.double() followed by the float64 call: what a float32 caller paid before.  On the
           pipelined handle the temporary is dropped after each step without a join, so a side
           stream may still be reading a block the next step's widening reuses (torch keeps the
           memory; the outputs of these timed steps are not read).  A correct caller joins first or
           holds two copies: the pipelined widen figures are a lower bound of what it pays

and the SC stage's step (sc_device is the SC kernel and nothing else) is set against its HBM floor,
row bytes per frame at 6.29 TB/s, for either row type.

One JSON line per point, then tables.  python tools/bench_f32.py [--frames N] [--steps K] [--calls sc,decode,adaptive]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

POLY = "0x1864CFB"
HBM_BPS = 6.29e12
CALLS = ("sc", "decode", "adaptive")


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


def run_point(torch, dev, N, K, L, E, ebno, B, steps, warmup, seed, reps, calls, nbuf_max):
    from polar_code_amd import _native
    from polar_code_amd.polar.polar import construct_info_set

    info = construct_info_set(N, K)
    dec = _native.Decoder(N, info, L, POLY)
    if E:
        dec.set_rate_match(E)
    if not dec.f32_available():
        raise SystemExit(f"({N},{K}) L={L} E={E}: no float32 kernels on this handle")
    dec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    n_in, W, kp = E or N, dec.W, K - 24
    rate = kp / E if E else K / N
    nbuf = max(1, min(steps, nbuf_max))
    llr = [torch.empty((B, n_in), dtype=torch.float64, device=dev) for _ in range(nbuf)]
    for i in range(nbuf):
        dec.channel_device(seed, int(round(ebno * 10)), ebno, rate, kp, i * B, B, llr[i].data_ptr(), 0)
    llr32 = [x.float() for x in llr]
    best = [torch.empty((B, W), dtype=torch.int64, device=dev) for _ in range(2)]
    flags = [torch.empty((B,), dtype=torch.uint8, device=dev) for _ in range(2)]
    stage = [torch.empty((B,), dtype=torch.uint8, device=dev) for _ in range(2)]
    n_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)

    def out(i):
        return dict(d_best=best[i & 1].data_ptr(), d_flags=flags[i & 1].data_ptr())

    f64 = {"sc": lambda p, i: dec.sc_device(p, B, d_stage=stage[i & 1].data_ptr(), **out(i)),
           "decode": lambda p, i: dec.decode_device(p, B, **out(i)),
           "adaptive": lambda p, i: dec.adaptive_async_device(p, B, d_stage=stage[i & 1].data_ptr(), d_n_escalated=n_dev.data_ptr(),
                                                              **out(i))}
    f32 = {"sc": lambda p, i: dec.sc_device_f32(p, B, d_stage=stage[i & 1].data_ptr(), **out(i)),
           "decode": lambda p, i: dec.decode_device_f32(p, B, **out(i)),
           "adaptive": lambda p, i: dec.adaptive_async_device_f32(p, B, d_stage=stage[i & 1].data_ptr(),
                                                                  d_n_escalated=n_dev.data_ptr(), **out(i))}

    def variants(call):
        def widen(i):
            wide = llr32[i % nbuf].double()  # (the pass a float32 caller ran before: 512 B read, 1,024 B written per frame)
            f64[call](wide.data_ptr(), i)

        return {"f64": lambda i: f64[call](llr[i % nbuf].data_ptr(), i),
                "f32": lambda i: f32[call](llr32[i % nbuf].data_ptr(), i),
                "widen": widen}

    res = {}
    for call in calls:
        for pipe in (False, True):
            v = variants(call)
            if pipe:
                dec.set_pipelined(True)
            tail = dec.join if pipe else (lambda: None)
            for fn in v.values():
                for i in range(warmup):
                    fn(i)
            tail()
            ms = {k: [] for k in v}
            for _ in range(reps):  # the three variants alternate
                for k, fn in v.items():
                    ms[k].append(timed(torch, dev, fn, steps, tail))
            if pipe:
                dec.set_pipelined(False)
            res[call + ("_pipelined" if pipe else "")] = ms
    # the two row types gave the same outputs (on the last batch decoded, through the adaptive call)
    same = None
    if "adaptive" in calls:
        wide = llr32[0].double()
        f32["adaptive"](llr32[0].data_ptr(), 0)  # (output set 0: the float32 call ...)
        f64["adaptive"](wide.data_ptr(), 1)      # (... set 1: the float64 call on the same rows widened)
        dec.sync()
        same = bool(torch.equal(best[0], best[1]) and torch.equal(flags[0], flags[1]) and torch.equal(stage[0], stage[1]))
    dec.sync()
    del llr, llr32, best, flags, stage
    dec.close()
    torch.cuda.empty_cache()
    return {"code": f"({N},{K})" + (f" E={E}" if E else ""), "L": L, "ebno_db": ebno, "frames_per_step": B, "steps": steps,
            "nbuf": nbuf, "ms": res, "sc_floor_f64_ms": B * n_in * 8 / HBM_BPS * 1e3, "sc_floor_f32_ms": B * n_in * 4 / HBM_BPS * 1e3,
            "f32_equals_f64_on_widened_rows": same, "build_hash": _native.build_hash()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nbuf", type=int, default=8, help="batches the steps rotate over (1 GB each at float64, 10^6 frames)")
    ap.add_argument("--calls", type=str, default=",".join(CALLS))
    ap.add_argument("--points", type=str, default="", help="subset, e.g. 8:5.0,4:6.0,nr (L:dB of the (128,64) code; nr)")
    args = ap.parse_args()
    calls = [c for c in args.calls.split(",") if c]
    assert all(c in CALLS for c in calls), calls
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    points = [(128, 64, L, 0, db) for L in (8, 4) for db in (4.0, 5.0, 6.0)] + [(128, 88, 8, 256, 5.0)]
    if args.points:
        want = set(args.points.split(","))
        points = [p for p in points if ("nr" if p[3] else f"{p[2]}:{p[4]}") in want]
    rows = []
    stream = torch.cuda.Stream(dev)  # (the handle runs on it and the events bracket exactly its work)
    with torch.cuda.stream(stream):
        for N, K, L, E, ebno in points:
            r = run_point(torch, dev, N, K, L, E, ebno, args.frames, max(args.steps, 1), args.warmup, args.seed,
                          max(args.reps, 1), calls, args.nbuf)
            rows.append(r)
            print(json.dumps(r), flush=True)

    def span(v):
        return f"{min(v):.3f} .. {max(v):.3f}"

    print()
    print("| code | dB | call | f64 ms (min .. max) | f32 ms | widen + f64 ms | f32 / f64 | f32 / widen | verdict |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        for call, ms in r["ms"].items():
            a, b, c = ms["f64"], ms["f32"], ms["widen"]
            verdict = ("within f64's spread" if min(a) <= min(b) <= max(a) else "below f64" if min(b) < min(a)
                       else "SLOWER than f64 beyond its spread")
            print(f"| {r['code']} L={r['L']} | {r['ebno_db']:.1f} | {call} | {span(a)} | {span(b)} | {span(c)} | "
                  f"{min(b) / min(a):.3f} | {min(b) / min(c):.3f} | {verdict} |")
    if "sc" in calls:
        print()
        print("| code | dB | t_sc f64 ms | f64 floor ms | t_sc / floor | t_sc f32 ms | f32 floor ms | t_sc / floor |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            a, b = min(r["ms"]["sc"]["f64"]), min(r["ms"]["sc"]["f32"])
            print(f"| {r['code']} L={r['L']} | {r['ebno_db']:.1f} | {a:.3f} | {r['sc_floor_f64_ms']:.3f} | {a / r['sc_floor_f64_ms']:.2f} | "
                  f"{b:.3f} | {r['sc_floor_f32_ms']:.3f} | {b / r['sc_floor_f32_ms']:.2f} |")
    bad = [r for r in rows if r["f32_equals_f64_on_widened_rows"] is False]
    if bad:
        raise SystemExit("float32 outputs differ from the float64 call's on the widened rows")


if __name__ == "__main__":
    main()
