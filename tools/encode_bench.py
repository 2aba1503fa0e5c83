"""Timing of the caller-payload TX (csrc/encode.hip) against the TX it stands beside.

  python tools/encode_bench.py [--frames 1000000] [--out profiles/encode_bench.txt] [--label TEXT]
  PSCL_LIB_PATH=<another build> python tools/encode_bench.py --only-channel --label parent ...

Per code -- (128,64), and (128,88) rate-matched to E = 256 -- and per call: 3 warm-up steps, then 20
timed steps between two HIP events, repeated 3 times; min .. max of the per-step time in us.
  (a) pscl_channel_device                      (Philox payloads; --only-channel measures it alone, for a
                                                run on the library of another commit beside this one's)
  (b) pscl_channel_payload_device, float64 rows
  (c) the same, float32 rows
  (d) pscl_encode_device, code words only
  (e) pscl_encode_device, float32 symbols only
  (f) the host path they replace: encode_rate_matched / polar.encode per row plus the copy to the
      device, on 10^4 frames, scaled to --frames
(d) and (e) draw no noise; their bytes per frame and the fraction of the 8 TB/s HBM peak are printed.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

POLY = "0x1864CFB"
CODES = [(128, 64, 0), (128, 88, 256)]
WARMUP, STEPS, REPEATS = 3, 20, 3
HBM_PEAK = 8.0e12


def timed(torch, fn):
    """min, max over REPEATS of the mean step time (us) of STEPS calls between two events."""
    out = []
    for _ in range(REPEATS):
        for _ in range(WARMUP):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / STEPS)
    return min(out), max(out)


def measure(frames: int, only_channel: bool) -> dict:
    import torch

    dev = torch.device("cuda", 0)
    # (a stream of its own: the handle runs on the caller's stream only where that is not the null stream)
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        return _measure(frames, only_channel, dev)


def _measure(frames: int, only_channel: bool, dev) -> dict:
    import numpy as np
    import torch

    from polar_code_amd import _native
    from polar_code_amd.nr.polar.scl_nr import encode_rate_matched
    from polar_code_amd.polar.crc import attach_crc
    from polar_code_amd.polar.polar import _polar_transform, construct_info_set

    res = {}
    for N, K, E in CODES:
        info = construct_info_set(N, K)
        dec = _native.Decoder(N, info, 8, POLY)
        if E:
            dec.set_rate_match(E)
        dec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        kp, Et = K - 24, E or N
        rate, B = kp / Et, frames
        r = {}
        rows = torch.empty((B, Et), dtype=torch.float64, device=dev)
        msg = torch.empty((B, dec.W), dtype=torch.int64, device=dev)
        r["a"] = timed(torch, lambda: dec.channel_device(1, 0, 3.0, rate, kp, 0, B, rows.data_ptr(), msg.data_ptr()))
        if not only_channel:
            pay = torch.randint(-2**62, 2**62, (B, dec.payload_words), dtype=torch.int64, device=dev)
            rows32 = torch.empty((B, Et), dtype=torch.float32, device=dev)
            code = torch.empty((B, dec.code_words), dtype=torch.int64, device=dev)
            r["b"] = timed(torch, lambda: dec.channel_payload_device(pay.data_ptr(), 1, 0, 3.0, rate, 0, B,
                                                                     d_llr=rows.data_ptr(), d_msg=msg.data_ptr()))
            r["c"] = timed(torch, lambda: dec.channel_payload_device(pay.data_ptr(), 1, 0, 3.0, rate, 0, B,
                                                                     d_llr=rows32.data_ptr(), llr_f32=True,
                                                                     d_msg=msg.data_ptr()))
            r["d"] = timed(torch, lambda: dec.encode_device(pay.data_ptr(), B, d_code=code.data_ptr()))
            r["e"] = timed(torch, lambda: dec.encode_device(pay.data_ptr(), B, d_sym=rows32.data_ptr(), sym_f32=True))
            r["d_bytes"] = 8 * dec.payload_words + 8 * dec.code_words
            r["e_bytes"] = 8 * dec.payload_words + 4 * Et
            # (f) the host path: one frame at a time, then one copy
            nh = 10_000
            bits = np.random.default_rng(0).integers(0, 2, size=(nh, kp), dtype=np.int8)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if E:
                tx = np.stack([encode_rate_matched(b, POLY, N, E, info) for b in bits])
            else:
                u = np.zeros((nh, N), np.int8)
                for i, b in enumerate(bits):
                    u[i, info] = attach_crc(b, POLY)
                tx = np.stack([_polar_transform(v) for v in u])
            sym = torch.from_numpy((1.0 - 2.0 * tx).astype(np.float32)).to(dev)
            torch.cuda.synchronize()
            r["f"] = (time.perf_counter() - t0) * 1e6 * frames / nh
            del sym
        res[f"{N},{K},{E}"] = r
        dec.close()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--out", default=None, help="append the report to this file")
    ap.add_argument("--only-channel", action="store_true", help="(a) alone: the run on another library")
    ap.add_argument("--label", default="this library")
    a = ap.parse_args()
    from polar_code_amd import _native

    res = measure(a.frames, a.only_channel)
    lines = [f"[{a.label}: {_native.LIB_PATH.name}, build {_native.build_hash() or '?'}] {a.frames} frames per call; "
             f"{WARMUP} warm-up + {STEPS} timed steps between HIP events, min .. max of {REPEATS} repeats, us per call"]
    names = {"a": "pscl_channel_device                     ", "b": "pscl_channel_payload_device float64     ",
             "c": "pscl_channel_payload_device float32     ", "d": "pscl_encode_device, code words only     ",
             "e": "pscl_encode_device, float32 symbols only"}
    for key, r in res.items():
        N, K, E = key.split(",")
        lines.append(f"code ({N},{K}) CRC-24" + (f", rate-matched E = {E}" if E != "0" else ""))
        for k, name in names.items():
            if k not in r:
                continue
            lo, hi = r[k]
            extra = ""
            if k in "de":
                by = r[k + "_bytes"]
                extra = (f"   {by} B/frame, {by * a.frames / (hi * 1e-6) / HBM_PEAK:.3f} .. "
                         f"{by * a.frames / (lo * 1e-6) / HBM_PEAK:.3f} of the 8 TB/s HBM peak")
            lines.append(f"  ({k}) {name} {lo:9.1f} .. {hi:9.1f}{extra}")
        if "f" in r:
            lines.append(f"  (f) host encode per row + copy (10^4 frames, scaled)   {r['f']:12.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
