#!/usr/bin/env python3
"""One timed make_dataset run (polar_code_amd/train/make_dataset.py) in Philox mode: the wall time of
generate_samples with --label host (the NumPy loop around batched device decodes) or --label native
(channel_device -> pscl_label_device on device buffers), and the decode-kernel time inside it.

    python tools/bench_label.py --label native --M 8 --snr_db 3.0 --frames 4194304 --batch 65536

A warm-up run of two batches comes first (library load, scratch growth, stream creation).  The
handle's kernel timing (pscl_timing_*) is on during the timed run: every launch_decode -- the
baseline and every forced-bit round -- is one timed launch, in both modes.  The baseline's part is
then measured on its own (one plain decode_device of one batch of the same frames, times the batch
count), so forced = total - baseline.  One JSON line.  tools/bench_label.sh alternates the two modes.
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", choices=["host", "native"], required=True)
    ap.add_argument("--M", type=int, default=8)
    ap.add_argument("--snr_db", type=float, default=3.0)
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    from polar_code_amd import _native, config
    from polar_code_amd.polar.polar import construct_info_set
    from polar_code_amd.train import make_dataset as md

    cfg = config.get_config()
    info = construct_info_set(cfg.N, cfg.K)
    dec = _native.get_decoder(cfg.N, info, a.M, cfg.crc_poly)
    with tempfile.TemporaryDirectory() as tmp:
        def run(frames, tag):
            argv = ["--M", str(a.M), "--snr_db", str(a.snr_db), "--frames", str(frames), "--seed", str(a.seed),
                    "--out", str(Path(tmp) / tag), "--rng", "philox", "--batch", str(a.batch), "--label", a.label]
            t0 = time.perf_counter()
            shard = md.generate_samples(md.build_argparser().parse_args(argv))
            dec.sync()
            return time.perf_counter() - t0, shard

        run(2 * a.batch, "warm")
        dec.timing_enable(True)
        secs, shard = run(a.frames, "timed")
        launches, kernel_ms = dec.timing_read()
        dec.timing_enable(False)
        import numpy as np

        meta = json.loads(str(np.load(shard)["meta"]))
    # the baseline's share: one plain decode of one batch, on the frames the run starts with
    n = min(a.batch, a.frames)
    with _native.DeviceArena(dec) as mem:
        d_llr, d_best, d_flags = mem.alloc(n * cfg.N * 8), mem.alloc(n * dec.W * 8), mem.alloc(n)
        dec.channel_device(a.seed, 0x7FFF0000 + int(round(a.snr_db * 10)), a.snr_db, cfg.K / cfg.N, cfg.K - cfg.crc_bits,
                           0, n, d_llr, 0)
        dec.decode_device(d_llr, n, d_best=d_best, d_flags=d_flags)  # (warm)
        dec.sync()
        dec.timing_enable(True)
        dec.decode_device(d_llr, n, d_best=d_best, d_flags=d_flags)
        _, base_ms = dec.timing_read()
        dec.timing_enable(False)
    batches = (a.frames + a.batch - 1) // a.batch
    base_ms *= a.frames / n
    print(json.dumps({
        "label": a.label, "M": a.M, "snr_db": a.snr_db, "frames": a.frames, "batch": a.batch, "batches": batches,
        "seconds": round(secs, 4), "frames_per_s": round(a.frames / secs, 1),
        "timed_launches": launches, "kernel_ms": round(kernel_ms, 2), "baseline_ms_est": round(base_ms, 2),
        "forced_ms_est": round(kernel_ms - base_ms, 2), "forced_share_of_wall": round((kernel_ms - base_ms) / (secs * 1e3), 4),
        "samples": meta["samples"], "failures": meta["failures"]}))


if __name__ == "__main__":
    main()
