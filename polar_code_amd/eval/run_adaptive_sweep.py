"""FER sweep with adaptive decoding: the SC baseline curve and the adaptive curve (SC first, the
list decoder only where SC fails the CRC) from the device Monte-Carlo loop.

    python -m polar_code_amd.eval.run_adaptive_sweep --M 8 --frames 1000000 --snr_lo 4 --snr_hi 6 \
        --snr_step 0.5 --seed 0 --include_uncoded

Frames are generated on the GPU by the Philox stream run_fer_sweep --rng philox uses (keyed by
seed, SNR and global frame index), so results do not depend on the GPU count.  Every SNR point is
enqueued with pscl_simulate_adaptive_device -- no host wait anywhere -- and the counters of the
whole sweep are read once at the end.  Multi-GPU: launch with torchrun; frames are sharded by
global index and the counters summed with one all-reduce (polar_code_amd/dist.py).
Output: fer_adaptive_M{M}.csv with columns
    snr_db,[fer_uncoded,ber_uncoded,]fer_sc,ber_sc,fer_adaptive,ber_adaptive,escalated
FER is the share of frames whose result fails the CRC (PSCL_CNT_FRAME_ERR / frames, as
run_fer_sweep), escalated the share of frames handed to the list decoder.

--retries R (R > 0, optionally --beta PATH) adds the third stage: DL-SCL flip retries for the frames
the list decoder fails too (pscl_simulate_adaptive_dl_device, the retry chains deferred on a
pipelined handle).  The CSV then gains fer_dl,ber_dl,avg_retries after escalated (avg_retries =
flip re-decodes / frames, as run_fer_sweep).  With R = 0 the sweep and its file are unchanged.
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Dict, List

import numpy as np

from .. import _native, config, dist
from ..polar.polar import construct_info_set
from ..utils.seeding import philox_stream_id, seed_all


def csv_header(include_uncoded: bool, retries: int = 0) -> List[str]:
    head = ["snr_db"]
    if include_uncoded:
        head += ["fer_uncoded", "ber_uncoded"]
    head += ["fer_sc", "ber_sc", "fer_adaptive", "ber_adaptive", "escalated"]
    return head + (["fer_dl", "ber_dl", "avg_retries"] if retries > 0 else [])


def snr_points(args: argparse.Namespace) -> np.ndarray:
    return (np.arange(args.snr_lo, args.snr_hi + 1e-9, args.snr_step) if args.snr_step > 0
            else np.array([args.snr_lo]))


def row_from_counters(snr_db: float, cnt: np.ndarray, frames: int, K: int, payload_bits: int,
                      include_uncoded: bool, retries: int = 0) -> Dict[str, float]:
    """One CSV row from the summed counters [3, PSCL_NCOUNT] (rows SC, adaptive, uncoded), or with
    retries > 0 [4, PSCL_NCOUNT] (rows SC, adaptive, final, uncoded)."""
    sc, ad, un = (cnt[0], cnt[1], cnt[3]) if retries > 0 else cnt
    nan = float("nan")
    row = {"snr_db": float(snr_db),
           "fer_sc": sc[_native.CNT_FRAME_ERR] / frames if frames else nan,
           "ber_sc": sc[_native.CNT_BIT_ERR] / (frames * K) if frames else nan,
           "fer_adaptive": ad[_native.CNT_FRAME_ERR] / frames if frames else nan,
           "ber_adaptive": ad[_native.CNT_BIT_ERR] / (frames * K) if frames else nan,
           "escalated": ad[_native.CNT_ESCALATED] / frames if frames else nan}
    if retries > 0:
        dl = cnt[2]
        row["fer_dl"] = dl[_native.CNT_FRAME_ERR] / frames if frames else nan
        row["ber_dl"] = dl[_native.CNT_BIT_ERR] / (frames * K) if frames else nan
        row["avg_retries"] = dl[_native.CNT_RETRIES] / max(frames, 1)
    if include_uncoded:
        row["fer_uncoded"] = un[_native.CNT_FRAME_ERR] / frames if frames else nan
        row["ber_uncoded"] = un[_native.CNT_BIT_ERR] / (frames * payload_bits) if frames else nan
    return row


def sweep_counters(args: argparse.Namespace, points, info_set, device: int, payload_bits: int, start: int,
                   stop: int) -> np.ndarray:
    """This rank's frames [start, stop) of every point, enqueued at once: int64 [points, 3, PSCL_NCOUNT]
    (with --retries: [points, 4, PSCL_NCOUNT])."""
    cfg = config.get_config()
    dec = _native.get_decoder(cfg.N, info_set, args.M, cfg.crc_poly, device)
    nc = _native.PSCL_NCOUNT
    batch = args.batch or (1 << 20)
    retries = getattr(args, "retries", 0)
    rows = 4 if retries > 0 else 3
    if retries > 0:
        dec.set_beta(np.load(args.beta) if getattr(args, "beta", None) else None)
    with _native.DeviceArena(dec) as mem:
        nbytes = len(points) * rows * nc * 8
        d_cnt = mem.alloc(nbytes)
        mem.memset(d_cnt, 0, nbytes)
        for i, snr_db in enumerate(points):
            for b0 in range(start, stop, batch):
                if retries > 0:
                    dec.simulate_adaptive_dl_device(args.seed, philox_stream_id(float(snr_db)), float(snr_db),
                                                    cfg.K / cfg.N, payload_bits, b0, min(stop, b0 + batch) - b0, retries,
                                                    args.include_uncoded, d_cnt + i * rows * nc * 8)
                else:
                    dec.simulate_adaptive_device(args.seed, philox_stream_id(float(snr_db)), float(snr_db), cfg.K / cfg.N,
                                                 payload_bits, b0, min(stop, b0 + batch) - b0, args.include_uncoded,
                                                 d_cnt + i * 3 * nc * 8)
        dec.join()
        return mem.download(d_cnt, nbytes, np.int64).reshape(len(points), rows, nc)  # (the one host wait)


def write_csv(results: List[Dict[str, float]], args: argparse.Namespace) -> Path:
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    path = out / f"fer_adaptive_M{args.M}.csv"
    head = csv_header(args.include_uncoded, getattr(args, "retries", 0))
    with path.open("w") as f:
        f.write(",".join(head) + "\n")
        for row in results:
            f.write(",".join(f"{row[k]:.3f}" if k == "snr_db" else f"{row[k]:.6e}" for k in head) + "\n")
    return path


def run_sweep(args: argparse.Namespace) -> List[Dict[str, float]]:
    cfg = config.get_config()
    seed_all(args.seed)
    ctx = dist.init()
    info_set = construct_info_set(cfg.N, cfg.K)
    payload_bits = cfg.K - cfg.crc_bits
    points = snr_points(args)
    start, stop = dist.shard(args.frames, ctx.rank, ctx.world)
    cnt = sweep_counters(args, points, info_set, ctx.device, payload_bits, start, stop)
    cnt = dist.allreduce_sum(cnt.reshape(-1), ctx).reshape(cnt.shape)
    results = [row_from_counters(float(s), cnt[i], args.frames, cfg.K, payload_bits, args.include_uncoded, args.retries)
               for i, s in enumerate(points)]
    if ctx.is_root:
        for row in results:
            print(f"SNR={row['snr_db']:.2f} dB -> SC FER={row['fer_sc']:.3e}, BER={row['ber_sc']:.3e}; "
                  f"adaptive FER={row['fer_adaptive']:.3e}, BER={row['ber_adaptive']:.3e}; "
                  f"escalated {row['escalated']:.3e}"
                  + (f"; DL FER={row['fer_dl']:.3e}, BER={row['ber_dl']:.3e}, avg retries {row['avg_retries']:.3e}"
                     if args.retries > 0 else ""), flush=True)
        print(f"Saved FER table to {write_csv(results, args)}")
    return results


def build_argparser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="FER sweep with adaptive (SC-then-list) decoding")
    parser.add_argument("--M", type=int, required=True, help="List size of the escalation")
    parser.add_argument("--frames", type=int, default=10000, help="Frames per SNR point")
    parser.add_argument("--snr_lo", type=float, default=4.0)
    parser.add_argument("--snr_hi", type=float, default=6.5)
    parser.add_argument("--snr_step", type=float, default=0.5)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--include_uncoded", action="store_true", help="Also simulate an uncoded BPSK baseline")
    parser.add_argument("--batch", type=int, default=None, help="frames per call (default 2^20)")
    parser.add_argument("--retries", type=int, default=0,
                        help="DL-SCL flip retries for the frames the list decoder fails (0: adaptive decoding only)")
    parser.add_argument("--beta", type=str, default=None, help="Path to trained beta matrix (.npy), used with --retries")
    parser.add_argument("--out_dir", type=str, default="results")
    return parser


def main(argv: List[str] | None = None) -> None:
    args = build_argparser().parse_args(argv)
    run_sweep(args)
    dist.finalize()


if __name__ == "__main__":
    main()
