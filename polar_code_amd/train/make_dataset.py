"""Flip-label dataset for beta training (mirror of dl_scl_polar/train/make_dataset.py:24-141).

    python -m polar_code_amd.train.make_dataset --M 8 --snr_db 5.0 --frames 1000000 --out data/ds

Same CLI, same shard (``{out}_part0.npz``: ``abs_l0`` float32[S, K], ``flip_idx`` int32[S],
``meta`` JSON) and, in the default replay mode, the same samples as the reference:

* all-zero payload, CRC attached, encoded, BPSK; noise from ``default_rng(seed)`` drawn in the
  reference's order (one N-vector per frame), ``llr = 2 (x + n) / sigma^2``;
* baseline SCL on the GPU for a whole batch; frames whose best candidate passes the CRC are
  skipped (:63-64);
* for the failing frames: ``|L0|`` = the best path's decision LLRs cast to float32 (:66),
  their ``np.argsort`` order (:71), and up to min(8, K) flips tried in that order, each
  forcing the *baseline* best bits' prefix (:74-82, not chained like decode_with_retries).
  All failing frames of a batch are re-decoded together, one GPU batch per flip rank; a frame
  is labelled by the first flip whose result passes the CRC and equals the sent message
  (:86-88); frames without such a flip count as failures.

``--rng philox`` generates the frames on the GPU (counter-based, independent of batching)
and maps them to the all-zero codeword by the channel's symmetry (LLR sign flip where the
sent bit is 1: same noise law), for datasets far larger than the NumPy stream makes sense for.

``--label native`` (default ``host``, the loop above) labels a batch in one native call
(``pscl_label_device``; ``pscl_label_cpu`` with ``--device cpu``): baseline, replay, order, forced
retries and labels without a host trip per round, same shards.  With ``--rng philox`` the frames
stay on the device and are labelled by their own messages (no symmetry mapping; only the failing
frames' ``|L0|`` rows and labels are downloaded).  Equal ``|L0|`` values resolve to the lower index
there, where ``np.argsort``'s order on ties depends on the NumPy build.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import List, Optional

import numpy as np

from .. import _native, config
from ..polar.crc import attach_crc
from ..polar.polar import construct_info_set, encode
from ..utils.seeding import seed_all


def decode_batch(llr: np.ndarray, info_set, M: int, crc, forced: Optional[np.ndarray] = None, device=0):
    """(best bits [B, K] int8, CRC pass [B] bool) of decode_scl for a batch (GPU `device`, or "cpu":
    the host decoder)."""
    dec = _native.get_decoder(llr.shape[1], info_set, M, crc, device)
    out = dec.decode(llr, forced, want_metrics=False, want_cands=False, want_info_llrs=False)
    return out["best_bits"], out["crc_pass"]


def best_path_llrs(llr: np.ndarray, info_set, M: int, crc, bits: np.ndarray, device=0) -> np.ndarray:
    """best_path_info_llrs [B, K] of the paths with information bits `bits`: the decision-LLR replay
    of the decoder in use (GPU `device`, or "cpu": the host decoder's), any N the decoders take."""
    return _native.get_decoder(llr.shape[1], info_set, M, crc, device).path_llrs(llr, bits)


def _force_prefix_flip(bits: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """Rows of flip.py:30-34: bits[:i] forced, bit i flipped, the rest free (-1)."""
    B, K = bits.shape
    col = np.arange(K)[None, :]
    i = idx[:, None]
    forced = np.where(col < i, bits, np.int8(-1)).astype(np.int8)
    forced[np.arange(B), idx] = 1 - bits[np.arange(B), idx]
    return forced


def label_batch(llr: np.ndarray, info_set, M: int, crc: str, sent: np.ndarray, device=0):
    """Samples of one batch, in frame order: (abs_l0 float32 [S, K], labels int32 [S], failures).
    sent: the one sent message [K], or each frame's own [B, K]."""
    sent = np.asarray(sent)
    on = {} if device == 0 else {"device": device}  # (the default device: the helpers' own)
    bits, ok = decode_batch(llr, info_set, M, crc, **on)
    fail = np.flatnonzero(~ok)
    K = bits.shape[1]
    if fail.size == 0:
        return np.zeros((0, K), np.float32), np.zeros(0, np.int32), 0
    base = bits[fail]
    l0 = best_path_llrs(llr[fail], info_set, M, crc, base, **on)
    abs_l0 = np.abs(np.asarray(l0, dtype=np.float32))
    order = np.stack([np.argsort(row) for row in abs_l0])  # per frame, as make_dataset.py:71
    label = np.full(fail.size, -1, np.int32)
    for t in range(min(8, K)):
        todo = np.flatnonzero(label < 0)
        if todo.size == 0:
            break
        idx = order[todo, t]
        cand, cpass = decode_batch(llr[fail[todo]], info_set, M, crc, _force_prefix_flip(base[todo], idx), **on)
        want = sent[None, :] if sent.ndim == 1 else sent[fail[todo]]
        hit = cpass & np.all(cand == want, axis=1)
        label[todo[hit]] = idx[hit]
    keep = label >= 0
    return abs_l0[keep], label[keep], int(np.count_nonzero(~keep))


def label_batch_native(llr: np.ndarray, info_set, M: int, crc: str, sent: np.ndarray, device=0):
    """label_batch as one native call (--label native): pscl_label_device on GPU `device`, or
    pscl_label_cpu with device "cpu".  Same return value; on ties of |L0| the order is the engine's
    (the lower index first), where np.argsort's depends on the NumPy build."""
    out = _native.get_decoder(llr.shape[1], info_set, M, crc, device).label(llr, sent, max_flips=8)
    keep = out["flip"] >= 0
    return out["abs_l0"][keep], out["flip"][keep], int(out["counts"][_native.LBL_UNREPAIRED])


def _philox_label_native(seed: int, snr_db: float, frame0: int, n: int, info_set, M: int, crc: str, kp: int, device=0):
    """n frames from the device TX chain, labelled where they lie: channel_device, then label_device
    on its rows with the frames' own message words as the sent words -- no symmetry mapping, and only
    the entries' rows (the failing frames' |L0| and labels) are downloaded.  Returns label_batch's tuple."""
    cfg = config.get_config()
    dec = _native.get_decoder(cfg.N, info_set, M, crc, device)
    W, K = dec.W, dec.K
    with _native.DeviceArena(dec) as mem:
        d_llr = mem.alloc(n * cfg.N * 8)
        d_msg = mem.alloc(n * W * 8)
        d_counts = mem.alloc(_native.PSCL_NLABEL * 8)
        dec.channel_device(seed, 0x7FFF0000 + int(round(snr_db * 10)), snr_db, cfg.K / cfg.N, kp, frame0, n, d_llr, d_msg)
        cap = _native.label_capacity(n, K)
        for _ in range(2):
            d_frame, d_abs, d_flip = mem.alloc(cap * 8), mem.alloc(cap * K * 4), mem.alloc(cap * 4)
            try:
                A = dec.label_device(d_llr, n, d_msg, W, 8, cap, d_frame=d_frame, d_abs_l0=d_abs, d_flip=d_flip,
                                     d_counts=d_counts)
                break
            except _native.LabelCapacity as e:
                if cap >= e.entries:
                    raise
                cap = e.entries
        dec.sync()
        counts = mem.download(d_counts, _native.PSCL_NLABEL * 8, np.int64)
        frame = mem.download(d_frame, cap * 8, np.int64)[:A]
        abs_l0 = mem.download(d_abs, cap * K * 4, np.float32)[:A * K].reshape(A, K)
        flip = mem.download(d_flip, cap * 4, np.int32)[:A]
    o = np.argsort(frame, kind="stable")
    abs_l0, flip = abs_l0[o], flip[o]
    keep = flip >= 0
    return abs_l0[keep], flip[keep], int(counts[_native.LBL_UNREPAIRED])


def _philox_frames(seed: int, snr_db: float, frame0: int, n: int, info_set, M: int, crc: str, kp: int):
    """n frames from the device TX chain, mapped to the all-zero codeword."""
    cfg = config.get_config()
    dec = _native.get_decoder(cfg.N, info_set, M, crc)
    W = dec.W
    with _native.DeviceArena(dec) as mem:
        d_llr = mem.alloc(n * cfg.N * 8)
        d_msg = mem.alloc(n * W * 8)
        dec.channel_device(seed, 0x7FFF0000 + int(round(snr_db * 10)), snr_db, cfg.K / cfg.N, kp, frame0, n, d_llr,
                           d_msg)
        llr = mem.download(d_llr, n * cfg.N * 8, np.float64).reshape(n, cfg.N)
        words = mem.download(d_msg, n * W * 8, np.uint64).reshape(n, W)
    msg = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(n, -1)[:, :cfg.K]
    x = encode(msg.astype(np.int8))
    return llr * (1.0 - 2.0 * x)


def generate_samples(args: argparse.Namespace) -> Path:
    cfg = config.get_config()
    seed_all(args.seed)
    info_set = construct_info_set(cfg.N, cfg.K)
    payload_bits = cfg.K - cfg.crc_bits
    sent = attach_crc(np.zeros(payload_bits, dtype=np.int8), cfg.crc_poly)
    symbols = 1.0 - 2.0 * encode(sent)
    rate = cfg.K / cfg.N
    noise_var = 1.0 / (2.0 * rate * 10 ** (args.snr_db / 10.0))
    sigma = np.sqrt(noise_var)
    rng = np.random.default_rng(args.seed)

    xs: List[np.ndarray] = []
    ys: List[np.ndarray] = []
    failures = 0
    dev = getattr(args, "device", "0")
    dev = "cpu" if dev == "cpu" else int(dev)
    native = getattr(args, "label", "host") == "native"
    if native and args.rng == "philox" and dev == "cpu":
        raise ValueError("--rng philox generates frames on the GPU: use a GPU --device")
    for b0 in range(0, args.frames, args.batch):
        n = min(args.batch, args.frames - b0)
        if native and args.rng == "philox":  # generated and labelled on the device, by the frames' own messages
            a, lab, nf = _philox_label_native(args.seed, args.snr_db, b0, n, info_set, args.M, cfg.crc_poly, payload_bits, dev)
            xs.append(a)
            ys.append(lab)
            failures += nf
            continue
        if args.rng == "replay":
            noise = rng.normal(0.0, sigma, size=(n, cfg.N))  # = n successive size-N draws
            llr = 2.0 * (symbols[None, :] + noise) / noise_var
        else:
            llr = _philox_frames(args.seed, args.snr_db, b0, n, info_set, args.M, cfg.crc_poly, payload_bits)
        a, lab, nf = (label_batch_native if native else label_batch)(llr, info_set, args.M, cfg.crc_poly, sent, dev)
        xs.append(a)
        ys.append(lab)
        failures += nf
    abs_array = np.concatenate(xs).astype(np.float32)
    label_array = np.concatenate(ys).astype(np.int32)
    if label_array.size == 0:
        raise RuntimeError("No samples collected; consider increasing frames or SNR")
    meta = {"M": args.M, "EbN0_dB": args.snr_db, "seed": args.seed, "frames": args.frames,
            "crc_poly": cfg.crc_poly, "crc_bits": cfg.crc_bits, "samples": int(label_array.size),
            "failures": int(failures)}
    out = Path(args.out)
    out_dir = out.parent if out.parent != Path("") else Path(".")
    out_dir.mkdir(parents=True, exist_ok=True)
    shard = out_dir / f"{out.name}_part0.npz"
    np.savez_compressed(shard, abs_l0=abs_array, flip_idx=label_array, meta=json.dumps(meta))
    print(f"Saved {label_array.size} samples to {shard}")
    return shard


def build_argparser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Generate DL-SCL flip dataset")
    p.add_argument("--M", type=int, required=True, help="SCL list size")
    p.add_argument("--snr_db", type=float, default=5.0, help="AWGN Eb/N0 in dB")
    p.add_argument("--frames", type=int, default=100000, help="Number of frames to simulate")
    p.add_argument("--seed", type=int, default=0, help="RNG seed")
    p.add_argument("--out", type=str, required=True, help="Output prefix for dataset shards")
    # engine options (not in the reference)
    p.add_argument("--rng", choices=["replay", "philox"], default="replay",
                   help="replay: the reference's NumPy stream (identical samples); philox: GPU-generated frames")
    p.add_argument("--batch", type=int, default=1 << 16, help="frames per GPU batch")
    p.add_argument("--device", type=str, default="0", help="GPU index, or cpu: the host decoder and its replay")
    p.add_argument("--label", choices=["host", "native"], default="host",
                   help="host: the NumPy loop around batched decodes; native: one labelling call per batch "
                        "(pscl_label_device, or pscl_label_cpu with --device cpu)")
    return p


def main(argv: list[str] | None = None) -> None:
    generate_samples(build_argparser().parse_args(argv))


if __name__ == "__main__":
    main()
