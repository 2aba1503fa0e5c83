"""GPU: the device FER sweep (pscl_simulate / pscl_simulate_device, run_fer_sweep --rng philox)
held to the oracle (C restatement of the reference, test infrastructure only).

One call of the product path does TX, the uncoded baseline, SCL, DL-SCL and the counting on the
device; on a pipelined handle each block's retry chains run beside the next block's and the next
SNR point's TX and baseline.  Every other test of this path compares HIP with HIP.  Here the rows
of every point are regenerated with pscl_channel_device (itself pinned to a NumPy restatement of
its stream by test_gpu_channel.py), decoded by the oracle (decode_batch for the SCL row, dl_batch
for the DL-SCL row), and every counter of both rows is rebuilt on the host and compared exactly;
the uncoded row is restated on the host from its Philox stream.

Counters compared (include/polar_scl.h, PSCL_CNT_*):
  SCL row      FRAMES, FRAME_ERR, BIT_ERR, PAYLOAD_ERR, PAYLOAD_BIT          exact
  DL-SCL row   the same five and RETRIES = sum(attempts - 1)                 exact
  uncoded row  FRAMES exact; FRAME_ERR, BIT_ERR within n_amb, the number of decisions with
               |y| < 1e-4 (the ones fp32 Box-Muller against libm can flip)
The header leaves undefined, and nothing here asserts: RETRIES of the SCL row (it defines the
counter for d_counters_dl only), PAYLOAD_ERR / PAYLOAD_BIT / RETRIES of the uncoded row
(pscl_uncoded_device adds FRAMES, FRAME_ERR and BIT_ERR only), and slots 6 and 7 of every row.

  2a  run_fer_sweep._philox_sweep_device: 6 points x 3 blocks, partial last blocks, a frame range
      across 2^32, under the default schedule, both TX forms and exact warm starts; L = 8 and 4
  2b  run_fer_sweep.run_sweep: the returned rows and the written CSV
  2c  simulate on N = 256, on (128,88) with and without rate matching, on a punctured (128,64)
  2d  the 2^20-frame chunk boundary of one call (HIP against HIP: "shards add up exactly")
"""
import math
from collections import namedtuple

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from polar_code_amd import _native
from polar_code_amd.dlscl.flip import words_to_bits
from polar_code_amd.eval import run_fer_sweep as rfs
from polar_code_amd.nr.polar import derate_match_polar, subblock_deinterleave
from polar_code_amd.polar.polar import construct_info_set
from polar_code_amd.utils.seeding import philox_stream_id
from test_gpu_baseline_configs import _host_counts, _nr_internal
from test_gpu_channel import M32, host_bm, host_payload, host_stream, philox4x32

pytestmark = pytest.mark.gpu
POLY = "0x1864CFB"
CRC_BITS = 24
FRAMES, FRAME_ERR, BIT_ERR, PAY_ERR, PAY_BIT, RETRIES = 0, 1, 2, 3, 4, 5
SCL_KEYS = (FRAMES, FRAME_ERR, BIT_ERR, PAY_ERR, PAY_BIT)
DL_KEYS = SCL_KEYS + (RETRIES,)
NAMES = {FRAMES: "FRAMES", FRAME_ERR: "FRAME_ERR", BIT_ERR: "BIT_ERR", PAY_ERR: "PAYLOAD_ERR",
         PAY_BIT: "PAYLOAD_BIT", RETRIES: "RETRIES"}

Code = namedtuple("Code", "N K E")  # E = 0: no rate matching
P128 = Code(128, 64, 0)


def _kp(code):
    return code.K - CRC_BITS


def _rate(code):
    """The rate the callers pass: K / N (run_fer_sweep), k_payload / E on a rate-matched handle
    (test_gpu_baseline_configs._batch)."""
    return _kp(code) / code.E if code.E else code.K / code.N


def _host_uncoded(seed, sid, ebno_db, kp, frame0, n):
    """The uncoded row restated as test_gpu_channel.test_uncoded_stream does: the payload of
    host_payload, noise blocks (frame, 0x40000000 + c), sigma^2 = 1 / (2 Eb/N0), decision y < 0.
    Returns frame errors, bit errors, the ambiguous decisions (|y| < 1e-4) and their expectation."""
    k0 = seed & 0xFFFFFFFF
    k1 = ((seed >> 32) ^ ((sid * 0x85EBCA6B) & 0xFFFFFFFF)) & 0xFFFFFFFF
    fr = np.arange(frame0, frame0 + n, dtype=np.uint64)
    lo, hi = fr & M32, fr >> np.uint64(32)
    pay = host_payload(k0, k1, lo, hi, kp)
    sigma = math.sqrt(1.0 / (2.0 * 10 ** (ebno_db / 10.0)))
    err = np.zeros((n, kp), bool)
    n_amb = 0
    for c in range((kp + 1) // 2):
        c2 = np.full(n, 0x40000000 + c, np.uint64)
        cx, cy, cz, cw = philox4x32((lo, hi, c2, np.zeros(n, np.uint64)), k0, k1)
        zz = host_bm((cy << np.uint64(32)) | cx, (cw << np.uint64(32)) | cz)
        for h in range(2):
            q = 2 * c + h
            if q < kp:
                y = (1.0 - 2.0 * pay[:, q]) + sigma * zz[h]
                err[:, q] = (y < 0.0) != (pay[:, q] == 1)
                n_amb += int(np.count_nonzero(np.abs(y) < 1e-4))
    # P(|y| < 1e-4) = 2e-4 * the density of N(+-1, sigma) at 0
    expect = 2e-4 * math.exp(-1.0 / (2.0 * sigma * sigma)) / (sigma * math.sqrt(2.0 * math.pi)) * n * kp
    return {"frame_err": int(err.any(axis=1).sum()), "bit_err": int(err.sum()), "n_amb": n_amb, "expect": expect,
            "payload": pay}


def _internal_rows(llr, code):
    """Received rows -> the decoder's N internal LLRs (scl_nr.py:47-48 front end)."""
    if not code.E:
        return llr
    mirror = lambda r: subblock_deinterleave(derate_match_polar(r, code.N), code.N)
    if code.E == 2 * code.N:
        out = _nr_internal(llr, code.N)
        np.testing.assert_array_equal(out[:200], np.stack([mirror(r) for r in llr[:200]]))
        return out
    return np.stack([mirror(r) for r in llr])


_ORACLE = {}  # (code, L, beta name, retries, seed, (snr, frame0, n)) -> host counters of the point


def _oracle_points(code, L, beta_name, retries, seed, points):
    """Host counters of every point (snr_db, frame0, n): rows [frame0, frame0 + n) regenerated by
    pscl_channel_device, decoded by the oracle, counted on the host; the uncoded row restated.
    Cached per point at module scope: the schedule variants of a case pay for the oracle once."""
    todo = [p for p in points if (code, L, beta_name, retries, seed, p) not in _ORACLE]
    if todo:
        oracle.set_num_threads(16)
        info = construct_info_set(code.N, code.K)
        beta = np.load(GOLDEN / f"beta_{beta_name}.npy") if beta_name else None
        kp, rate, row = _kp(code), _rate(code), code.E or code.N
        tx = _native.Decoder(code.N, info, 2, POLY)  # (the TX chain does not depend on the list size)
        if code.E:
            tx.set_rate_match(code.E)
        W = tx.W
        for snr, frame0, n in todo:
            sid = philox_stream_id(snr)
            with _native.DeviceArena(tx) as mem:
                d_llr, d_msg = mem.alloc(n * row * 8), mem.alloc(n * W * 8)
                tx.channel_device(seed, sid, snr, rate, kp, frame0, n, d_llr, d_msg)
                llr = mem.download(d_llr, n * row * 8, np.float64).reshape(n, row)
                msg = words_to_bits(mem.download(d_msg, n * W * 8, np.uint64).reshape(n, W), code.K)
            llr = _internal_rows(llr, code)
            bits_s, ok_s = oracle.decode_batch(llr, info, L, POLY)
            bits_d, ok_d, att = oracle.dl_batch(llr, info, L, retries, POLY, beta)
            np.testing.assert_array_equal(att > 1, ~ok_s)  # (retried iff the baseline fails)
            scl = _host_counts(bits_s, msg, ok_s, kp)
            dl = _host_counts(bits_d, msg, ok_d, kp)
            dl[RETRIES] = int((att - 1).sum())
            unc = _host_uncoded(seed, sid, snr, kp, frame0, n)
            # (the transmitted payload is the restated one: both words of the frame counter)
            np.testing.assert_array_equal(msg[:, :kp], unc.pop("payload"))
            _ORACLE[(code, L, beta_name, retries, seed, (snr, frame0, n))] = {
                "scl": scl, "dl": dl, "unc": unc, "n": n, "kp": kp}
        tx.close()
    return [_ORACLE[(code, L, beta_name, retries, seed, p)] for p in points]


def _check_point(cnt, host, tag, include_uncoded=True):
    """Device counters [3][PSCL_NCOUNT] of one point against the host's."""
    print(f"{tag}: SCL {host['scl'][FRAME_ERR]}/{host['n']} frames fail "
          f"({100.0 * host['scl'][FRAME_ERR] / host['n']:.2f} %), DL-SCL {host['dl'][FRAME_ERR]}, "
          f"{host['dl'][RETRIES]} retries; uncoded {host['unc']['frame_err']} frames, {host['unc']['bit_err']} bits, "
          f"{host['unc']['n_amb']} ambiguous ({host['unc']['expect']:.2f} expected)")
    for row, name, keys in ((0, "scl", SCL_KEYS), (1, "dl", DL_KEYS)):
        for k in keys:
            assert int(cnt[row][k]) == host[name][k], (
                f"{tag}: {name} {NAMES[k]} device {int(cnt[row][k])} oracle {host[name][k]}")
    if include_uncoded:
        u = host["unc"]
        assert u["n_amb"] < 3 * u["expect"] + 10, f"{tag}: {u['n_amb']} ambiguous decisions, {u['expect']:.2f} expected"
        assert int(cnt[2][FRAMES]) == host["n"], f"{tag}: uncoded FRAMES"
        assert abs(int(cnt[2][FRAME_ERR]) - u["frame_err"]) <= u["n_amb"], (
            f"{tag}: uncoded FRAME_ERR device {int(cnt[2][FRAME_ERR])} host {u['frame_err']} +- {u['n_amb']}")
        assert abs(int(cnt[2][BIT_ERR]) - u["bit_err"]) <= u["n_amb"], (
            f"{tag}: uncoded BIT_ERR device {int(cnt[2][BIT_ERR])} host {u['bit_err']} +- {u['n_amb']}")


@pytest.mark.parametrize("N,K", [(128, 64), (256, 128)])
def test_channel_rows_across_2_32(N, K):
    """The rows the oracle legs decode, where the high word of the Philox frame counter changes:
    pscl_channel_device over frames [2^32 - 40, 2^32 + 40) against test_gpu_channel's NumPy
    restatement (message words exact, normals within its 2e-5; a dropped high word would give the
    rows of frames 0..39, unrelated normals)."""
    info = construct_info_set(N, K)
    dec = _native.Decoder(N, info, 2, POLY)
    B, frame0, seed, sid, kp = 80, 2**32 - 40, 3, philox_stream_id(6.5), K - CRC_BITS
    with _native.DeviceArena(dec) as mem:
        d_llr, d_msg = mem.alloc(B * N * 8), mem.alloc(B * dec.W * 8)
        dec.channel_device(seed, sid, 6.5, K / N, kp, frame0, B, d_llr, d_msg)
        llr = mem.download(d_llr, B * N * 8, np.float64).reshape(B, N)
        words = mem.download(d_msg, B * dec.W * 8, np.uint64).reshape(B, dec.W)
    dec.close()
    msg, ref = host_stream(seed, sid, frame0, B, N, info, K, kp, POLY, 6.5, K / N)
    np.testing.assert_array_equal(words_to_bits(words, K), msg)
    sig = math.sqrt(1.0 / (2.0 * (K / N) * 10 ** 0.65))
    err = np.abs(llr - ref) * sig / 2.0
    assert err.max() < 2e-5, err.max()


# ---------------------------------------------------------------------------------------------
# 2a. the north-star loop
SWEEP_FLAGS = ["--retries", "8", "--rng", "philox", "--include_uncoded", "--seed", "3", "--batch", "7000"]
SWEEP_SNR = [4.0, 4.5, 5.0, 5.5, 6.0, 6.5]
# 3 blocks per point (18 pipelined calls: the kDlPar = 4 scratch sets wrap four times); last blocks
# of 6001, 5995 and 6000 frames; the last range crosses the 32-bit boundary of the frame counter
SWEEP_RANGES = [(0, 20_001), (5, 20_000), (0, 20_000), (12_345, 32_345), (0, 20_000),
                (2**32 - 10_000, 2**32 + 10_000)]


def _sweep_vs_oracle(L, npts, knobs, fused):
    info = construct_info_set(128, 64)
    beta = np.load(GOLDEN / f"beta_M{L}.npy")
    args = rfs.build_argparser().parse_args(["--M", str(L), "--beta", str(GOLDEN / f"beta_M{L}.npy")] + SWEEP_FLAGS)
    pts, ranges = SWEEP_SNR[:npts], SWEEP_RANGES[:npts]
    host = _oracle_points(P128, L, f"M{L}", 8, 3, tuple((s, a, b - a) for s, (a, b) in zip(pts, ranges)))
    # a parity assert cannot show that chains ran: the oracle's own results must
    assert host[0]["scl"][FRAME_ERR] >= 0.05 * host[0]["n"] and host[0]["dl"][RETRIES] > 0
    assert host[2]["scl"][FRAME_ERR] >= 50
    dec = _native.get_decoder(128, info, L, POLY, 0)  # (the handle _philox_sweep_device takes)
    dec.set_tuning(**knobs)
    try:
        before = dec.path_stats()["fused_tx_blocks"]
        got = rfs._philox_sweep_device(args, pts, ranges, info, beta, 0, 40)
        blocks = dec.path_stats()["fused_tx_blocks"] - before
    finally:
        dec.set_tuning(**{k: 0 for k in knobs})
    assert blocks == (3 * npts if fused else 0), f"{blocks} fused-TX blocks of {3 * npts}"
    for i, (snr, r) in enumerate(zip(pts, ranges)):
        _check_point(got[i], host[i], f"L={L} {knobs} {snr} dB frames {r}")


@pytest.mark.parametrize("knobs,fused", [({}, False), ({"tx_fused": 1}, True), ({"tx_fused": 2}, False),
                                         ({"dl_warm_apx": 2}, False)],
                         ids=["default", "tx_fused1", "tx_fused2", "dl_warm_apx2"])
def test_pipelined_sweep_vs_oracle_L8(knobs, fused):
    """run_fer_sweep --M 8 --retries 8 --rng philox --include_uncoded --seed 3 --batch 7000 with
    beta_M8 over 4.0 .. 6.5 dB: every counter of every point against the oracle."""
    _sweep_vs_oracle(8, 6, knobs, fused)


def test_pipelined_sweep_vs_oracle_L4():
    """The same loop at L = 4 / beta_M4, default schedule, on the first three points."""
    _sweep_vs_oracle(4, 3, {}, False)


# ---------------------------------------------------------------------------------------------
# 2b. the CSV rows
def test_run_sweep_rows_and_csv_vs_oracle(tmp_path):
    """run_sweep's returned rows and the written fer_M8.csv against rows computed from the oracle's
    counts with run_sweep's own expressions."""
    frames = 20_000
    args = rfs.build_argparser().parse_args(
        ["--M", "8", "--beta", str(GOLDEN / "beta_M8.npy")] + SWEEP_FLAGS +
        ["--frames", str(frames), "--snr_lo", "4", "--snr_hi", "4.5", "--snr_step", "0.5", "--out_dir", str(tmp_path),
         "--plot_dir", str(tmp_path), "--no_plot"])
    rows = rfs.run_sweep(args)
    snrs = [4.0, 4.5]
    host = _oracle_points(P128, 8, "M8", 8, 3, tuple((s, 0, frames) for s in snrs))
    assert len(rows) == len(snrs)
    want_rows = []
    for row, snr, h in zip(rows, snrs, host):
        bits = np.int64(frames * 64)  # (int64 counters divided as run_sweep divides them)
        want = {"snr_db": float(snr), "fer_scl": np.int64(h["scl"][FRAME_ERR]) / frames,
                "fer_dl": np.int64(h["dl"][FRAME_ERR]) / frames, "ber_scl": np.int64(h["scl"][BIT_ERR]) / bits,
                "ber_dl": np.int64(h["dl"][BIT_ERR]) / bits, "avg_retries": np.int64(h["dl"][RETRIES]) / max(frames, 1)}
        assert set(row) == set(want) | {"fer_uncoded", "ber_uncoded"}
        for k, v in want.items():
            assert row[k] == v, f"{snr} dB {k}: run_sweep {row[k]!r} oracle {v!r}"
        u = h["unc"]
        assert u["n_amb"] < 3 * u["expect"] + 10
        # within n_amb / denominator (1e-6 of a count covers the rounding of the product)
        assert abs(row["fer_uncoded"] * frames - u["frame_err"]) <= u["n_amb"] + 1e-6, (snr, row["fer_uncoded"], u)
        assert abs(row["ber_uncoded"] * (frames * 40) - u["bit_err"]) <= u["n_amb"] + 1e-6, (snr, row["ber_uncoded"], u)
        want_rows.append(dict(want, fer_uncoded=row["fer_uncoded"], ber_uncoded=row["ber_uncoded"]))
    lines = ["snr_db,fer_uncoded,ber_uncoded,fer_scl,ber_scl,fer_dl,ber_dl"]
    for w in want_rows:  # (write_outputs' formats; the uncoded columns were held to the host above)
        lines.append(",".join([f"{w['snr_db']:.3f}"] + [f"{w[k]:.6e}" for k in (
            "fer_uncoded", "ber_uncoded", "fer_scl", "ber_scl", "fer_dl", "ber_dl")]))
    assert (tmp_path / "fer_M8.csv").read_text() == "\n".join(lines) + "\n"


# ---------------------------------------------------------------------------------------------
# 2c. simulate on the codes it never ran on (beta = None: flips ranked by |L0|)
def _simulate_vs_oracle(code, L, retries, snr, seed, frame0, n, blocks=None):
    """One dec.simulate call -- or, with blocks, simulate_device calls of `blocks` frames on a
    pipelined handle -- against the oracle."""
    host, = _oracle_points(code, L, None, retries, seed, ((snr, frame0, n),))
    assert host["dl"][RETRIES] > 0 and host["scl"][FRAME_ERR] > 0  # (chains ran)
    info = construct_info_set(code.N, code.K)
    dec = _native.Decoder(code.N, info, L, POLY)
    if code.E:
        dec.set_rate_match(code.E)
    dec.set_beta(None)
    sid, rate, kp = philox_stream_id(snr), _rate(code), _kp(code)
    if blocks is None:
        got = dec.simulate(seed, sid, snr, rate, kp, frame0, n, retries, True)
    else:
        nc = _native.PSCL_NCOUNT
        dec.set_pipelined(True)
        with _native.DeviceArena(dec) as mem:
            d_cnt = mem.alloc(3 * nc * 8)
            mem.memset(d_cnt, 0, 3 * nc * 8)
            for b0 in range(0, n, blocks):
                dec.simulate_device(seed, sid, snr, rate, kp, frame0 + b0, min(blocks, n - b0), retries, True, d_cnt)
            dec.join()
            dec.sync()
            got = mem.download(d_cnt, 3 * nc * 8, np.int64).reshape(3, nc)
    dec.close()
    _check_point(got, host, f"N={code.N} K={code.K} E={code.E} L={L} {snr} dB blocks={blocks}")


@pytest.mark.parametrize("blocks", [None, 3000], ids=["plain", "pipelined"])
def test_simulate_n256_vs_oracle(blocks):
    """N = 256, K = 128, L = 4, 6 retries at 5 dB: the long TX kernel, the separate uncoded launch
    and the long decoders (restated stream on the CPU, seed 17: 446 of 6000 baselines fail, 1987
    retries)."""
    _simulate_vs_oracle(Code(256, 128, 0), 4, 6, 5.0, 17, 1000, 6000, blocks)


def test_simulate_k88_E256_vs_oracle():
    """(128,88) rate matched to E = 256, L = 8, 8 retries at 5 dB, rate 64/256: repetition, two
    message words, LLR scratch rows of E doubles (restated stream on the CPU, seed 19: 711 of 8000
    baselines fail, 4257 retries)."""
    _simulate_vs_oracle(Code(128, 88, 256), 8, 8, 5.0, 19, 1000, 8000)


def test_simulate_k88_vs_oracle():
    """(128,88) without rate matching, L = 8, 8 retries at 4.5 dB: the runtime-information-set lane
    kernel on the simulate path (restated stream on the CPU, seed 23: 39 of 6000 baselines fail,
    202 retries)."""
    _simulate_vs_oracle(Code(128, 88, 0), 8, 8, 4.5, 23, 1000, 6000)


# E = 100 point, chosen on the CPU with the restated stream and the oracle (seed 29, frames
# [1000, 7000)): 6.0 dB -> 664 of 6000 baselines fail (11.07 %), 4251 retries
# (5.0 dB: 36.93 %, 4.0 dB: 68.07 %)
E100_SNR = 6.0


def test_simulate_E100_punctured_vs_oracle():
    """(128,64) punctured to E = 100 (punctured positions decode as LLR -1.0, rate_match.py:19-39),
    L = 4, 8 retries, rate 40/100."""
    _simulate_vs_oracle(Code(128, 64, 100), 4, 8, E100_SNR, 29, 1000, 6000)


# ---------------------------------------------------------------------------------------------
# 2d. the 2^20 chunk boundary (HIP against HIP, no oracle)
def test_simulate_chunk_boundary_adds_up():
    """One call of 2^20 + 777 frames -- the only size at which simulate's chunk loop runs twice --
    equals the calls over [0, 2^20) and [2^20, 2^20 + 777) added; on a plain handle through
    simulate, then on a pipelined one through simulate_device."""
    info = construct_info_set(128, 64)
    seed, sid, cut, tail, nc = 31, philox_stream_id(5.0), 2**20, 777, _native.PSCL_NCOUNT
    dec = _native.Decoder(128, info, 8, POLY)
    dec.set_beta(np.load(GOLDEN / "beta_M8.npy"))
    one = dec.simulate(seed, sid, 5.0, 0.5, 40, 0, cut + tail, 8, True)
    parts = dec.simulate(seed, sid, 5.0, 0.5, 40, 0, cut, 8, True) + dec.simulate(seed, sid, 5.0, 0.5, 40, cut, tail, 8,
                                                                                 True)
    np.testing.assert_array_equal(one, parts)
    assert one[0][FRAMES] == cut + tail and one[2][FRAMES] == cut + tail
    assert one[0][FRAME_ERR] > 1000 and one[1][RETRIES] > 1000 and one[2][FRAME_ERR] > 0  # (so equality bites)
    dec.set_pipelined(True)
    with _native.DeviceArena(dec) as mem:
        d_one, d_parts = mem.alloc(3 * nc * 8), mem.alloc(3 * nc * 8)
        mem.memset(d_one, 0, 3 * nc * 8)
        mem.memset(d_parts, 0, 3 * nc * 8)
        dec.simulate_device(seed, sid, 5.0, 0.5, 40, 0, cut + tail, 8, True, d_one)
        dec.simulate_device(seed, sid, 5.0, 0.5, 40, 0, cut, 8, True, d_parts)
        dec.simulate_device(seed, sid, 5.0, 0.5, 40, cut, tail, 8, True, d_parts)
        dec.join()
        dec.sync()
        p_one = mem.download(d_one, 3 * nc * 8, np.int64).reshape(3, nc)
        p_parts = mem.download(d_parts, 3 * nc * 8, np.int64).reshape(3, nc)
    dec.close()
    np.testing.assert_array_equal(p_one, p_parts)
    np.testing.assert_array_equal(p_one, one)
