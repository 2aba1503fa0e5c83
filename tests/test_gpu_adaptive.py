"""GPU: adaptive decoding (pscl_adaptive_device) -- the lane-parallel SC kernel on every frame, the
list decoder only on the frames whose SC result fails the CRC.  Bits, CRC flag, best index, stage
and the escalated count equal the composition of the oracle's sc_decode + check_crc and
decode_batch (adaptive_cases.compose), bit for bit."""
import numpy as np
import pytest

import adaptive_cases as ac
import oracle
from polar_code_amd import _native

pytestmark = pytest.mark.gpu


def _words(bits):
    B, K = bits.shape
    W = (K + 63) // 64
    w = np.zeros((B, W), np.uint64)
    for j in range(K):
        w[:, j >> 6] |= bits[:, j].astype(np.uint64) << np.uint64(j & 63)
    return w


def _check(dec, rows, exp, tag, sl=slice(None)):
    out = dec.decode_adaptive(rows)
    ac.assert_equals(out, exp, tag, sl)
    assert out["n_escalated"] == int(np.count_nonzero(exp["stage"][sl] == 2)), tag
    return out


@pytest.fixture(scope="module")
def dec8():
    return _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)


@pytest.mark.parametrize("L", [8, 4])
def test_mixed_batch_equals_composition(L, dec8):
    exp = ac.mixed_expected(L)
    B = len(ac.mixed_rows())
    assert B == 4099 and 0.15 * B < exp["n_escalated"] < 0.5 * B  # (the oracle alone: 1040 with this seed)
    dec = dec8 if L == 8 else _native.Decoder(128, ac.info_set(128, 64), L, ac.POLY24)
    out = _check(dec, ac.mixed_rows(), exp, f"mixed L={L}")
    differs = int(np.count_nonzero((exp["best_bits"] != exp["list_bits"]).any(axis=1)))
    if differs == 0:
        pytest.skip("this seed gives no frame where the composition differs from plain SCL")
    assert np.count_nonzero((out["best_bits"] != exp["list_bits"]).any(axis=1)) == differs


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_small_and_ragged_batches(B, dec8):
    _check(dec8, ac.mixed_rows()[:B], ac.mixed_expected(8), f"B={B}", slice(0, B))


def test_no_frame_escalates(dec8):
    rows, exp = ac.allpass_case()
    assert exp["n_escalated"] == 0
    out = _check(dec8, rows, exp, "all pass")
    assert out["n_escalated"] == 0 and np.all(out["stage"] == 1)


def test_every_frame_escalates(dec8):
    rows, exp = ac.allfail_case()
    assert exp["n_escalated"] == len(rows)
    out = _check(dec8, rows, exp, "all fail")
    np.testing.assert_array_equal(out["best_bits"], exp["list_bits"])  # plain L = 8 exactly
    np.testing.assert_array_equal(out["best_idx"], exp["list_idx"])
    np.testing.assert_array_equal(out["crc_pass"], exp["list_ok"])


def test_nr_rate_matched():
    info, E, B = ac.info_set(128, 88), 256, 2051
    rows, exp = ac.nr_case()
    assert rows.shape == (B, E) and 0 < exp["n_escalated"] < B  # (the oracle: 920 SC passes)
    dec = _native.Decoder(128, info, 8, ac.POLY24)
    dec.set_rate_match(E)
    _check(dec, rows, exp, "NR (128,88) E=256")


@pytest.mark.parametrize("E", [100, 400])
def test_other_rate_matched_lengths(E):
    """E < N (positions beyond E padded) and E = 3 N + 16 (means over 3 and 4 repeats: the
    de-rate-match's division and its power-of-two form side by side)."""
    info, B = ac.info_set(128, 64), 300
    rows = ac.make_llr(80 + E, B, info, ac.POLY24, 5.0, E=E)
    exp = ac.compose(rows, info, 4, ac.POLY24, E=E)
    dec = _native.Decoder(128, info, 4, ac.POLY24)
    dec.set_rate_match(E)
    _check(dec, rows, exp, f"(128,64) E={E}")


def test_runtime_info_set_and_crc16():
    """(128,40) + CRC-16: the run-time mask with another frozen-sub-tree pattern; stage 2 of this
    code is the handle's plain decode through the runtime-information-set screening kernel."""
    info, B = ac.info_set(128, 40), 2051
    rows = ac.make_llr(78, B, info, ac.POLY16, 3.0)
    exp = ac.compose(rows, info, 4, ac.POLY16)
    assert 0 < exp["n_escalated"] < B  # (the oracle: 640 SC passes)
    dec = _native.Decoder(128, info, 4, ac.POLY16)
    _check(dec, rows, exp, "(128,40) CRC-16")


def _corner_rows(golden):
    rng = np.random.default_rng(4242)
    a = rng.choice([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], size=(96, 128))            # zeros of both signs, ties
    b = rng.choice([-1.0, 1.0], size=(64, 128))                                  # every min a tie
    c = rng.choice([-1e30, 1e30, -1.0, 1.0, 0.0, 3.5e29], size=(96, 128))        # magnitudes up to 1e30
    return np.concatenate([golden("g9_sc.npz")["llr"], a, b, c])


def _make_sc_pass(rows, info, crc):
    """Rows whose SC result passes the CRC, made from `rows` by codeword sign flips: SC commutes
    with the sign pattern of a codeword (f and g are odd in the flipped operands), so flipping by
    the codeword of the SC result moves that result to the all-zero message, which passes.  A leaf
    LLR of exactly zero breaks the symmetry (it decides 0 either way); such rows are retried and
    dropped if they do not settle.  Every value keeps its magnitude: ties and zeros survive."""
    keep = []
    for r in rows:
        r = r.copy()
        for _ in range(6):
            s = oracle.sc_decode(r, info)
            if not s.any():
                keep.append(r)
                break
            u = np.zeros(128, np.int8)
            u[info] = s
            r = np.where(oracle.polar_transform(u) == 1, -r, r)
    return np.array(keep)


def test_exact_arithmetic_corners_in_stage_1(golden, dec8):
    info = ac.info_set(128, 64)
    np.testing.assert_array_equal(golden("g9_sc.npz")["info"], info)
    raw = _corner_rows(golden)
    # the composition on the raw rows (most fail the CRC here)
    _check(dec8, raw, ac.compose(raw, info, 8, ac.POLY24), "corners, raw")
    # and rows on which stage 1 decides every frame: its bits are the oracle's SC bits on every row
    rows = _make_sc_pass(raw, info, ac.POLY24)
    assert len(rows) >= len(raw) // 2
    assert np.any(rows == 0.0) and np.any(np.signbit(rows) & (rows == 0.0)) and np.abs(rows).max() == 1e30
    sc = np.stack([oracle.sc_decode(r, info) for r in rows])
    assert all(oracle.check_crc(b, ac.POLY24) for b in sc)
    out = dec8.decode_adaptive(rows)
    assert out["n_escalated"] == 0 and np.all(out["stage"] == 1) and np.all(out["crc_pass"])
    np.testing.assert_array_equal(out["best_bits"], sc)


def _stage1_decides(dec, rows, t, tag):
    out = dec.decode_adaptive(rows)
    np.testing.assert_array_equal(out["best_bits"], t, err_msg=f"{tag}: stage-1 bits")
    assert np.all(out["crc_pass"]), tag
    assert np.all(out["stage"] == 1) and np.all(out["best_idx"] == 0) and out["n_escalated"] == 0, tag


@pytest.mark.parametrize("name", [n for n, _ in ac.family()])
def test_every_branch_state(name):
    """The 14 block sets (every SC node in each of its three states, the root skips, full and empty
    mask words, the lane offsets 0, 32, 32, 64) and the 5 edge sets (K = 27, 63, 65, 90: partial
    syndrome nibbles, one and two output words; the mirrored (128,64) set), B = 256 + 3, L = 4.  On
    the shifted rows stage 1 decides every frame and its bits are the random CRC-valid targets; the
    raw rows equal the composition (there the runtime-information-set list kernel runs, and for
    K = 65, 90 the gather and scatter with two words)."""
    case = ac.family_case(name)
    B = len(case["raw"])
    assert B == 259 and case["t"].any(axis=1).sum() > B // 2  # (K = 27 has 3 payload bits: some targets are zero)
    dec = _native.Decoder(128, case["info"], 4, ac.POLY24)
    _stage1_decides(dec, case["shifted"], case["t"], f"{name} shifted")
    _check(dec, case["raw"], case["exp"], f"{name} raw")


@pytest.mark.parametrize("E", [200, 256])
def test_rate_matched_front_end_on_a_block_set(E):
    """A set that is not reliability ordered behind the rate-matched front end.  E = 200: one
    repeat plus a remainder of 72, the de-rate-match's means over 2 values and over 1; E = 256:
    every mean over 2.  The rows are shifted through the TX chain so that stage 1 decides."""
    info, B = ac.family_set("bit3=0"), 259
    raw = ac.make_llr(600 + E, B, info, ac.POLY24, 5.0, E=E)
    rows, t = ac.shift_to_valid(raw, info, ac.POLY24, seed=700 + E, E=E)
    dec = _native.Decoder(128, info, 4, ac.POLY24)
    dec.set_rate_match(E)
    _stage1_decides(dec, rows, t, f"bit3=0 E={E} shifted")
    _check(dec, raw, ac.compose(raw, info, 4, ac.POLY24, E=E), f"bit3=0 E={E} raw")


def _source_ints(pattern, what):
    """Integers of the SC source, by pattern -- failing loudly when the pattern is gone, so that a
    change of a grid cap cannot quietly leave these tests inside one grid pass."""
    import re
    from pathlib import Path

    src = (Path(_native.__file__).resolve().parent / "csrc" / "sc128_lane.hip").read_text()
    m = re.search(pattern, src, re.S)
    assert m, f"sc128_lane.hip: {what} not found; update the pattern with the kernel"
    return [int(g) for g in m.groups()]


def _frames_per_grid_pass(rm):
    cap, cap2 = _source_ints(r"int64_t pscl_sc_lane_grid\([^{]*\{.*?if \(grid > (\d+)\) grid = (\d+);", "the SC grid cap")
    (fpw,) = _source_ints(r"constexpr int kFramesPerWave = (\d+);", "frames per wavefront")
    w_rm, w_plain = _source_ints(r"constexpr int wavesPerWg\(bool rm\) \{ return rm \? (\d+) : (\d+); \}", "wavefronts per workgroup")
    assert cap == cap2
    return cap * fpw * (w_rm if rm else w_plain)


def _timed_tiled(dec, rows, exp, reps, tag):
    import time

    t0 = time.perf_counter()
    big = np.tile(rows, (reps, 1))
    want = ac.tiled(exp, reps)
    t1 = time.perf_counter()
    out = dec.decode_adaptive(big)
    t2 = time.perf_counter()
    ac.assert_equals(out, want, tag)
    assert out["n_escalated"] == want["n_escalated"], tag
    print(f"{tag}: B = {len(big)}, {out['n_escalated']} escalated; tile {t1 - t0:.3f} s, "
          f"upload + decode + unpack {t2 - t1:.3f} s, compare {time.perf_counter() - t2:.3f} s")
    return out


def test_plain_rows_past_the_grid_cap(dec8):
    """B = 33 * 4099 = 135267 > 2048 * 64: the frame loop's second iteration (workgroups 0..65)."""
    reps = 33
    B = reps * len(ac.mixed_rows())
    per_pass = _frames_per_grid_pass(False)
    assert B == 135267 and B > per_pass, (B, per_pass)
    _timed_tiled(dec8, ac.mixed_rows(), ac.mixed_expected(8), reps, "plain, two grid passes")


def test_rate_matched_rows_past_the_grid_cap():
    """B = 40 * 2051 = 82040 > 2048 * 32: about 16.5 k frames (516 workgroups) take the second
    iteration, which reuses the wavefront's LDS staging rows behind the second fence."""
    reps = 40
    rows, exp = ac.nr_case()
    B = reps * len(rows)
    per_pass = _frames_per_grid_pass(True)
    assert B == 82040 and B - per_pass > 16000, (B, per_pass)
    dec = _native.Decoder(128, ac.info_set(128, 88), 8, ac.POLY24)
    dec.set_rate_match(256)
    _timed_tiled(dec, rows, exp, reps, "rate matched, two grid passes")


def test_gather_past_its_grid_cap(dec8):
    """Every one of B = 132000 frames escalates: n * 128 values exceed the gather kernel's
    65536 * 256 threads, so its grid-stride loop takes a second step; results are plain L = 8's."""
    reps = 132
    rows, exp = ac.allfail_case()
    B = reps * len(rows)
    per, cap, cap2, per2 = _source_ints(
        r"pscl_launch_gather_rows\([^{]*\{.*?\(n \* row \+ \d+\) / (\d+);\s*if \(grid > (\d+)\) grid = (\d+);.*?dim3\((\d+)\), 0, s, llr",
        "the gather kernel's grid cap")
    assert per == per2 and cap == cap2  # (threads per block; blocks)
    assert B == 132000 and exp["n_escalated"] == len(rows) and B * 128 > cap * per, (B, cap, per)
    out = _timed_tiled(dec8, rows, exp, reps, "all escalate, gather stride")
    assert out["n_escalated"] == B and np.all(out["stage"] == 2)
    np.testing.assert_array_equal(out["best_bits"], np.tile(exp["list_bits"], (reps, 1)))
    np.testing.assert_array_equal(out["best_idx"], np.tile(exp["list_idx"], reps))
    np.testing.assert_array_equal(out["crc_pass"], np.tile(exp["list_ok"], reps))


def test_counters_with_reference(dec8):
    rows, exp = ac.mixed_rows(), ac.mixed_expected(8)
    B, K, kp = len(rows), 64, 40
    rng = np.random.default_rng(99)
    ref = exp["list_bits"].copy()
    flip = rng.random(ref.shape) < 0.01
    ref ^= flip.astype(np.int8)
    d = exp["best_bits"] != ref
    want = np.zeros(_native.PSCL_NCOUNT, np.int64)
    want[_native.CNT_FRAMES] = B
    want[_native.CNT_FRAME_ERR] = np.count_nonzero(~exp["crc_pass"])
    want[_native.CNT_BIT_ERR] = d.sum()
    want[_native.CNT_PAYLOAD_ERR] = np.count_nonzero(d[:, :kp].any(axis=1))
    want[_native.CNT_PAYLOAD_BIT] = d[:, :kp].sum()
    want[_native.CNT_ESCALATED] = exp["n_escalated"]
    with _native.DeviceArena(dec8) as mem:
        d_llr, d_ref = mem.alloc(rows.nbytes), mem.alloc(B * 8)
        d_best, d_flags, d_cnt = mem.alloc(B * 8), mem.alloc(B), mem.alloc(8 * _native.PSCL_NCOUNT)
        mem.upload(d_llr, rows)
        mem.upload(d_ref, _words(ref))
        mem.memset(d_cnt, 0, 8 * _native.PSCL_NCOUNT)
        for calls in (1, 2):  # two calls into the same counters add up
            n = dec8.adaptive_device(d_llr, B, d_best=d_best, d_flags=d_flags, d_ref=d_ref, k_payload=kp, d_counters=d_cnt)
            assert n == exp["n_escalated"]
            dec8.sync()
            got = mem.download(d_cnt, 8 * _native.PSCL_NCOUNT, np.int64)
            np.testing.assert_array_equal(got, calls * want, err_msg=f"after {calls} call(s)")
    with pytest.raises(ValueError):
        dec8.adaptive_device(1, 1, d_best=1, d_flags=1, d_ref=1, d_counters=0)


def test_tensor_entry_on_a_side_stream():
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    rows, exp = ac.mixed_rows()[:1500], ac.mixed_expected(8)
    dec = SCLDecoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    host = dec.decode_adaptive(rows)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        llr = torch.from_numpy(rows.copy()).to("cuda")
        best, flags, stage = dec.decode_tensor_adaptive(llr)
    stream.synchronize()
    flags, stage = flags.cpu().numpy(), stage.cpu().numpy()
    words = best.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(words, _words(host["bits"]))
    np.testing.assert_array_equal((flags & _native.PSCL_FLAG_CRC_PASS) != 0, host["crc_pass"])
    np.testing.assert_array_equal(flags & _native.PSCL_FLAG_IDX_MASK, host["best_idx"])
    np.testing.assert_array_equal(stage, host["stage"])
    np.testing.assert_array_equal(host["bits"], exp["best_bits"][:1500])
    dec.native.set_stream(None)


def test_behind_a_pending_pipelined_decode_and_plain_decode_unchanged():
    rows, exp = ac.mixed_rows(), ac.mixed_expected(8)
    B = len(rows)
    fresh = _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24).decode_adaptive(rows)
    dec = _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    with _native.DeviceArena(dec) as mem:
        d_llr = mem.alloc(rows.nbytes)
        mem.upload(d_llr, rows)
        pb, pf = [mem.alloc(B * 8) for _ in range(3)], [mem.alloc(B) for _ in range(3)]
        ab, af, ast = mem.alloc(B * 8), mem.alloc(B), mem.alloc(B)
        dec.decode_device(d_llr, B, d_best=pb[0], d_flags=pf[0])  # plain, before
        dec.set_pipelined(True)
        dec.decode_device(d_llr, B, d_best=pb[1], d_flags=pf[1])  # pipelined: its re-decode is pending
        n = dec.adaptive_device(d_llr, B, d_best=ab, d_flags=af, d_stage=ast)
        dec.set_pipelined(False)
        dec.decode_device(d_llr, B, d_best=pb[2], d_flags=pf[2])  # plain, after
        dec.sync()
        plain = [(mem.download(pb[i], B * 8, np.uint64), mem.download(pf[i], B, np.uint8)) for i in range(3)]
        words, flags, stage = mem.download(ab, B * 8, np.uint64), mem.download(af, B, np.uint8), mem.download(ast, B, np.uint8)
    assert n == fresh["n_escalated"] == exp["n_escalated"]
    np.testing.assert_array_equal(words, _words(fresh["best_bits"])[:, 0])
    np.testing.assert_array_equal((flags & 0x80) != 0, fresh["crc_pass"])
    np.testing.assert_array_equal(flags & 0x3F, fresh["best_idx"])
    np.testing.assert_array_equal(stage, fresh["stage"])
    want_w, want_f = _words(exp["list_bits"])[:, 0], np.where(exp["list_ok"], 0x80, 0) | exp["list_idx"]
    for i, (w, f) in enumerate(plain):
        np.testing.assert_array_equal(w, want_w, err_msg=f"plain decode {i}: words")
        np.testing.assert_array_equal(f, want_f.astype(np.uint8), err_msg=f"plain decode {i}: flags")


def test_errors():
    rows = ac.mixed_rows()[:4]
    with pytest.raises(ValueError):
        _native.Decoder(128, ac.info_set(128, 64), 8, None).decode_adaptive(rows)
    with pytest.raises(NotImplementedError, match="N = 128"):
        _native.Decoder(256, ac.info_set(256, 128), 4, ac.POLY24).decode_adaptive(np.ones((2, 256)))
    dec = _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    assert dec.decode_adaptive(np.zeros((0, 128)))["n_escalated"] == 0  # B = 0 is fine
