"""GPU: staged decoding at N = 32 .. 1024 -- pscl_sc_device (the lane-parallel SC kernels of
sc_lane.hip, sc128_lane.hip at N = 128) and pscl_escalate_device (the list decode of the frames
whose SC result fails the CRC).  After the SC stage bits, pass flag and stage equal the oracle's
sc_decode + check_crc on every row; after the escalation everything equals the composition
(adaptive_cases.compose), bit for bit."""
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
import oracle
import staged_cases as sc
from polar_code_amd import _native

pytestmark = pytest.mark.gpu

PASS, IDX = _native.PSCL_FLAG_CRC_PASS, _native.PSCL_FLAG_IDX_MASK


class Batch:
    """A device batch of one decoder: rows uploaded, output buffers, and the unpacked outputs."""

    def __init__(self, dec, mem, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        self.dec, self.mem, self.B = dec, mem, len(rows)
        B, W = self.B, dec.W
        self.d_llr = mem.alloc(max(rows.nbytes, 8))
        self.out = dict(d_best=mem.alloc(max(B * W * 8, 8)), d_flags=mem.alloc(max(B, 8)), d_stage=mem.alloc(max(B, 8)))
        if B:
            mem.upload(self.d_llr, rows)

    def sc(self, **kw):
        self.dec.sc_device(self.d_llr, self.B, **self.out, **kw)

    def escalate(self, **kw):
        return self.dec.escalate_device(self.d_llr, self.B, **self.out, **kw)

    def read(self):
        B, W, K = self.B, self.dec.W, self.dec.K
        self.dec.sync()
        w = self.mem.download(self.out["d_best"], max(B * W * 8, 8), np.uint64)[:B * W].reshape(B, W)
        flags = self.mem.download(self.out["d_flags"], max(B, 8), np.uint8)[:B]
        stage = self.mem.download(self.out["d_stage"], max(B, 8), np.uint8)[:B]
        j = np.arange(K)
        bits = ((w[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)
        return {"best_bits": bits, "crc_pass": (flags & PASS) != 0, "best_idx": (flags & IDX).astype(np.int32),
                "stage": stage.copy(), "words": w.copy(), "flags": flags.copy()}


def assert_sc(out, bits, ok, tag):
    np.testing.assert_array_equal(out["best_bits"], bits, err_msg=f"{tag}: SC bits")
    np.testing.assert_array_equal(out["crc_pass"], ok, err_msg=f"{tag}: SC pass flag")
    np.testing.assert_array_equal(out["best_idx"], 0, err_msg=f"{tag}: SC index")
    np.testing.assert_array_equal(out["stage"], np.where(ok, 1, 2), err_msg=f"{tag}: SC stage")


def staged(dec, rows, exp, tag):
    """sc_device, checked against the composition's SC half, then escalate_device, checked whole."""
    with _native.DeviceArena(dec) as mem:
        b = Batch(dec, mem, rows)
        b.sc()
        assert_sc(b.read(), exp["sc_bits"], exp["sc_ok"], tag)
        n = b.escalate()
        out = b.read()
    ac.assert_equals(out, exp, tag)
    assert n == exp["n_escalated"], tag
    return out


def stage1_decides(dec, rows, t, tag):
    with _native.DeviceArena(dec) as mem:
        b = Batch(dec, mem, rows)
        b.sc()
        n = b.escalate()
        out = b.read()
    np.testing.assert_array_equal(out["best_bits"], t, err_msg=f"{tag}: stage-1 bits")
    assert np.all(out["crc_pass"]) and np.all(out["stage"] == 1) and np.all(out["best_idx"] == 0) and n == 0, tag


# ---- 1. mixed batches
@pytest.mark.parametrize("name,L", [("pw256", 8), ("pw512", 8), ("pw1024", 8), ("c64", 8), ("c32", 8),
                                    ("pw512", 4), ("c64", 16), ("pw256", 2)])
def test_mixed_batch_equals_composition(name, L):
    case = sc.mixed_case(name, L)
    B = len(case["rows"])
    assert 0 < case["exp"]["n_escalated"] < B  # (from the oracle alone)
    dec = _native.Decoder(case["N"], case["info"], L, case["crc"])
    staged(dec, case["rows"], case["exp"], f"{name} L={L}")
    host = dec.decode_staged(case["rows"])
    ac.assert_equals(host, case["exp"], f"{name} L={L}: decode_staged")
    assert host["n_escalated"] == case["exp"]["n_escalated"]
    bits, ok = dec.decode_sc(case["rows"])
    np.testing.assert_array_equal(bits, case["exp"]["sc_bits"])
    np.testing.assert_array_equal(ok, case["exp"]["sc_ok"])


# ---- 2. every branch state
@pytest.mark.parametrize("N,name", [(N, n) for N in sc.LENGTHS for n, _ in sc.block_family(N)])
def test_every_branch_state(N, name):
    """Every block set of every length at L = 4: the raw rows equal the composition; on the shifted
    rows stage 1 decides every frame and its bits are the random CRC-valid targets."""
    case = sc.family_case(N, name)
    B = len(case["raw"])
    assert B == (259 if N <= 64 else 67) and case["t"].any(axis=1).sum() > B // 2
    dec = _native.Decoder(N, case["info"], 4, case["crc"])
    stage1_decides(dec, case["shifted"], case["t"], f"N={N} {name} shifted")
    staged(dec, case["raw"], case["exp"], f"N={N} {name} raw")


# ---- 3. epilogue edges
@pytest.mark.parametrize("N,K", [(256, 27), (256, 63), (256, 65), (256, 129), (256, 250), (1024, 513), (1024, 960)])
def test_epilogue_edges(N, K):
    """K on either side of the output-word boundaries and in a partial syndrome nibble (constructed
    sets, CRC-24, L = 4, B = 67)."""
    info = ac.info_set(N, K)
    raw = ac.make_llr(300 + N + K, 67, info, ac.POLY24, 4.0, N=N)
    dec = _native.Decoder(N, info, 4, ac.POLY24)
    staged(dec, raw, ac.compose(raw, info, 4, ac.POLY24, N=N), f"({N},{K}) raw")
    rows, t = ac.shift_to_valid(raw, info, ac.POLY24, seed=310 + K, N=N)
    stage1_decides(dec, rows, t, f"({N},{K}) shifted")


# ---- 4. exact-arithmetic corners
def _corner_rows(N, info):
    rng = np.random.default_rng(4300 + N)
    K = len(info)
    cw = np.empty((48, N))
    for b in range(48):  # noiseless codewords at +-c: every f a tie, g sums exactly 0 or 2 c
        u = np.zeros(N, np.int8)
        u[info] = rng.integers(0, 2, size=K)
        cw[b] = (1.0 - 2.0 * oracle.polar_transform(u)) * (1.0, 2.5, 1e30)[b % 3]
    small = rng.choice([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], size=(64, N))
    return np.concatenate([np.zeros((3, N)), -np.zeros((2, N)), cw, small])


@pytest.mark.parametrize("N", [256, 1024])
def test_exact_arithmetic_corners(N):
    info = sc.pw_info_set(N, N // 2)
    rows = _corner_rows(N, info)
    bits, ok = sc.sc_expected(rows, info, ac.POLY24)
    assert bits[:5].sum() == 0 and bits[5:53].any() and 0 < ok.sum()
    dec = _native.Decoder(N, info, 4, ac.POLY24)
    with _native.DeviceArena(dec) as mem:
        b = Batch(dec, mem, rows)
        b.sc()
        assert_sc(b.read(), bits, ok, f"N={N} corners")


# ---- 5. past the grid cap
def _frames_per_grid_pass(N):
    """From the source, failing loudly when a pattern is gone, so that a change of the grid cap
    cannot quietly leave these tests inside one grid pass."""
    src = (Path(_native.__file__).resolve().parent / "csrc" / "sc_lane.hip").read_text()
    vals = []
    for pat in (r"constexpr int kScLaneGridCap = (\d+);", r"constexpr int kWavesPerWg = (\d+);"):
        m = re.search(pat, src)
        assert m, f"sc_lane.hip: {pat} not found; update the pattern with the kernel"
        vals.append(int(m.group(1)))
    assert re.search(r"if \(grid > kScLaneGridCap\) grid = kScLaneGridCap;", src)
    assert re.search(r"constexpr int groupLanes\(int N\) \{ return N / 32 > 4 \? N / 32 : 4; \}", src)
    return vals[0] * vals[1] * (64 // max(4, N // 32))


@pytest.mark.parametrize("name,reps", [("pw1024", 63), ("c64", 254)])
def test_past_the_grid_cap(name, reps):
    case = sc.mixed_case(name)
    B = reps * len(case["rows"])
    assert B > _frames_per_grid_pass(case["N"]), (B, _frames_per_grid_pass(case["N"]))
    dec = _native.Decoder(case["N"], case["info"], 8, case["crc"])
    want = ac.tiled(case["exp"], reps)
    want["sc_bits"], want["sc_ok"] = np.tile(case["exp"]["sc_bits"], (reps, 1)), np.tile(case["exp"]["sc_ok"], reps)
    staged(dec, np.tile(case["rows"], (reps, 1)), want, f"{name} x {reps}")


# ---- 6. N = 128: the two halves equal the adaptive call
def _adaptive_equals_halves(dec, rows):
    with _native.DeviceArena(dec) as mem:
        a, b = Batch(dec, mem, rows), Batch(dec, mem, rows)
        na = dec.adaptive_device(a.d_llr, a.B, **a.out)
        b.sc()
        nb = b.escalate()
        oa, ob = a.read(), b.read()
    assert na == nb and 0 < na < len(rows)
    for k in ("words", "flags", "stage"):
        np.testing.assert_array_equal(oa[k], ob[k], err_msg=k)


def test_n128_halves_equal_adaptive_device():
    _adaptive_equals_halves(_native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24), ac.mixed_rows())
    dec = _native.Decoder(128, ac.info_set(128, 88), 8, ac.POLY24)
    dec.set_rate_match(256)
    _adaptive_equals_halves(dec, ac.nr_case()[0])


# ---- 7. counters
def test_counters_with_reference():
    case = sc.mixed_case("pw256")
    rows, exp, K, kp = case["rows"], case["exp"], 128, 104
    B, NC = len(rows), _native.PSCL_NCOUNT
    ref = exp["list_bits"] ^ (np.random.default_rng(98).random(exp["list_bits"].shape) < 0.01).astype(np.int8)
    want_sc = sc.host_counts(exp["sc_bits"], exp["sc_ok"], ref, kp, NC)
    want_fin = sc.host_counts(exp["best_bits"], exp["crc_pass"], ref, kp, NC, exp["n_escalated"])
    assert want_sc[1] == exp["n_escalated"] and want_sc[2] > want_fin[2] > 0
    dec = _native.Decoder(256, case["info"], 8, ac.POLY24)
    with _native.DeviceArena(dec) as mem:
        b = Batch(dec, mem, rows)
        d_ref, d_c1, d_c2 = mem.alloc(B * dec.W * 8), mem.alloc(8 * NC), mem.alloc(8 * NC)
        mem.upload(d_ref, sc.words(ref))
        mem.memset(d_c1, 0, 8 * NC)
        mem.memset(d_c2, 0, 8 * NC)
        for calls in (1, 2):  # two rounds into the same counters add up
            b.sc(d_ref=d_ref, k_payload=kp, d_counters=d_c1)
            assert b.escalate(d_ref=d_ref, k_payload=kp, d_counters=d_c2) == exp["n_escalated"]
            dec.sync()
            np.testing.assert_array_equal(mem.download(d_c1, 8 * NC, np.int64), calls * want_sc, err_msg="SC counters")
            np.testing.assert_array_equal(mem.download(d_c2, 8 * NC, np.int64), calls * want_fin, err_msg="final counters")
    with pytest.raises(ValueError):
        dec.sc_device(1, 1, d_best=1, d_flags=1, d_ref=1, d_counters=0)


# ---- 8. ordering
def test_tensor_entry_on_a_side_stream():
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    case = sc.mixed_case("pw256")
    dec = SCLDecoder(256, case["info"], 8, ac.POLY24)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        llr = torch.from_numpy(case["rows"].copy()).to("cuda")
        best, flags, stage = dec.decode_tensor_staged(llr)
    stream.synchronize()
    flags, exp = flags.cpu().numpy(), case["exp"]
    np.testing.assert_array_equal(best.cpu().numpy().view(np.uint64), sc.words(exp["best_bits"]))
    np.testing.assert_array_equal((flags & PASS) != 0, exp["crc_pass"])
    np.testing.assert_array_equal(flags & IDX, exp["best_idx"])
    np.testing.assert_array_equal(stage.cpu().numpy(), exp["stage"])
    host = dec.decode_staged(case["rows"])
    np.testing.assert_array_equal(host["bits"], exp["best_bits"])
    dec.native.set_stream(None)


def test_sc_behind_a_pending_pipelined_decode():
    case = sc.mixed_case("pw256")
    rows, exp = case["rows"], case["exp"]
    B = len(rows)
    dec = _native.Decoder(256, case["info"], 8, ac.POLY24)
    with _native.DeviceArena(dec) as mem:
        b = Batch(dec, mem, rows)
        pb, pf = mem.alloc(B * dec.W * 8), mem.alloc(B)
        dec.set_pipelined(True)
        dec.decode_device(b.d_llr, B, d_best=pb, d_flags=pf)  # pipelined: its re-decode may be pending
        b.sc()
        n = b.escalate()
        dec.set_pipelined(False)
        out = b.read()
        w, f = mem.download(pb, B * dec.W * 8, np.uint64).reshape(B, dec.W), mem.download(pf, B, np.uint8)
    ac.assert_equals(out, exp, "behind a pipelined decode")
    assert n == exp["n_escalated"]
    np.testing.assert_array_equal(w, sc.words(exp["list_bits"]))
    np.testing.assert_array_equal(f, (np.where(exp["list_ok"], PASS, 0) | exp["list_idx"]).astype(np.uint8))


def test_next_batch_sc_before_this_batch_escalation():
    case = sc.mixed_case("pw256")
    rows, exp = case["rows"], case["exp"]
    h = len(rows) // 2
    parts = [(rows[:h], slice(0, h)), (rows[h:], slice(h, None))]
    dec = _native.Decoder(256, case["info"], 8, ac.POLY24)
    with _native.DeviceArena(dec) as mem:
        b0, b1 = (Batch(dec, mem, r) for r, _ in parts)
        b0.sc()
        b1.sc()  # batch 1's SC stage is queued before batch 0's escalation waits on the host
        n0 = b0.escalate()
        n1 = b1.escalate()
        outs = [b0.read(), b1.read()]
    for out, n, (_, sl) in zip(outs, (n0, n1), parts):
        ac.assert_equals(out, exp, f"batch {sl}", sl)
        assert n == int(np.count_nonzero(exp["stage"][sl] == 2))
    assert n0 + n1 == exp["n_escalated"]


# ---- 9. errors
def test_errors():
    with pytest.raises(NotImplementedError):
        _native.Decoder(16, ac.info_set(16, 12), 4, sc.POLY8).decode_sc(np.ones((2, 16)))
    rm = _native.Decoder(256, ac.info_set(256, 128), 4, ac.POLY24)
    rm.set_rate_match(300)
    with pytest.raises(NotImplementedError):
        rm.decode_sc(np.ones((2, 300)))
    nocrc = _native.Decoder(256, ac.info_set(256, 128), 4, None)
    bits, ok = nocrc.decode_sc(np.ones((3, 256)))  # without a CRC the pass flag is set
    assert bits.shape == (3, 128) and not bits.any() and ok.all()
    with pytest.raises(ValueError):
        nocrc.decode_staged(np.ones((2, 256)))
    dec = _native.Decoder(256, ac.info_set(256, 128), 4, ac.POLY24)
    out = dec.decode_staged(np.zeros((0, 256)))  # B = 0 is fine
    assert out["n_escalated"] == 0 and out["best_bits"].shape == (0, 128)
