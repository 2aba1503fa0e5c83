"""GPU: the float32-row entry points (pscl_sc_device_f32, pscl_decode_device_f32,
pscl_escalate_device_f32, pscl_adaptive_async_device_f32).  Every test builds its rows as float32,
widens them on the host (astype(np.float64), exact) and takes its expected values from the oracle
alone on the widened rows; where the float64 entry point exists its outputs on the widened rows are
compared too, word for word.  No tolerance anywhere: widening is exact, so the contract is equality."""
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
import f32_cases as fc
import staged_cases as sg
from polar_code_amd import _native

pytestmark = pytest.mark.gpu

NC = _native.PSCL_NCOUNT
PASS, IDX = _native.PSCL_FLAG_CRC_PASS, _native.PSCL_FLAG_IDX_MASK
EUNSUP, EINVAL = -5, -1
SENTINEL = 0x5A


def _bits(words, K):
    j = np.arange(K)
    return ((words[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)


class Batch:
    """Rows on the device (float32: optionally starting `offset` bytes into their allocation), output
    buffers of B + pad frames pre-filled with a sentinel, optional reference words and counters."""

    def __init__(self, dec, mem, rows, offset=0, pad=0, ref_bits=None):
        assert rows.dtype in (np.float32, np.float64) and rows.flags.c_contiguous
        self.dec, self.mem, self.B, self.pad, self.f32 = dec, mem, len(rows), pad, rows.dtype == np.float32
        B, W = self.B, dec.W
        self.d_llr = mem.alloc(max(rows.nbytes, 8) + offset) + offset
        if B:
            mem.upload(self.d_llr, rows)
        n = B + pad
        self.d_best, self.d_flags, self.d_stage = mem.alloc(max(n * W * 8, 8)), mem.alloc(max(n, 8)), mem.alloc(max(n, 8))
        for d, size in ((self.d_best, n * W * 8), (self.d_flags, n), (self.d_stage, n)):
            mem.memset(d, SENTINEL, max(size, 8))
        self.d_n, self.d_cnt, self.d_ref = mem.alloc(8), mem.alloc(8 * NC), 0
        mem.memset(self.d_n, 0xFF, 8)
        mem.memset(self.d_cnt, 0, 8 * NC)
        if ref_bits is not None:
            self.d_ref = mem.alloc(B * W * 8)
            mem.upload(self.d_ref, sg.words(ref_bits))

    def _ref(self, kp):
        return dict(d_ref=self.d_ref, k_payload=kp, d_counters=self.d_cnt) if self.d_ref else {}

    def sc(self, kp=0):
        f = self.dec.sc_device_f32 if self.f32 else self.dec.sc_device
        f(self.d_llr, self.B, d_best=self.d_best, d_flags=self.d_flags, d_stage=self.d_stage, **self._ref(kp))

    def decode(self, kp=0):
        f = self.dec.decode_device_f32 if self.f32 else self.dec.decode_device
        f(self.d_llr, self.B, d_best=self.d_best, d_flags=self.d_flags, **self._ref(kp))

    def escalate(self, kp=0):
        f = self.dec.escalate_device_f32 if self.f32 else self.dec.escalate_device
        return f(self.d_llr, self.B, d_best=self.d_best, d_flags=self.d_flags, d_stage=self.d_stage, **self._ref(kp))

    def adaptive(self, kp=0):
        f = self.dec.adaptive_async_device_f32 if self.f32 else self.dec.adaptive_async_device
        f(self.d_llr, self.B, d_best=self.d_best, d_flags=self.d_flags, d_stage=self.d_stage, d_n_escalated=self.d_n,
          **self._ref(kp))

    def read(self, sync=True):
        """The outputs of the B frames; asserts that the pad frames behind them still hold the sentinel."""
        B, W, K, n = self.B, self.dec.W, self.dec.K, self.B + self.pad
        if sync:
            self.dec.sync()
        w = self.mem.download(self.d_best, max(n * W * 8, 8), np.uint64)[:n * W].reshape(n, W)
        flags = self.mem.download(self.d_flags, max(n, 8), np.uint8)[:n]
        stage = self.mem.download(self.d_stage, max(n, 8), np.uint8)[:n]
        assert np.all(w[B:] == np.uint64(0x5A5A5A5A5A5A5A5A)) and np.all(flags[B:] == SENTINEL) and np.all(stage[B:] == SENTINEL), \
            "outputs written behind frame B"
        w, flags, stage = w[:B], flags[:B], stage[:B]
        return {"best_bits": _bits(w, K), "crc_pass": (flags & PASS) != 0, "best_idx": (flags & IDX).astype(np.int32),
                "stage": stage.copy(), "words": w.copy(), "flags": flags.copy(),
                "n_escalated": int(self.mem.download(self.d_n, 8, np.int32)[0]),
                "counters": self.mem.download(self.d_cnt, 8 * NC, np.int64)}


def assert_sc(out, bits, ok, tag):
    np.testing.assert_array_equal(out["best_bits"], bits, err_msg=f"{tag}: SC bits")
    np.testing.assert_array_equal(out["crc_pass"], ok, err_msg=f"{tag}: SC pass flag")
    np.testing.assert_array_equal(out["best_idx"], 0, err_msg=f"{tag}: SC index")
    np.testing.assert_array_equal(out["stage"], np.where(ok, 1, 2), err_msg=f"{tag}: SC stage")


def assert_list(out, exp, tag, sl=slice(None)):
    np.testing.assert_array_equal(out["best_bits"], exp["list_bits"][sl], err_msg=f"{tag}: list bits")
    np.testing.assert_array_equal(out["crc_pass"], exp["list_ok"][sl], err_msg=f"{tag}: list pass flag")
    np.testing.assert_array_equal(out["best_idx"], exp["list_idx"][sl], err_msg=f"{tag}: list index")


def assert_same(a, b, tag, keys=("words", "flags", "stage")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {k} differs from the float64 entry point's")


def sc_both(dec, rows32, bits, ok, tag, offset=0, pad=0):
    """sc_device_f32 against the oracle and against sc_device on the widened rows."""
    with _native.DeviceArena(dec) as mem:
        a, b = Batch(dec, mem, rows32, offset=offset, pad=pad), Batch(dec, mem, fc.widen(rows32), pad=pad)
        a.sc()
        b.sc()
        oa, ob = a.read(), b.read()
    assert_sc(oa, bits, ok, tag)
    assert_same(oa, ob, tag)
    return oa


def decode_both(dec, rows32, exp, tag, sl=slice(None), offset=0, pad=0):
    """decode_device_f32 against the oracle's list decode and against decode_device on the widened
    rows; returns (outputs, deferred-frame count of the float32 call)."""
    with _native.DeviceArena(dec) as mem:
        a, b = Batch(dec, mem, rows32, offset=offset, pad=pad), Batch(dec, mem, fc.widen(rows32), pad=pad)
        a.decode()
        oa, na = a.read(), dec.screening_count()
        b.decode()
        ob, nb = b.read(), dec.screening_count()
    assert_list(oa, exp, tag, sl)
    assert_same(oa, ob, tag, ("words", "flags"))
    assert na == nb, (tag, "deferred-frame count", na, nb)
    return oa, na


def adaptive_both(dec, rows32, exp, tag, sl=slice(None), pad=0, path="screened"):
    dec.adaptive_stats(reset=True)
    with _native.DeviceArena(dec) as mem:
        a, b = Batch(dec, mem, rows32, pad=pad), Batch(dec, mem, fc.widen(rows32), pad=pad)
        a.adaptive()
        oa = a.read()
        st = dec.adaptive_stats()
        b.adaptive()
        ob = b.read()
    ac.assert_equals(oa, exp, tag, sl)
    assert oa["n_escalated"] == int(np.count_nonzero(exp["stage"][sl] == 2)) == ob["n_escalated"], tag
    assert_same(oa, ob, tag)
    other = "exact" if path == "screened" else "screened"
    assert st[path] == 1 and st[other] == 0, (tag, st)
    return oa


@pytest.fixture(scope="module")
def dec8():
    return _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)


@pytest.fixture(scope="module")
def dec4():
    return _native.Decoder(128, ac.info_set(128, 64), 4, ac.POLY24)


def _nr(L, E):
    dec = _native.Decoder(128, ac.info_set(128, 88), L, ac.POLY24)
    dec.set_rate_match(E)
    return dec


def test_covered_handles_report_native_kernels(dec8, dec4):
    assert dec8.f32_available() and dec4.f32_available() and _nr(8, 256).f32_available() and _nr(4, 201).f32_available()


# ---- 1. the SC stage

def test_sc_mixed_batch(dec8):
    rows, exp = fc.mixed_rows(), fc.mixed_expected(8)
    assert rows.dtype == np.float32 and len(rows) == 4099
    assert 1 <= exp["n_escalated"] <= len(rows) - 1 and 900 < exp["n_escalated"] < 1200  # (about a quarter at 5 dB)
    sc_both(dec8, rows, exp["sc_bits"], exp["sc_ok"], "mixed")


@pytest.mark.parametrize("B", [1, 15, 16, 17, 63, 65])
def test_sc_prefixes_over_sentinel_outputs(B, dec8):
    exp = fc.mixed_expected(8)
    sc_both(dec8, np.ascontiguousarray(fc.mixed_rows()[:B]), exp["sc_bits"][:B], exp["sc_ok"][:B], f"B={B}", pad=48)


@pytest.mark.parametrize("name", [n for n, _ in ac.block_family()])
def test_sc_every_branch_state(name):
    """The 14 block information sets reach all 381 branch states of the SC tree; raw Gaussian rows and
    rows shifted by a codeword (on which SC decides non-zero CRC-valid words)."""
    case = fc.family_rows(name)
    assert len(ac.block_family()) == 14  # (that they reach all 381 states: tests/test_adaptive_cpu.py)
    dec = _native.Decoder(128, case["info"], 4, ac.POLY24)
    for k in ("raw", "shifted"):
        rows, bits, ok = case[k]
        assert len(rows) == 259
        sc_both(dec, rows, bits, ok, f"{name} {k}")
    assert case["shifted"][1].any() and case["shifted"][2].mean() > 0.9  # (the shift survives the rounding)


def _frames_per_grid_pass():
    src = (Path(_native.__file__).resolve().parent / "csrc" / "sc128_lane.hip").read_text()

    def ints(pattern, what):
        m = re.search(pattern, src, re.S)
        assert m, f"sc128_lane.hip: {what} not found; update the pattern with the kernel"
        return [int(g) for g in m.groups()]

    cap, cap2 = ints(r"int64_t pscl_sc_lane_grid\([^{]*\{.*?if \(grid > (\d+)\) grid = (\d+);", "the SC grid cap")
    (fpw,) = ints(r"constexpr int kFramesPerWave = (\d+);", "frames per wavefront")
    _, w_plain = ints(r"constexpr int wavesPerWg\(bool rm\) \{ return rm \? (\d+) : (\d+); \}", "wavefronts per workgroup")
    assert cap == cap2
    # (the float32 launch takes the float64 launch's grid)
    assert re.search(r"pscl_launch_sc_lane_f32\([^{]*\{.*?pscl_sc_lane_grid\(P\)", src, re.S)
    return cap * fpw * w_plain


def test_sc_past_the_grid_cap(dec8):
    """33 x 4099 frames: more than one pass of the capped grid (few distinct rows, tiled)."""
    reps = 33
    rows, exp = fc.mixed_rows(), fc.mixed_expected(8)
    B = reps * len(rows)
    assert B > _frames_per_grid_pass(), (B, _frames_per_grid_pass())
    with _native.DeviceArena(dec8) as mem:
        a = Batch(dec8, mem, np.ascontiguousarray(np.tile(rows, (reps, 1))))
        a.sc()
        out = a.read()
    assert_sc(out, np.tile(exp["sc_bits"], (reps, 1)), np.tile(exp["sc_ok"], reps), "two grid passes")


# ---- 2. rate-matched rows: E = 256 (means of two), 100 (E <= N, padding), odd 201 and 255 (rows on
# 4-byte boundaries), d_llr a view 4 bytes into its allocation

@pytest.mark.parametrize("E", [256, 100, 201, 255])
def test_rate_matched_sc(E):
    rows, exp = fc.nr_rows(E), fc.nr_expected(E, 8)
    assert rows.shape == (263, E) and rows.dtype == np.float32
    sc_both(_nr(8, E), rows, exp["sc_bits"], exp["sc_ok"], f"NR SC E={E}", offset=4, pad=5)


@pytest.mark.parametrize("L", [8, 4])
@pytest.mark.parametrize("E", [256, 100, 201, 255])
def test_rate_matched_list_decode(E, L):
    dec = _nr(L, E)
    assert dec.f32_available()
    decode_both(dec, fc.nr_rows(E), fc.nr_expected(E, L), f"NR list E={E} L={L}", offset=4, pad=5)


@pytest.mark.parametrize("L", [8, 4])
@pytest.mark.parametrize("E", [256, 201])
def test_rate_matched_adaptive(E, L):
    exp = fc.nr_expected(E, L)
    assert 0 < exp["n_escalated"] < 263
    adaptive_both(_nr(L, E), fc.nr_rows(E), exp, f"NR adaptive E={E} L={L}", pad=5)


# ---- 3. exact-arithmetic corners

def test_corners_sc(dec8):
    rows, s0 = fc.corner_rows()
    bits, ok = sg.sc_expected(fc.widen(rows), ac.info_set(128, 64), ac.POLY24)
    assert bits[:5].sum() == 0 and bits[5:53].any()
    # the subnormal rows carry a codeword's signs: their SC result is not all zero, as it would be flushed
    assert bits[s0:s0 + 32].any(axis=1).all()
    sc_both(dec8, rows, bits, ok, "corners")


@pytest.mark.parametrize("L", [8, 4])
def test_corners_list_decode(L, dec8, dec4):
    rows, _ = fc.corner_rows()
    exp = ac.compose(fc.widen(rows), ac.info_set(128, 64), L, ac.POLY24)
    _, deferred = decode_both(dec8 if L == 8 else dec4, rows, exp, f"corners L={L}")
    assert deferred > 0  # (ties and the 3e38 rows go to the exact float32 re-decode)


# ---- 4. the plain list decode

@pytest.mark.parametrize("L", [8, 4])
def test_list_mixed_batch(L, dec8, dec4):
    decode_both(dec8 if L == 8 else dec4, fc.mixed_rows(), fc.mixed_expected(L), f"mixed L={L}")


@pytest.mark.parametrize("L", [8, 4])
@pytest.mark.parametrize("B", [1, 7, 9, 15, 17, 130])
def test_list_prefixes_over_sentinel_outputs(B, L, dec8, dec4):
    decode_both(dec8 if L == 8 else dec4, np.ascontiguousarray(fc.mixed_rows()[:B]), fc.mixed_expected(L), f"B={B} L={L}",
                slice(0, B), pad=40)


@pytest.mark.parametrize("L", [8, 4])
@pytest.mark.parametrize("B", [1, 7, 9, 15, 17, 130])
def test_list_prefixes_nr_code_odd_E(B, L):
    """The same prefixes on the NR (128,88) code, rows of E = 201 floats from a pointer 4 bytes into its
    allocation: ragged wavefronts of the code-2 float32 instances (8 and 16 frames per wavefront)."""
    decode_both(_nr(L, 201), np.ascontiguousarray(fc.nr_rows(201)[:B]), fc.nr_expected(201, L), f"NR E=201 B={B} L={L}",
                slice(0, B), offset=4, pad=40)


@pytest.mark.parametrize("L", [8, 4])
def test_list_deferred_ties_take_the_f32_exact_redecode(L, dec8, dec4):
    rows, exps = fc.tie_case()
    _, deferred = decode_both(dec8 if L == 8 else dec4, rows, exps[L], f"ties L={L}", pad=9)
    assert deferred > 0


@pytest.mark.parametrize("nr", [False, True])
@pytest.mark.parametrize("L", [8, 4])
def test_list_counters_with_reference(L, nr, dec8, dec4):
    if nr:
        dec, rows, exp, kp = _nr(L, 256), fc.nr_rows(256), fc.nr_expected(256, L), 64
    else:
        dec, rows, exp, kp = (dec8 if L == 8 else dec4), fc.mixed_rows()[:1500], fc.mixed_expected(L), 40
    B = len(rows)
    lb, lok = exp["list_bits"][:B], exp["list_ok"][:B]
    ref = lb ^ (np.random.default_rng(97).random(lb.shape) < 0.01).astype(np.int8)
    want = sg.host_counts(lb, lok, ref, kp, NC)
    with _native.DeviceArena(dec) as mem:
        a, b = Batch(dec, mem, np.ascontiguousarray(rows), ref_bits=ref), Batch(dec, mem, fc.widen(rows), ref_bits=ref)
        a.decode(kp)
        b.decode(kp)
        oa, ob = a.read(), b.read()
    np.testing.assert_array_equal(oa["counters"], want)
    np.testing.assert_array_equal(oa["counters"], ob["counters"])


# ---- 5. pscl_adaptive_async_device_f32

@pytest.mark.parametrize("L", [8, 4])
def test_adaptive_mixed_batch(L, dec8, dec4):
    adaptive_both(dec8 if L == 8 else dec4, fc.mixed_rows(), fc.mixed_expected(L), f"adaptive mixed L={L}", pad=3)


def test_adaptive_no_frame_escalates(dec8):
    rows, exp = fc.allpass_case()
    assert exp["n_escalated"] == 0
    out = adaptive_both(dec8, rows, exp, "all pass")
    assert out["n_escalated"] == 0 and np.all(out["stage"] == 1)


def test_adaptive_every_frame_escalates(dec8):
    rows, exp = fc.allfail_case()
    assert exp["n_escalated"] == len(rows)
    out = adaptive_both(dec8, rows, exp, "all fail")
    assert_list(out, exp, "all fail")


@pytest.mark.parametrize("L", [8, 4])
def test_adaptive_ragged_escalated_count(L, dec8, dec4):
    exp = fc.mixed_expected(L)
    B = next(b for b in range(2000, 4099) if np.count_nonzero(exp["stage"][:b] == 2) % 16 not in (0, 8))
    n = int(np.count_nonzero(exp["stage"][:B] == 2))
    assert n % (64 // L) != 0 and n > 64
    out = adaptive_both(dec8 if L == 8 else dec4, np.ascontiguousarray(fc.mixed_rows()[:B]), exp, f"ragged {n} L={L}", slice(0, B))
    assert out["n_escalated"] == n


@pytest.mark.parametrize("L", [8, 4])
def test_adaptive_deferred_ties_are_listed_by_row(L, dec8, dec4):
    rows, exps = fc.tie_case()
    dec = dec8 if L == 8 else dec4
    assert exps[L]["n_escalated"] > 100
    adaptive_both(dec, rows, exps[L], f"adaptive ties L={L}", pad=7)
    with _native.DeviceArena(dec) as mem:
        a = Batch(dec, mem, rows)
        a.adaptive()
        a.read()
        assert dec.screening_count() > 0  # (the float32 exact re-decode ran)


def test_adaptive_counters_and_device_count(dec8):
    rows, exp, kp = fc.mixed_rows(), fc.mixed_expected(8), 40
    ref = exp["list_bits"] ^ (np.random.default_rng(99).random(exp["list_bits"].shape) < 0.01).astype(np.int8)
    want = sg.host_counts(exp["best_bits"], exp["crc_pass"], ref, kp, NC, escalated=exp["n_escalated"])
    with _native.DeviceArena(dec8) as mem:
        a, b, c = Batch(dec8, mem, rows, ref_bits=ref), Batch(dec8, mem, fc.widen(rows), ref_bits=ref), Batch(dec8, mem, rows)
        a.adaptive(kp)
        b.adaptive(kp)
        c.adaptive()
        oa, ob, oc = a.read(), b.read(), c.read()
    np.testing.assert_array_equal(oa["counters"], want)
    assert want[_native.CNT_ESCALATED] == exp["n_escalated"] == oa["n_escalated"] == oc["n_escalated"]
    np.testing.assert_array_equal(oa["counters"], ob["counters"])
    np.testing.assert_array_equal(oc["counters"], np.zeros(NC, np.int64))  # (untouched without d_ref)


@pytest.mark.parametrize("cap", [16, 1])
def test_adaptive_capped_grid_strides_over_the_list(cap):
    rows, exp = fc.allfail_case()
    rows, B = np.ascontiguousarray(rows[:300]), 300
    dec = _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    dec.set_tuning(adapt_grid=cap)
    assert B > cap * 8  # (8 frames per workgroup at L = 8: more than one pass)
    adaptive_both(dec, rows, exp, f"{cap} workgroups", slice(0, B))


def _five_calls():
    (r2, e2), (r3, e3) = fc.allfail_case(), fc.allpass_case()
    t, te = fc.tie_case()
    m, me = fc.mixed_rows(), fc.mixed_expected(8)
    return [(m, me), (r2, e2), (t, te[8]), (r3, e3), (np.ascontiguousarray(m[:1500]), {k: (v[:1500] if isinstance(v, np.ndarray) else v) for k, v in me.items()})]


def _run_five(dec, mem, calls, kp, pipelined, depth=1):
    """Five calls whose outputs alternate between two buffer sets; the counters add up in one buffer.
    Returns the two sets' final contents (calls 3 and 4... the last writer of each) and the counters."""
    W, bmax = dec.W, max(len(r) for r, _ in calls)
    sets = [dict(best=mem.alloc(bmax * W * 8), flags=mem.alloc(bmax), stage=mem.alloc(bmax), n=mem.alloc(8)) for _ in range(2)]
    for s in sets:
        for k, size in (("best", bmax * W * 8), ("flags", bmax), ("stage", bmax), ("n", 8)):
            mem.memset(s[k], SENTINEL, size)
    d_cnt = mem.alloc(8 * NC)
    mem.memset(d_cnt, 0, 8 * NC)
    ins = []
    for r, e in calls:
        d_llr, d_ref = mem.alloc(r.nbytes), mem.alloc(len(r) * W * 8)
        mem.upload(d_llr, r)
        mem.upload(d_ref, sg.words(e["list_bits"][:len(r)]))
        ins.append((d_llr, d_ref))
    if pipelined:
        dec.set_pipelined(True, depth=depth)
    try:
        for i, ((r, _), (d_llr, d_ref)) in enumerate(zip(calls, ins)):
            s = sets[i & 1]
            f = dec.adaptive_async_device_f32 if r.dtype == np.float32 else dec.adaptive_async_device
            f(d_llr, len(r), d_best=s["best"], d_flags=s["flags"], d_stage=s["stage"], d_ref=d_ref, k_payload=kp,
              d_counters=d_cnt, d_n_escalated=s["n"])
        if pipelined:
            dec.join()
        dec.sync()
    finally:
        if pipelined:
            dec.set_pipelined(False)
    out = [{k: mem.download(s[k], size, np.uint8) for k, size in (("best", bmax * W * 8), ("flags", bmax), ("stage", bmax), ("n", 8))}
           for s in sets]
    return out, mem.download(d_cnt, 8 * NC, np.int64)


@pytest.mark.parametrize("depth", [1, 2])
def test_adaptive_pipelined_equals_stream_ordered(depth, dec8):
    calls, kp = _five_calls(), 40
    want = sum(sg.host_counts(e["best_bits"][:len(r)], e["crc_pass"][:len(r)], e["list_bits"][:len(r)], kp, NC,
                              escalated=int(np.count_nonzero(e["stage"][:len(r)] == 2))) for r, e in calls)
    with _native.DeviceArena(dec8) as mem:
        plain, cnt_plain = _run_five(dec8, mem, calls, kp, False)
        piped, cnt_piped = _run_five(dec8, mem, calls, kp, True, depth)
    np.testing.assert_array_equal(cnt_plain, want)  # (the oracle's, over all five calls)
    np.testing.assert_array_equal(cnt_piped, want)
    for a, b in zip(plain, piped):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # the sets hold the last writers' outputs: call 4 (set 0) and call 3 (set 1), over call 2's longer batch
    for s, i in ((0, 4), (1, 3)):
        r, e = calls[i]
        B = len(r)
        words = piped[s]["best"].view(np.uint64)[:B].reshape(B, 1)
        np.testing.assert_array_equal(_bits(words, 64), e["best_bits"][:B])
        np.testing.assert_array_equal(piped[s]["stage"][:B], e["stage"][:B])
        assert int(piped[s]["n"].view(np.int32)[0]) == int(np.count_nonzero(e["stage"][:B] == 2))


@pytest.mark.parametrize("first", ["f32", "f64"])
def test_dtype_does_not_leak_between_pipelined_calls(first, dec8):
    """A float64 call directly after a float32 call on a pipelined handle, and the reverse, through the
    adaptive call and through the plain decode: both batches hold rows the screening pass defers, so
    each call leaves an exact re-decode on a side stream that must read its own call's row type."""
    t32, te = fc.tie_case()
    m32, me = np.ascontiguousarray(fc.mixed_rows()[:1500]), fc.mixed_expected(8)
    # the two batches differ, and so do their types: (ties, mixed) typed (first, other)
    a_rows, b_rows = (t32, fc.widen(m32)) if first == "f32" else (fc.widen(t32), m32)
    with _native.DeviceArena(dec8) as mem:
        dec8.set_pipelined(True)
        try:
            ad = [Batch(dec8, mem, r) for r in (a_rows, b_rows, a_rows, b_rows)]
            for b in ad:
                b.adaptive()
            dec8.join()
            dec8.sync()
            pl = [Batch(dec8, mem, r) for r in (a_rows, b_rows, a_rows, b_rows)]
            for b in pl:
                b.decode()
            dec8.join()
            dec8.sync()
        finally:
            dec8.set_pipelined(False)
        for i, b in enumerate(ad):
            exp, sl = (te[8], slice(None)) if i % 2 == 0 else (me, slice(0, 1500))
            out = b.read()
            ac.assert_equals(out, exp, f"adaptive call {i} ({first} first)", sl)
            assert out["n_escalated"] == int(np.count_nonzero(exp["stage"][sl] == 2))
        for i, b in enumerate(pl):
            exp, sl = (te[8], slice(None)) if i % 2 == 0 else (me, slice(0, 1500))
            assert_list(b.read(), exp, f"plain call {i} ({first} first)", sl)


# ---- 6. pscl_escalate_device_f32 after pscl_sc_device_f32

@pytest.mark.parametrize("L", [8, 4])
def test_escalate_after_sc_equals_the_async_call(L, dec8, dec4):
    dec, rows, exp = (dec8 if L == 8 else dec4), fc.mixed_rows(), fc.mixed_expected(L)
    with _native.DeviceArena(dec) as mem:
        a, b = Batch(dec, mem, rows), Batch(dec, mem, rows)
        a.adaptive()
        b.sc()
        n = b.escalate()
        oa, ob = a.read(), b.read()
    ac.assert_equals(ob, exp, f"staged L={L}")
    assert n == exp["n_escalated"] == oa["n_escalated"]
    assert_same(ob, oa, f"staged L={L}")


def test_escalate_rate_matched_odd_E():
    dec, rows, exp = _nr(8, 201), fc.nr_rows(201), fc.nr_expected(201, 8)
    with _native.DeviceArena(dec) as mem:
        b = Batch(dec, mem, rows, offset=4)
        b.sc()
        n = b.escalate()
        ob = b.read()
    ac.assert_equals(ob, exp, "staged NR E=201")
    assert n == exp["n_escalated"] > 0


# ---- 7. refusals

def _refused_handles():
    info = ac.info_set(128, 64)
    off = _native.Decoder(128, info, 8, ac.POLY24)
    off.set_screening(False)
    knob = _native.Decoder(128, info, 8, ac.POLY24)
    knob.set_tuning(lane_exact=1)
    rm64 = _native.Decoder(128, info, 8, ac.POLY24)
    rm64.set_rate_match(256)  # (the (128,64) code on rate-matched rows: no lane-per-path kernel)
    return {"N=256": _native.Decoder(256, sg.pw_info_set(256, 128), 8, ac.POLY24),
            "L=2": _native.Decoder(128, info, 2, ac.POLY24),
            "L=16": _native.Decoder(128, info, 16, ac.POLY24),
            "(128,40)+CRC-16": _native.Decoder(128, ac.info_set(128, 40), 4, ac.POLY16),
            "screening off": off, "lane_exact knob": knob, "(128,64) rate matched": rm64}


@pytest.mark.parametrize("what", ["N=256", "L=2", "L=16", "(128,40)+CRC-16", "screening off", "lane_exact knob",
                                  "(128,64) rate matched"])
def test_refusals(what):
    dec = _refused_handles()[what]
    lib, h = _native.lib(), dec.handle
    assert not dec.f32_available() and lib.pscl_f32_available(h) == 0
    row = dec.E or dec.N
    with _native.DeviceArena(dec) as mem:
        d_llr, d_best, d_flags, d_stage = mem.alloc(4 * row * 4), mem.alloc(4 * dec.W * 8), mem.alloc(8), mem.alloc(8)
        mem.memset(d_llr, 0, 4 * row * 4)
        assert lib.pscl_decode_device_f32(h, d_llr, 4, d_best, d_flags, None, 0, None) == EUNSUP
        assert lib.pscl_last_error()  # (names the reason)
        msg = lib.pscl_last_error().decode()
        assert lib.pscl_escalate_device_f32(h, d_llr, 4, d_best, d_flags, d_stage, None, 0, None, None) == EUNSUP
        assert lib.pscl_adaptive_async_device_f32(h, d_llr, 4, d_best, d_flags, d_stage, None, 0, None, None) == EUNSUP
        assert lib.pscl_sc_device_f32(h, d_llr, 4, d_best, d_flags, d_stage, None, 0, None) == (EUNSUP if dec.N != 128 else 0)
        dec.sync()
    key = {"N=256": "N = 128", "L=2": "L = 4 and 8", "L=16": "L = 4 and 8", "(128,40)+CRC-16": "information set",
           "screening off": "screening", "lane_exact knob": "PSCL_TUNE_LANE_EXACT", "(128,64) rate matched": "(128,88)"}[what]
    assert key in msg, msg


def test_argument_errors_match_the_float64_calls(dec8):
    lib, h = _native.lib(), dec8.handle
    p = 4096  # (any non-NULL value: the argument checks come before any launch)
    for f64, f32, tail in ((lib.pscl_sc_device, lib.pscl_sc_device_f32, ()), (lib.pscl_escalate_device, lib.pscl_escalate_device_f32, (None,)),
                           (lib.pscl_adaptive_async_device, lib.pscl_adaptive_async_device_f32, (None,))):
        for args in ((h, p, -1, p, p, None, None, 0, None), (h, None, 4, p, p, None, None, 0, None), (h, p, 4, None, p, None, None, 0, None),
                     (h, p, 4, p, None, None, None, 0, None), (h, p, 4, p, p, None, p, 0, None), (h, p, 4, p, p, None, None, 65, None)):
            assert f64(*args, *tail) == f32(*args, *tail) == EINVAL, args
        assert f64(h, None, 0, None, None, None, None, 0, None, *tail) == f32(h, None, 0, None, None, None, None, 0, None, *tail) == 0
    for args32 in ((h, p, -1, p, p, None, 0, None), (h, None, 4, p, p, None, 0, None), (h, p, 4, p, p, p, 0, None), (h, p, 4, p, p, None, 65, None)):
        args64 = args32[:3] + (None,) + args32[3:5] + (None, None, None) + args32[5:]
        assert lib.pscl_decode_device(*args64) == lib.pscl_decode_device_f32(*args32) == EINVAL, args32
    assert lib.pscl_decode_device_f32(h, None, 0, None, None, None, 0, None) == 0
    nocrc = _native.Decoder(128, ac.info_set(128, 64), 8, None)
    assert lib.pscl_adaptive_async_device_f32(nocrc.handle, p, 4, p, p, None, None, 0, None, None) == EINVAL
    assert lib.pscl_escalate_device_f32(nocrc.handle, p, 4, p, p, None, None, 0, None, None) == EINVAL


def _widening_case(what):
    """(N, info, L, crc, float32 rows) of a handle without float32 list kernels."""
    info64 = ac.info_set(128, 64)
    if what == "N=256":
        return 256, sg.pw_info_set(256, 128), 8, ac.POLY24, fc.f32(sg.mixed_rows("pw256"))
    if what == "(128,40)+CRC-16":
        info = ac.info_set(128, 40)
        return 128, info, 4, ac.POLY16, fc.f32(ac.make_llr(78, 300, info, ac.POLY16, 3.0))
    L = {"L=2": 2, "L=16": 16, "screening off": 8}[what]
    return 128, info64, L, ac.POLY24, np.ascontiguousarray(fc.mixed_rows()[:300])


@pytest.mark.parametrize("what", ["N=256", "L=2", "L=16", "(128,40)+CRC-16", "screening off"])
def test_torch_methods_widen_where_there_is_no_native_kernel(what):
    """The refused handles through the torch methods: float32 tensors give the float64 path's results --
    the oracle's on the widened rows, and the same tensors as the float64 call.  N = 256 is the one
    handle on which decode_tensor_sc widens too (pscl_sc_device_f32 takes N = 128 only)."""
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    N, info, L, crc, rows32 = _widening_case(what)
    K = len(info)
    exp = ac.compose(fc.widen(rows32), info, L, crc, N=N)
    assert 0 < exp["n_escalated"] < len(rows32)
    dec = SCLDecoder(N, info, L, crc)
    if what == "screening off":
        dec.native.set_screening(False)
    assert not dec.native.f32_available()
    methods = ("decode_tensor", "decode_tensor_sc", "decode_tensor_adaptive_async", "decode_tensor_staged")
    stream = torch.cuda.Stream()  # (the handle runs on the caller's stream: the tensors' producer and consumer)
    with torch.cuda.stream(stream):
        llr = torch.from_numpy(rows32.copy()).to("cuda")
        wide = llr.double()
        got = {m: getattr(dec, m)(llr) for m in methods}
        ref = {m: getattr(dec, m)(wide) for m in methods}
    stream.synchronize()
    for m in methods:
        for a, b in zip(got[m], ref[m]):
            assert torch.equal(a, b), (what, m, "differs from the float64 call")
    want = {"decode_tensor": (exp["list_bits"], exp["list_ok"], None),
            "decode_tensor_sc": (exp["sc_bits"], exp["sc_ok"], np.where(exp["sc_ok"], 1, 2)),
            "decode_tensor_adaptive_async": (exp["best_bits"], exp["crc_pass"], exp["stage"]),
            "decode_tensor_staged": (exp["best_bits"], exp["crc_pass"], exp["stage"])}
    for m, (bits, ok, stage) in want.items():
        out = got[m]
        np.testing.assert_array_equal(_bits(out[0].cpu().numpy().view(np.uint64), K), bits, err_msg=f"{what} {m}: bits")
        np.testing.assert_array_equal((out[1].cpu().numpy() & PASS) != 0, ok, err_msg=f"{what} {m}: pass flag")
        if stage is not None:
            np.testing.assert_array_equal(out[2].cpu().numpy(), stage, err_msg=f"{what} {m}: stage")
    assert int(got["decode_tensor_adaptive_async"][3].cpu()[0]) == exp["n_escalated"]
    dec.native.set_stream(None)


# ---- 8. the torch methods on a side stream

def test_tensor_methods_on_a_side_stream():
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    rows32, exp = np.ascontiguousarray(fc.mixed_rows()[:1500]), fc.mixed_expected(8)
    dec = SCLDecoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    assert dec.native.f32_available()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        llr = torch.from_numpy(rows32.copy()).to("cuda")
        assert llr.dtype == torch.float32
        best, flags, stage, n_esc = dec.decode_tensor_adaptive_async(llr)
        sb, sf, ss = dec.decode_tensor_staged(llr)
        cb, cf, cs = dec.decode_tensor_sc(llr)
        lb, lf = dec.decode_tensor(llr)
    stream.synchronize()
    sl = slice(0, 1500)
    for tag, (w, f, s) in (("async", (best, flags, stage)), ("staged", (sb, sf, ss))):
        f = f.cpu().numpy()
        np.testing.assert_array_equal(w.cpu().numpy().view(np.uint64), sg.words(exp["best_bits"][sl]), err_msg=tag)
        np.testing.assert_array_equal((f & PASS) != 0, exp["crc_pass"][sl], err_msg=tag)
        np.testing.assert_array_equal(f & IDX, exp["best_idx"][sl], err_msg=tag)
        np.testing.assert_array_equal(s.cpu().numpy(), exp["stage"][sl], err_msg=tag)
    assert n_esc.dtype == torch.int32 and int(n_esc.cpu()[0]) == int(np.count_nonzero(exp["stage"][sl] == 2))
    np.testing.assert_array_equal(cb.cpu().numpy().view(np.uint64), sg.words(exp["sc_bits"][sl]))
    np.testing.assert_array_equal((cf.cpu().numpy() & PASS) != 0, exp["sc_ok"][sl])
    np.testing.assert_array_equal(cs.cpu().numpy(), np.where(exp["sc_ok"][sl], 1, 2))
    lf = lf.cpu().numpy()
    np.testing.assert_array_equal(lb.cpu().numpy().view(np.uint64), sg.words(exp["list_bits"][sl]))
    np.testing.assert_array_equal((lf & PASS) != 0, exp["list_ok"][sl])
    np.testing.assert_array_equal(lf & IDX, exp["list_idx"][sl])
    dec.native.set_stream(None)
