"""GPU: every screening decoder, and the exact kernels behind them, on metric gaps inside the ordering
margin (near_tie_cases.py).

The screening kernels (scl128_lane.hip, scl_lane_long.hip, the APX instances of scl128_impl.h, their
float32, row-list and forced-bit instances) rank paths on metrics with an fp32 tail and are bit-exact only
because every ordering must clear MARGIN = 2 N DELTA, else the frame goes to the exact kernel.  AWGN rows
never come that close, and integer rows tie exactly (identical approximate keys), so neither shows a tier
that lost its margin.  These rows are integer rows with every tie opened by d = 1e-12 .. 1e-8 (INSIDE the
margin and below the tail's own error) or 1e-7 .. 1e-3 (STRADDLE: either side of the margin); the
un-margined model of test_near_tie_cpu.py is wrong on 12 % .. 99 % of the INSIDE frames of every case.
What this does and does not pin (a build with MARGIN = 0.0 still passes: the certificate's high-word keys
defer these rows by themselves) is in DESIGN.md section 5.2.

Every assertion is bit for bit, on every frame, against the exact oracle alone."""
import numpy as np
import pytest

import adaptive_cases as ac
import dl_short_cases as ds
import near_tie_cases as nt
from polar_code_amd import _native
from polar_code_amd.dlscl.flip import decode_with_retries_batch, decode_with_retries_device

pytestmark = pytest.mark.gpu

PLAIN = ("best_bits", "crc_pass", "best_idx", "n_paths")
PASS, IDX = _native.PSCL_FLAG_CRC_PASS, _native.PSCL_FLAG_IDX_MASK


def _decoder(c, screening=True, **tuning):
    dec = _native.Decoder(c.N, nt.info_of(c), c.L, nt.POLY)
    if c.E:
        dec.set_rate_match(c.E)
    if not screening:
        dec.set_screening(False)
    if tuning:
        dec.set_tuning(**tuning)
    return dec


def _plain(dec, rows):
    return dec.decode(rows, want_metrics=False, want_cands=False, want_info_llrs=False)


def _assert_plain(out, exp, tag, keys=PLAIN):
    for k in keys:
        np.testing.assert_array_equal(np.asarray(out[k]), exp[k], err_msg=f"{tag}: {k}")


def _bits(words, K):
    j = np.arange(K)
    return ((words[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)


# ---- 1. plain decodes: screening on == screening off == the oracle, every case

@pytest.mark.parametrize("name", nt.NAMES)
def test_plain_decode_screened_equals_exact_equals_oracle(name):
    c = nt.case(name)
    scr, ex = _decoder(c), _decoder(c, screening=False)
    for cls in ("inside", "straddle"):
        rows, exp = nt.rows_of(name, cls), nt.expected(name, cls)
        a = _plain(scr, rows)
        n_def = scr.screening_count()
        b = _plain(ex, rows)
        print(f"near-tie {name} {cls}: n_def / B = {n_def} / {c.B} = {n_def / c.B:.3f}")
        _assert_plain(a, exp, f"{name} {cls} screened")
        _assert_plain(b, exp, f"{name} {cls} exact")
        assert ex.screening_count() == 0
        if cls == "inside":
            assert n_def > 0, name  # (the screening pass ran and handed frames over)
    scr.close()
    ex.close()


# ---- 2. the exact kernels on the same rows: full outputs against oracle.decode_scl, every frame

def _assert_full(out, full, tag, info_llrs=True):
    n, cands, mets, illr, best = full
    L = cands.shape[1]
    assert np.all(n == L), tag  # (every list is full: all L entries are compared)
    np.testing.assert_array_equal(out["n_paths"], n, err_msg=tag)
    np.testing.assert_array_equal(out["cands"], cands, err_msg=f"{tag}: candidates / list order")
    np.testing.assert_array_equal(out["metrics"].view(np.int64), mets.view(np.int64), err_msg=f"{tag}: metrics")
    if info_llrs:
        np.testing.assert_array_equal(out["info_llrs"].view(np.int64), illr.view(np.int64), err_msg=f"{tag}: decision LLRs")
    np.testing.assert_array_equal(out["best_idx"], best, err_msg=tag)
    np.testing.assert_array_equal(out["best_bits"], cands[np.arange(len(n)), best], err_msg=tag)


@pytest.mark.parametrize("cls", ["inside", "straddle"])
@pytest.mark.parametrize("name", [nt.GENERIC64.name, "n128k64_L2", "n128k64_L8", "n128k88e256_L4", "n256k128_L8",
                                  "n1024k512_L4"])
def test_exact_kernels_full_outputs(name, cls):
    """One case per exact kernel family.  With decision LLRs: the decision-history kernels (the generic
    scl_kernels.hip at N = 64 and 128, scl_long.hip at N = 256 and 1024).  Without: the compiled-code
    `spec` instances at N = 128 ((128,64) plain, (128,88) rate matched) and the long kernel's plain form."""
    c = nt.case(name)
    rows, full = nt.rows_of(name, cls), nt.full_expected(name, cls)
    dec = _decoder(c)
    _assert_full(dec.decode(rows), full, f"{name} {cls} with history")
    _assert_full(dec.decode(rows, want_info_llrs=False), full, f"{name} {cls} without history", info_llrs=False)
    dec.close()


@pytest.mark.parametrize("lane_exact", [1, 2, 3])
@pytest.mark.parametrize("name", ["n128k64_L4", "n128k64_L8"])
def test_lane_exact_instances(name, lane_exact):
    """PSCL_TUNE_LANE_EXACT: the deferred frames' re-decode on the exact lane-per-path kernel (1) or the
    two-lanes-per-path one (2), and every frame on the former, unscreened (3).  Those kernels write best
    bits, CRC flag, best index and path count only: all of them, on every frame."""
    c = nt.case(name)
    dec = _decoder(c, lane_exact=lane_exact)
    for cls in ("inside", "straddle"):
        out = _plain(dec, nt.rows_of(name, cls))
        n_def = dec.screening_count()
        _assert_plain(out, nt.expected(name, cls), f"{name} {cls} lane_exact={lane_exact}")
        assert (n_def == 0) if lane_exact == 3 else (cls != "inside" or n_def > 0)
    launches = dec.path_stats()["lane_exact_launches"]
    assert (launches == 0) if lane_exact == 2 else (launches > 0)
    dec.close()


# ---- 3. float32 rows

def _device_plain(dec, rows, f32):
    B, W = len(rows), dec.W
    with _native.DeviceArena(dec) as mem:
        d_llr, d_best, d_flags = mem.alloc(rows.nbytes), mem.alloc(B * W * 8), mem.alloc(B)
        mem.upload(d_llr, rows)
        mem.memset(d_best, 0x5A, B * W * 8)
        mem.memset(d_flags, 0x5A, B)
        (dec.decode_device_f32 if f32 else dec.decode_device)(d_llr, B, d_best=d_best, d_flags=d_flags)
        dec.sync()
        n_def = dec.screening_count()
        words, flags = mem.download(d_best, B * W * 8, np.uint64).reshape(B, W), mem.download(d_flags, B, np.uint8)
    return {"best_bits": _bits(words, dec.K), "crc_pass": (flags & PASS) != 0, "best_idx": (flags & IDX).astype(np.int32),
            "words": words, "flags": flags}, n_def


@pytest.mark.parametrize("name", ["n128k64_L4", "n128k64_L8", "n128k88e256_L4", "n128k88e256_L8"])
def test_float32_rows(name):
    """decode_device_f32 on (base + 1e-7 g).astype(float32) against the float64 decode of the widened
    rows (word for word) and the oracle on them."""
    c = nt.case(name)
    rows32, exp = nt.rows_of(name, "f32"), nt.expected(name, "f32")
    assert rows32.dtype == np.float32
    dec = _decoder(c)
    assert dec.f32_available()
    a, n32 = _device_plain(dec, rows32, True)
    b, n64 = _device_plain(dec, rows32.astype(np.float64), False)
    print(f"near-tie {name} f32: n_def / B = {n32} / {c.B} (float64 decode of the widened rows: {n64})")
    _assert_plain(a, exp, f"{name} float32", PLAIN[:3])
    _assert_plain(b, exp, f"{name} widened", PLAIN[:3])
    np.testing.assert_array_equal(a["words"], b["words"])
    np.testing.assert_array_equal(a["flags"], b["flags"])
    assert n32 > 0
    dec.close()


# ---- 4. adaptive and staged calls

def _buffers(dec, mem, rows):
    B = len(rows)
    d = dict(llr=mem.alloc(rows.nbytes), best=mem.alloc(B * dec.W * 8), flags=mem.alloc(B), stage=mem.alloc(B), n=mem.alloc(8))
    mem.upload(d["llr"], np.ascontiguousarray(rows, np.float64))
    mem.memset(d["best"], 0x5A, B * dec.W * 8)
    mem.memset(d["flags"], 0x5A, B)
    mem.memset(d["stage"], 0x5A, B)
    mem.memset(d["n"], 0xFF, 8)
    return d


def _read(dec, mem, d, B):
    words = mem.download(d["best"], B * dec.W * 8, np.uint64).reshape(B, dec.W)
    flags = mem.download(d["flags"], B, np.uint8)
    return {"best_bits": _bits(words, dec.K), "crc_pass": (flags & PASS) != 0, "best_idx": (flags & IDX).astype(np.int32),
            "stage": mem.download(d["stage"], B, np.uint8), "n_escalated": int(mem.download(d["n"], 8, np.int32)[0])}


def _reversed(exp):
    out = {k: exp[k][::-1] for k in ("best_bits", "crc_pass", "best_idx", "stage")}
    out["n_escalated"] = exp["n_escalated"]
    return out


def _adaptive_calls(dec, name):
    """adaptive_async_device stream ordered and pipelined (depth 2, two calls in flight), and sc_device +
    escalate_device, on INSIDE + STRADDLE rows against adaptive_cases.compose; every stage 2 on a row-list
    screening kernel (adaptive_stats)."""
    rows, exp = nt.both_rows(name), nt.composed(name)
    B = len(rows)
    assert exp["n_escalated"] > B // 2  # (integer-like rows mostly fail the SC stage's CRC: stage 2 sees them)
    back = np.ascontiguousarray(rows[::-1])
    with _native.DeviceArena(dec) as mem:
        dec.adaptive_stats(reset=True)
        d = _buffers(dec, mem, rows)
        dec.adaptive_async_device(d["llr"], B, d_best=d["best"], d_flags=d["flags"], d_stage=d["stage"], d_n_escalated=d["n"])
        dec.sync()
        out = _read(dec, mem, d, B)
        ac.assert_equals(out, exp, f"{name} stream ordered")
        assert out["n_escalated"] == exp["n_escalated"]
        assert dec.screening_count() > 0
        st = dec.adaptive_stats(reset=True)
        assert st["screened"] == 1 and st["exact"] == 0, st
        bufs = [_buffers(dec, mem, r) for r in (rows, back)]
        dec.set_pipelined(True, depth=2)
        try:
            for b in bufs:
                dec.adaptive_async_device(b["llr"], B, d_best=b["best"], d_flags=b["flags"], d_stage=b["stage"],
                                          d_n_escalated=b["n"])
            dec.join()
            dec.sync()
        finally:
            dec.set_pipelined(False)
        for b, e, tag in ((bufs[0], exp, "first"), (bufs[1], _reversed(exp), "second")):
            out = _read(dec, mem, b, B)
            ac.assert_equals(out, e, f"{name} pipelined, {tag} call")
            assert out["n_escalated"] == e["n_escalated"]
        st = dec.adaptive_stats(reset=True)
        assert st["screened"] == 2 and st["exact"] == 0, st
    out = dec.decode_staged(rows)  # sc_device, then escalate_device
    ac.assert_equals(out, exp, f"{name} escalate_device")
    assert out["n_escalated"] == exp["n_escalated"]
    assert dec.screening_count() > 0  # (its dense stage 2 is a screened plain decode)


@pytest.mark.parametrize("name", ["n128k64_L8", "n256k128_L8"])
def test_adaptive_calls(name):
    dec = _decoder(nt.case(name))
    _adaptive_calls(dec, name)
    dec.close()


def test_staged_rate_matched():
    """(256,128) through E = 300 with pscl_set_rate_match_staged: the de-rate-matching pass, then the plain
    rows' screening kernels -- the plain decode and the adaptive calls."""
    name = nt.RM256.name
    c = nt.case(name)
    dec = _decoder(c)
    dec.set_rate_match_staged(True)
    for cls in ("inside", "straddle"):  # (the mode is decode_device's, not the host-array decode's)
        out, n_def = _device_plain(dec, nt.rows_of(name, cls), False)
        print(f"near-tie {name} staged {cls}: n_def / B = {n_def} / {c.B} = {n_def / c.B:.3f}")
        _assert_plain(out, nt.expected(name, cls), f"{name} staged {cls}", PLAIN[:3])
        if cls == "inside":
            assert n_def > 0
    assert dec.rm_staged_stats(reset=True) == {"passes": 2, "rows": 2 * c.B}
    _adaptive_calls(dec, name)
    assert dec.rm_staged_stats()["passes"] > 0
    dec.close()


# ---- 5. forced-bit instances: the DL-SCL retry rounds

TUNINGS = ({"dl_screen": 1}, {"dl_screen": 1, "dl_retry_lane": 2}, {"dl_lane": 2}, {"dl_screen": 1, "dl_fused_post": 1})


@pytest.mark.parametrize("with_beta", [False, True], ids=["none", "beta"])
@pytest.mark.parametrize("name", ["n128k64_L4", "n128k64_L8"])
def test_forced_bit_retries(name, with_beta):
    """decode_with_retries_device (4 retries) under the schedules that put the retry decodes on the
    forced-bit screening instances (lane-per-path, two-lanes-per-path, fused post pass) and the baseline on
    the two-lanes-per-path screening kernel: bits, success, attempts, tried order and the baseline against
    oracle.decode_with_retries on every frame, and the host-ranked loop too."""
    c = nt.case(name)
    rows, exp = nt.both_rows(name), nt.dl_expected(name, with_beta)
    beta = nt.dl_beta(c.K, c.L) if with_beta else None
    assert float((exp["attempts"] > 1).mean()) >= 0.25
    for tuning in TUNINGS:
        dev = decode_with_retries_device(rows, nt.info_of(c), c.L, nt.DL_RETRIES, crc=nt.POLY, beta=beta, tuning=tuning)
        ds.assert_equals(dev, exp, f"{name} {tuning}")
    host = decode_with_retries_batch(rows, nt.info_of(c), c.L, nt.DL_RETRIES, crc=nt.POLY, beta=beta)
    for k in ("tried", "attempts", "success", "best_bits"):
        np.testing.assert_array_equal(host[k], exp[k], err_msg=f"{name}: host-ranked {k}")
