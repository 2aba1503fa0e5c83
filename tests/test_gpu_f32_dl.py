"""GPU: DL-SCL retry chains on float32 LLR rows (pscl_dlscl_device_f32, pscl_retry_device_f32,
pscl_adaptive_dlscl_device_f32, pscl_path_llrs_device_f32) and the DL-SCL tensor methods.  Every
output -- best bits, CRC flag, best index of the final attempt, stage, attempts, the tried flips in
order -- and every counter equals the oracle composition on the rows widened on the host
(f32_dl_cases; test_f32_dl_cpu.py pins the cases' counts), and the float64 call on the widened rows
returns byte-identical buffers."""
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_dl_cases as dc
import f32_cases as fc
import f32_dl_cases as fd
import staged_cases as sg
from polar_code_amd import _native

pytestmark = pytest.mark.gpu

NC = _native.PSCL_NCOUNT
PASS, IDX = _native.PSCL_FLAG_CRC_PASS, _native.PSCL_FLAG_IDX_MASK
EUNSUP, EINVAL = -5, -1
SENTINEL = 0x5A
ROOT = Path(__file__).resolve().parent.parent
RAW = ("words", "flags", "stage", "attempts", "tried", "n_escalated", "counters")  # the buffers, byte for byte


def _bits(words, K):
    j = np.arange(K)
    return ((words[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)


def _noise(shape):
    """A fixed sparse bit pattern: the reference words differ from every stage's bits somewhere."""
    return (np.random.default_rng(99).random(shape) < 0.01).astype(np.int8)


class Bufs:
    """Device buffers of one call: float32 or float64 rows (float32 rows optionally `offset` bytes into
    their allocation), outputs of B + pad frames pre-filled with a sentinel, R tried columns."""

    def __init__(self, mem, dec, rows, R, ref_bits=None, offset=0, pad=0):
        assert rows.dtype in (np.float32, np.float64) and rows.flags.c_contiguous
        self.dec, self.mem, self.f32 = dec, mem, rows.dtype == np.float32
        self.B, self.R, self.W, self.K, self.n_out = len(rows), R, dec.W, dec.K, len(rows) + pad
        n, W = self.n_out, self.W
        self.llr = mem.alloc(max(rows.nbytes, 8) + offset) + offset
        if len(rows):
            mem.upload(self.llr, rows)
        self.sizes = {"best": n * W * 8, "flags": n, "stage": n, "att": n * 4, "tried": n * R * 4}
        for k, size in self.sizes.items():
            setattr(self, k, mem.alloc(max(size, 8)))
            mem.memset(getattr(self, k), SENTINEL, max(size, 8))
        self.n, self.cnt, self.ref = mem.alloc(8), mem.alloc(3 * NC * 8), 0
        mem.memset(self.n, 0xFF, 8)
        mem.memset(self.cnt, 0, 3 * NC * 8)
        if ref_bits is not None:
            self.ref = mem.alloc(self.B * W * 8)
            mem.upload(self.ref, sg.words(ref_bits))

    def _common(self, stride):
        kp = self.dec.K - self.dec.crc_deg
        return dict(d_best=self.best, d_flags=self.flags, d_attempts=self.att, d_tried=self.tried if self.R else 0,
                    tried_stride=self.R if stride is None else stride, d_ref=self.ref, k_payload=kp if self.ref else 0)

    def three_stage(self, retries, beta=None, stride=None):
        f = self.dec.adaptive_dlscl_device_f32 if self.f32 else self.dec.adaptive_dlscl_device
        f(self.llr, self.B, retries, beta=beta, d_stage=self.stage, d_counters=self.cnt if self.ref else 0, d_n_escalated=self.n,
          **self._common(stride))

    def dlscl(self, retries, beta=None):
        f = self.dec.dlscl_device_f32 if self.f32 else self.dec.dlscl_device
        f(self.llr, self.B, retries, beta=beta, d_counters_scl=self.cnt if self.ref else 0,
          d_counters_dl=self.cnt + NC * 8 if self.ref else 0, **self._common(None))

    def decode_then_retry(self, retries, beta=None):
        kp = self.dec.K - self.dec.crc_deg
        dec, ref = self.dec, dict(d_ref=self.ref, k_payload=kp) if self.ref else {}
        plain, retry = (dec.decode_device_f32, dec.retry_device_f32) if self.f32 else (dec.decode_device, dec.retry_device)
        plain(self.llr, self.B, d_best=self.best, d_flags=self.flags, **ref, **(dict(d_counters=self.cnt) if self.ref else {}))
        retry(self.llr, self.B, retries, beta=beta, d_best=self.best, d_flags=self.flags, d_stage=self.stage, d_attempts=self.att,
              d_tried=self.tried, tried_stride=self.R, **ref, **(dict(d_counters_dl=self.cnt + NC * 8) if self.ref else {}))

    def read(self):
        """The outputs of the B frames; asserts that the pad frames behind them still hold the sentinel."""
        mem, B, W, R, n = self.mem, self.B, self.W, self.R, self.n_out
        raw = {k: mem.download(getattr(self, k), max(size, 8), np.uint8)[:size] for k, size in self.sizes.items()}
        for k, per in (("best", W * 8), ("flags", 1), ("stage", 1), ("att", 4), ("tried", R * 4)):
            assert np.all(raw[k][B * per:] == SENTINEL), f"{k} written behind frame B"
        words = raw["best"][:B * W * 8].view(np.uint64).reshape(B, W)
        flags = raw["flags"][:B]
        return {"best_bits": _bits(words, self.K), "crc_pass": (flags & PASS) != 0, "best_idx": (flags & IDX).astype(np.int32),
                "stage": raw["stage"][:B].copy(), "attempts": raw["att"][:B * 4].view(np.int32).copy(),
                "tried": raw["tried"][:B * R * 4].view(np.int32).reshape(B, R).copy(),
                "n_escalated": int(mem.download(self.n, 8, np.int32)[0]),
                "counters": mem.download(self.cnt, 3 * NC * 8, np.int64).reshape(3, NC).copy(), "flags": flags.copy(),
                "words": words.copy()}


def assert_same(a, b, tag, keys=RAW):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {k} differs from the float64 call's on the widened rows")


def check_both(dec, rows32, exp, tag, retries=8, beta=None, offset=0, pad=0):
    """One pscl_adaptive_dlscl_device_f32 call with the oracle's final bits (plus noise) as the reference
    words: every key of adaptive_dl_cases.KEYS, the escalated count and the three counter rows against
    the oracle; then the float64 call on the widened rows: the same buffers and counters, byte for byte."""
    assert rows32.dtype == np.float32
    ref = exp["best_bits"] ^ _noise(exp["best_bits"].shape)
    with _native.DeviceArena(dec) as mem:
        a = Bufs(mem, dec, rows32, max(retries, 0), ref, offset=offset, pad=pad)
        b = Bufs(mem, dec, fc.widen(rows32), max(retries, 0), ref, pad=pad)
        a.three_stage(retries, beta)
        dec.sync()
        oa = a.read()
        b.three_stage(retries, beta)
        dec.sync()
        ob = b.read()
    dc.assert_equals(oa, exp, tag)
    assert oa["n_escalated"] == exp["n_escalated"], tag
    np.testing.assert_array_equal(oa["counters"], dc.counter_rows(exp, ref, dec.K - dec.crc_deg, NC), err_msg=tag)
    assert_same(oa, ob, tag)
    return oa


@pytest.fixture(scope="module")
def dec8():
    return _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)


@pytest.fixture(scope="module")
def dec4():
    return _native.Decoder(128, ac.info_set(128, 64), 4, ac.POLY24)


def _nr(L, E, info=None, crc=ac.POLY24):
    dec = _native.Decoder(128, ac.info_set(128, 88) if info is None else info, L, crc)
    dec.set_rate_match(E)
    return dec


# ---- 1. the mixed batch (and 7: the float64 call on the widened rows)

@pytest.mark.parametrize("L,with_beta", [(8, False), (8, True), (4, False), (4, True)])
def test_mixed_batch_equals_composition(L, with_beta, dec8, dec4):
    dec = dec8 if L == 8 else dec4
    assert dec.f32_available()
    exp = fd.mixed_case(L, with_beta)
    out = check_both(dec, fc.mixed_rows(), exp, f"mixed L={L} beta={with_beta}", beta=dc.golden_beta(L) if with_beta else None)
    assert np.count_nonzero(out["stage"] == 3) == exp["n_entries"] > 40


# ---- 2. the plain chain

@pytest.mark.parametrize("L", [8, 4])
def test_plain_chain_equals_dl_batch(L, dec8, dec4):
    dec, beta = (dec8 if L == 8 else dec4), dc.golden_beta(L)
    rows, exp = fd.plain_case(L)
    ref = exp["best_bits"] ^ _noise(exp["best_bits"].shape)
    want = np.zeros((3, NC), np.int64)
    want[0] = sg.host_counts(exp["base_bits"], exp["base_ok"], ref, 40, NC)  # (the baseline's block)
    want[1] = sg.host_counts(exp["best_bits"], exp["crc_pass"], ref, 40, NC)  # (the final outputs')
    want[1, _native.CNT_RETRIES] = int((exp["attempts"] - 1).sum())
    with _native.DeviceArena(dec) as mem:
        a, b, c = Bufs(mem, dec, rows, 8, ref), Bufs(mem, dec, rows, 8, ref), Bufs(mem, dec, fc.widen(rows), 8, ref)
        a.dlscl(8, beta)
        b.decode_then_retry(8, beta)
        c.dlscl(8, beta)
        dec.sync()
        x, y, z = a.read(), b.read(), c.read()
    dc.assert_equals(x, exp, f"dlscl_f32 L={L}", keys=fd.PLAIN_KEYS)
    np.testing.assert_array_equal(x["counters"], want, err_msg=f"L={L}: both counter blocks")
    keys = ("words", "flags", "attempts", "tried", "counters")
    assert_same(x, z, f"dlscl L={L}", keys)
    for k in keys:
        np.testing.assert_array_equal(y[k], x[k], err_msg=f"decode_f32 + retry_f32, L={L}: {k}")
    ent = ~exp["base_ok"]  # (pscl_retry_device_f32 marks the frames that enter a chain, no other)
    assert np.all(y["stage"][ent] == 3) and np.all(y["stage"][~ent] == SENTINEL) and np.all(x["stage"] == SENTINEL)


# ---- 3. ties: the screened retry decode defers, the exact float32 side chain decides

@pytest.mark.parametrize("L", [8, 4])
@pytest.mark.parametrize("with_beta", [False, True])
def test_ties_take_the_exact_f32_side_chain(L, with_beta, dec8, dec4):
    dec = dec8 if L == 8 else dec4
    rows, exp = fd.tie_case(L, with_beta)
    before = dec.path_stats()
    check_both(dec, rows, exp, f"ties L={L} beta={with_beta}", beta=dc.golden_beta(L) if with_beta else None)
    after = dec.path_stats()
    # (pscl_path_stats has no counter of the side chain's launches: what it shows is that the rounds ran
    # as the default chain -- eight separate post passes per call, none fused, none on the exact lane kernel)
    assert after["post_rounds"] - before["post_rounds"] == 16 and after["fused_post_rounds"] == before["fused_post_rounds"]
    assert after["lane_exact_launches"] == before["lane_exact_launches"]


# ---- 4. corners

def test_corners(dec8):
    rows, exp = fd.corner_case()
    check_both(dec8, rows, exp, "corners")


# ---- 5. rate matched

@pytest.mark.parametrize("E,offset", [(256, 0), (201, 4)])
def test_rate_matched(E, offset):
    rows, exp = fd.nr_case(E)
    assert exp["n_entries"] > 10
    check_both(_nr(8, E), rows, exp, f"NR (128,88) E={E}", offset=offset)


# ---- 6. sizes

@pytest.mark.parametrize("B", [1, 7, 63, 65])
def test_prefixes_over_sentinels(B, dec8):
    rows = np.ascontiguousarray(fc.mixed_rows()[:B])
    check_both(dec8, rows, dc.prefix(fd.mixed_case(8), B), f"B={B}", pad=5)


def test_no_frame_enters(dec8):
    rows, exp = fd.allpass_case()
    before = dec8.path_stats()
    out = check_both(dec8, rows, exp, "all pass")
    after = dec8.path_stats()
    assert after["post_rounds"] == before["post_rounds"] and after["fused_post_rounds"] == before["fused_post_rounds"]
    assert np.all(out["attempts"] == 1) and np.all(out["stage"] == 1) and np.all(out["tried"] == -1) and out["n_escalated"] == 0


def test_every_frame_enters_two_chains(dec8):
    rows, exp = fd.allfail_case()
    m = re.search(r"constexpr int kMinSplit = (\d+);", (ROOT / "polar_code_amd" / "csrc" / "capi.cpp").read_text())
    assert m and 5000 >= 2 * int(m.group(1)), "5,000 entries no longer reach the two-chain split"
    exp5 = dc.tiled(exp, 5)
    assert exp5["n_entries"] == 5000 and np.all(exp5["attempts"] == 9)
    tiled = np.ascontiguousarray(np.tile(rows, (5, 1)))
    out = check_both(dec8, tiled, exp5, "all fail x5")
    assert np.all(out["stage"] == 3)


def test_retries_3_with_stride_3(dec8):
    exp = fd.mixed_case(8, False, 3)
    assert exp["tried"].shape[1] == 3
    check_both(dec8, fc.mixed_rows(), exp, "retries 3", retries=3)


def test_retries_0_equals_adaptive_async_f32(dec8):
    rows = fc.mixed_rows()
    with _native.DeviceArena(dec8) as mem:
        a, b = Bufs(mem, dec8, rows, 0), Bufs(mem, dec8, rows, 0)
        a.three_stage(0)
        dec8.adaptive_async_device_f32(b.llr, b.B, d_best=b.best, d_flags=b.flags, d_stage=b.stage, d_n_escalated=b.n)
        dec8.sync()
        out, plain = a.read(), b.read()
    ac.assert_equals(out, fc.mixed_expected(8), "retries 0")
    assert np.all(out["attempts"] == 1) and out["n_escalated"] == 1040
    for k in ("words", "flags", "stage", "n_escalated"):
        np.testing.assert_array_equal(out[k], plain[k], err_msg=k)


# ---- 8. pipelined: the row type travels with the deferred chains

def test_pipelined_alternating_dtypes_equal_stream_ordered():
    """Five three-stage calls at depth 2, float64 and float32 rows alternating, on two alternating
    output sets: a call's chains are enqueued by the NEXT call, whose rows are of the other type.  The
    batches differ too (mixed rows, and mixed rows reversed), so chains that read the wrong batch or
    the wrong type cannot agree with the stream-ordered run, which the other tests hold to the oracle."""
    info, beta = ac.info_set(128, 64), dc.golden_beta(8)
    m32 = fc.mixed_rows()
    r32 = np.ascontiguousarray(m32[::-1])
    batches = [fc.widen(m32), r32, fc.widen(m32), r32, fc.widen(m32)]
    exp = fd.mixed_case(8, True)
    ref = exp["best_bits"] ^ _noise((4099, 64))
    res = {}
    for pipe in (True, False):
        dec = _native.Decoder(128, info, 8, ac.POLY24)
        if pipe:
            dec.set_pipelined(True, depth=2)
        with _native.DeviceArena(dec) as mem:
            ins = [Bufs(mem, dec, r, 8, ref if i % 2 == 0 else np.ascontiguousarray(ref[::-1])) for i, r in enumerate(batches)]
            outs = [Bufs(mem, dec, batches[0], 8) for _ in range(2)]
            d_cnt = mem.alloc(3 * NC * 8)
            mem.memset(d_cnt, 0, 3 * NC * 8)
            for i, b in enumerate(ins):
                o = outs[i % 2]
                call = dec.adaptive_dlscl_device_f32 if b.f32 else dec.adaptive_dlscl_device
                call(b.llr, 4099, 8, beta=beta, d_best=o.best, d_flags=o.flags, d_stage=o.stage, d_attempts=o.att,
                     d_tried=o.tried, tried_stride=8, d_ref=b.ref, k_payload=40, d_counters=d_cnt, d_n_escalated=o.n)
            dec.join()
            dec.sync()
            res[pipe] = ([o.read() for o in outs], mem.download(d_cnt, 3 * NC * 8, np.int64).reshape(3, NC).copy())
        dec.close()
    for i in range(2):
        assert_same(res[True][0][i], res[False][0][i], f"set {i}", keys=("words", "flags", "stage", "attempts", "tried", "n_escalated"))
    np.testing.assert_array_equal(res[True][1], res[False][1], err_msg="counters")
    dc.assert_equals(res[True][0][0], exp, "pipelined, last call (float64 rows)")
    rev = {k: exp[k][::-1] for k in dc.KEYS}
    dc.assert_equals(res[True][0][1], rev, "pipelined, fourth call (float32 rows)")
    np.testing.assert_array_equal(res[True][1], 5 * dc.counter_rows(exp, ref, 40, NC))


# ---- 9. the replay

@pytest.mark.parametrize("what", ["(128,64) plain", "(128,88) E=256", "(128,40) runtime set, E=201"])
def test_path_llrs_f32_equals_path_llrs_on_widened_rows(what, dec8):
    if what == "(128,64) plain":
        dec, rows = dec8, np.ascontiguousarray(fc.mixed_rows()[:263])
    elif what == "(128,88) E=256":
        dec, rows = _nr(8, 256), fc.nr_rows(256)
    else:
        dec = _nr(4, 201, ac.info_set(128, 40), ac.POLY16)
        rows = fc.nr_rows(201)  # (any received values: the replay follows the bits it is given)
    B, W, K = len(rows), dec.W, dec.K
    bits = sg.words(np.random.default_rng(7).integers(0, 2, size=(B, K)).astype(np.int8))
    with _native.DeviceArena(dec) as mem:
        d32, d64 = mem.alloc(rows.nbytes + 4) + 4, mem.alloc(rows.nbytes * 2)
        d_bits, o32, o64 = mem.alloc(B * W * 8), mem.alloc((B + 1) * K * 8), mem.alloc(B * K * 8)
        mem.upload(d32, rows)
        mem.upload(d64, fc.widen(rows))
        mem.upload(d_bits, bits)
        mem.memset(o32, SENTINEL, (B + 1) * K * 8)
        dec.path_llrs_device_f32(d32, B, d_bits, o32)
        dec.path_llrs_device(d64, B, d_bits, o64)
        dec.sync()
        a, b = mem.download(o32, (B + 1) * K * 8, np.uint64), mem.download(o64, B * K * 8, np.uint64)
    np.testing.assert_array_equal(a[:B * K], b, err_msg=what)  # (bit for bit)
    assert np.all(a[B * K:] == np.uint64(0x5A5A5A5A5A5A5A5A)) and len(np.unique(b)) > B


# ---- 10. refusals

def _refused_handles():
    info = ac.info_set(128, 64)
    off = _native.Decoder(128, info, 8, ac.POLY24)
    off.set_screening(False)
    knob = _native.Decoder(128, info, 8, ac.POLY24)
    knob.set_tuning(lane_exact=1)
    rm64 = _native.Decoder(128, info, 8, ac.POLY24)
    rm64.set_rate_match(256)
    fused = _native.Decoder(128, info, 8, ac.POLY24)
    fused.set_tuning(dl_fused_post=1)
    two_lane = _native.Decoder(128, info, 4, ac.POLY24)
    two_lane.set_tuning(dl_retry_lane=2)
    return {"N=256": _native.Decoder(256, sg.pw_info_set(256, 128), 8, ac.POLY24),
            "L=2": _native.Decoder(128, info, 2, ac.POLY24),
            "L=16": _native.Decoder(128, info, 16, ac.POLY24),
            "(128,40)+CRC-16": _native.Decoder(128, ac.info_set(128, 40), 4, ac.POLY16),
            "screening off": off, "lane_exact knob": knob, "(128,64) rate matched": rm64,
            "dl_fused_post knob": fused, "dl_retry_lane knob": two_lane}


KEY = {"N=256": "N = 128", "L=2": "L = 4 and 8", "L=16": "L = 4 and 8", "(128,40)+CRC-16": "information set",
       "screening off": "screening", "lane_exact knob": "PSCL_TUNE_LANE_EXACT", "(128,64) rate matched": "(128,88)",
       "dl_fused_post knob": "PSCL_TUNE_DL_FUSED_POST", "dl_retry_lane knob": "PSCL_TUNE_DL_RETRY_LANE"}


def _chain_calls(lib, h, d_llr, B, p_best, p_flags, p_stage=None, retries=8, p_tried=None, stride=0, p_ref=None, kp=0, p_cnt=None,
                 f64=True):
    """The three chain calls with one set of arguments: (float64 return codes, float32 return codes, the
    float32 calls' messages).  f64 = False: the float32 forms alone (float64 codes None)."""
    out = []
    for sfx in ("", "_f32"):
        codes, msgs = [], []
        if not sfx and not f64:
            out += [None, None]
            continue
        for code in (getattr(lib, "pscl_dlscl_device" + sfx)(h, d_llr, B, retries, p_best, p_flags, None, p_tried, stride, p_ref, kp, p_cnt, p_cnt),
                     getattr(lib, "pscl_retry_device" + sfx)(h, d_llr, B, retries, p_best, p_flags, p_stage, None, p_tried, stride, p_ref, kp, p_cnt),
                     getattr(lib, "pscl_adaptive_dlscl_device" + sfx)(h, d_llr, B, retries, p_best, p_flags, p_stage, None, p_tried, stride,
                                                                   p_ref, kp, p_cnt, None)):
            codes.append(code)
            msgs.append(lib.pscl_last_error().decode() if code else "")
        out += [codes, msgs]
    return out[0], out[2], out[3]


@pytest.mark.parametrize("what", sorted(KEY))
def test_refusals(what):
    dec = _refused_handles()[what]
    lib, h = _native.lib(), dec.handle
    knob = what.startswith("dl_")
    # (the two DL knobs leave the plain float32 decode native: pscl_f32_available keeps its answer)
    assert dec.f32_available() == knob and lib.pscl_f32_available(h) == int(knob)
    row = dec.E or dec.N
    with _native.DeviceArena(dec) as mem:
        d_llr, d_best, d_flags, d_stage = mem.alloc(4 * row * 8), mem.alloc(4 * dec.W * 8), mem.alloc(8), mem.alloc(8)
        mem.memset(d_llr, 0, 4 * row * 8)
        mem.memset(d_best, SENTINEL, 4 * dec.W * 8)
        _, codes, msgs = _chain_calls(lib, h, d_llr, 4, d_best, d_flags, d_stage, f64=False)
        dec.sync()
        assert np.all(mem.download(d_best, 4 * dec.W * 8, np.uint8) == SENTINEL)  # (nothing ran)
    assert codes == [EUNSUP] * 3, (what, codes, msgs)
    for m in msgs:
        assert KEY[what] in m, (what, m)
    # the replay takes every N = 128 handle
    with _native.DeviceArena(dec) as mem:
        d_llr, d_bits, d_out = mem.alloc(4 * row * 4), mem.alloc(4 * dec.W * 8), mem.alloc(4 * dec.K * 8)
        mem.memset(d_llr, 0, 4 * row * 4)
        mem.memset(d_bits, 0, 4 * dec.W * 8)
        assert lib.pscl_path_llrs_device_f32(h, d_llr, 4, d_bits, d_out) == (EUNSUP if dec.N != 128 else 0)
        dec.sync()


def test_argument_errors_come_first_with_the_float64_codes(dec8):
    lib, p = _native.lib(), 4096  # (any non-NULL value: the argument checks come before any launch)
    refused = _refused_handles()["(128,40)+CRC-16"]
    for h in (dec8.handle, refused.handle):  # (a refused handle reports the argument error, not PSCL_EUNSUP)
        for kw in (dict(B=-1), dict(d_llr=None), dict(p_best=None), dict(p_flags=None), dict(p_ref=p), dict(kp=65, p_ref=p, p_cnt=p),
                   dict(p_tried=p, stride=7)):
            args = dict(d_llr=p, B=4, p_best=p, p_flags=p)
            args.update(kw)
            c64, c32, msgs = _chain_calls(lib, h, **args)
            assert c64 == c32 == [EINVAL] * 3, (kw, c64, c32, msgs)
        c64, c32, _ = _chain_calls(lib, h, None, 0, None, None)  # B = 0 is fine
        assert c64 == c32 == [0, 0, 0]
    nocrc = _native.Decoder(128, ac.info_set(128, 64), 8, None)
    assert nocrc.f32_available()
    _, c32, msgs = _chain_calls(lib, nocrc.handle, p, 4, p, p, f64=False)  # (the float32 forms return before any launch)
    assert c32 == [EINVAL] * 3 and all("CRC" in m for m in msgs), (c32, msgs)


@pytest.mark.parametrize("knobs", [dict(dl_screen=2), dict(dl_screen=1), dict(dl_chunks=3), dict(dl_warm_apx=1), dict(dl_split=1)])
def test_native_knobs_keep_the_results(knobs):
    """The knobs the header lists as native: the plain chain on the first 1,027 rows under each equals
    the oracle (dl_chunks = 3 splits the float32 rows at chunk boundaries: 343 frames each)."""
    dec = _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    dec.set_tuning(**knobs)
    rows, exp = fd.plain_case(8)
    with _native.DeviceArena(dec) as mem:
        a = Bufs(mem, dec, rows, 8)
        a.dlscl(8, dc.golden_beta(8))
        dec.sync()
        dc.assert_equals(a.read(), exp, str(knobs), keys=fd.PLAIN_KEYS)


def test_post_epw_4_on_a_pipelined_handle():
    """PSCL_TUNE_POST_EPW = 4 (the narrow post pass at four entries per wavefront) is native too."""
    dec = _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    dec.set_tuning(post_epw=4)
    dec.set_pipelined(True, depth=2)
    rows, exp = fd.plain_case(8)
    with _native.DeviceArena(dec) as mem:
        bufs = [Bufs(mem, dec, rows, 8) for _ in range(2)]
        for b in bufs:
            b.dlscl(8, dc.golden_beta(8))
        dec.join()
        dec.sync()
        assert dec.path_stats()["post_epw4_launches"] > 0
        for b in bufs:
            dc.assert_equals(b.read(), exp, "post_epw=4", keys=fd.PLAIN_KEYS)
    dec.close()


# ---- 11. the tensor methods on a side stream

def _tensor_check(out, exp, K, tag, keys):
    got = {"best_bits": _bits(out["best"].cpu().numpy().view(np.uint64), K), "attempts": out["attempts"].cpu().numpy(),
           "tried": out["tried"].cpu().numpy()}
    f = out["flags"].cpu().numpy()
    got["crc_pass"], got["best_idx"] = (f & PASS) != 0, (f & IDX).astype(np.int32)
    if "stage" in out:
        got["stage"] = out["stage"].cpu().numpy()
    dc.assert_equals(got, exp, tag, keys=keys)


def test_tensor_methods_on_a_side_stream():
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    rows32, beta = fc.mixed_rows(), dc.golden_beta(8)
    exp, pexp = fd.mixed_case(8, True), fd.plain_case(8)[1]
    dec = SCLDecoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    assert dec.native.f32_available()
    stream = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(stream):
        llr32 = torch.from_numpy(rows32.copy()).to("cuda")
        for tag, llr in (("f32", llr32), ("f64", llr32.double())):
            cnt = torch.zeros((3, NC), dtype=torch.int64, device="cuda")
            refw = torch.from_numpy(sg.words(exp["best_bits"]).view(np.int64)).to("cuda")
            b, f, s, a, t, n = dec.decode_tensor_adaptive_dlscl(llr, 8, beta=beta, ref_words=refw, k_payload=40, counters=cnt)
            pb, pf, pa, pt = dec.decode_tensor_dlscl(llr[:fd.PLAIN_B].contiguous(), 8, beta=beta)
            rb, rf = dec.decode_tensor(llr[:fd.PLAIN_B].contiguous())
            rs = torch.full((fd.PLAIN_B,), SENTINEL, dtype=torch.uint8, device="cuda")
            ra, rt = dec.decode_tensor_retry(llr[:fd.PLAIN_B].contiguous(), rb, rf, 8, beta=beta, stage=rs)
            res[tag] = dict(three=dict(best=b, flags=f, stage=s, attempts=a, tried=t), n=n, cnt=cnt,
                            plain=dict(best=pb, flags=pf, attempts=pa, tried=pt), retry=dict(best=rb, flags=rf, attempts=ra, tried=rt), rs=rs)
    stream.synchronize()
    for tag, r in res.items():
        _tensor_check(r["three"], exp, 64, f"decode_tensor_adaptive_dlscl {tag}", dc.KEYS)
        assert r["n"].dtype == torch.int32 and int(r["n"].cpu()[0]) == exp["n_escalated"]
        np.testing.assert_array_equal(r["cnt"].cpu().numpy(), dc.counter_rows(exp, exp["best_bits"], 40, NC), err_msg=tag)
        _tensor_check(r["plain"], pexp, 64, f"decode_tensor_dlscl {tag}", fd.PLAIN_KEYS)
        _tensor_check(r["retry"], pexp, 64, f"decode_tensor_retry {tag}", fd.PLAIN_KEYS)
        np.testing.assert_array_equal(r["rs"].cpu().numpy(), np.where(pexp["base_ok"], SENTINEL, 3), err_msg=tag)
    dec.native.set_stream(None)


def test_tensor_methods_widen_where_there_is_no_native_kernel():
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    rows32, info, exp = fd.crc16_case()
    dec = SCLDecoder(128, info, 4, ac.POLY16)
    assert not dec.native.f32_available()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        llr = torch.from_numpy(rows32.copy()).to("cuda")
        b, f, s, a, t, n = dec.decode_tensor_adaptive_dlscl(llr, 8)
        sb, sf, ss = dec.decode_tensor_staged(llr)
        ra, rt = dec.decode_tensor_retry(llr, sb, sf, 8, stage=ss)
        wide = dec.decode_tensor_adaptive_dlscl(llr.double(), 8)
    stream.synchronize()
    _tensor_check(dict(best=b, flags=f, stage=s, attempts=a, tried=t), exp, 40, "widened three-stage", dc.KEYS)
    _tensor_check(dict(best=sb, flags=sf, stage=ss, attempts=ra, tried=rt), exp, 40, "widened staged + retry", dc.KEYS)
    assert int(n.cpu()[0]) == exp["n_escalated"]
    for x, y in zip((b, f, s, a, t, n), wide):
        assert torch.equal(x, y)
    dec.native.set_stream(None)
