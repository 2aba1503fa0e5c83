"""GPU: DL-SCL retries on an adaptive baseline (pscl_retry_device, pscl_adaptive_dlscl_device,
pscl_simulate_adaptive_dl[_device]).  Every output -- best bits, CRC flag, best index of the final
attempt, stage, attempts, the tried flips in order -- and the three counter rows equal the oracle
composition of adaptive_dl_cases.compose_dl, bit for bit.  The counts asserted beside each input are
the oracle's on the CPU (test_adaptive_dl_cpu.py pins them too)."""
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_dl_cases as dc
import oracle
import staged_cases as sg
from polar_code_amd import _native

pytestmark = pytest.mark.gpu

NC = _native.PSCL_NCOUNT
ROOT = Path(__file__).resolve().parent.parent


def _bits(words, K):
    j = np.arange(K)
    return ((words[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)


class Bufs:
    """Device buffers of one call on host rows; outputs sentinel-filled (0x5A bytes)."""

    def __init__(self, mem, dec, rows, R, ref_bits=None):
        rows = np.ascontiguousarray(rows, np.float64)
        self.B, self.R, self.W, self.K = len(rows), R, dec.W, dec.K
        B, W = self.B, self.W
        self.mem = mem
        self.llr = mem.alloc(max(rows.nbytes, 8))
        self.best, self.flags, self.stage = mem.alloc(max(B * W * 8, 8)), mem.alloc(max(B, 8)), mem.alloc(max(B, 8))
        self.att, self.tried = mem.alloc(max(B * 4, 8)), mem.alloc(max(B * R * 4, 8))
        self.n, self.cnt, self.ref = mem.alloc(8), mem.alloc(3 * NC * 8), 0
        if B:
            mem.upload(self.llr, rows)
        for p, n in ((self.best, B * W * 8), (self.flags, B), (self.stage, B), (self.att, B * 4), (self.tried, B * R * 4)):
            mem.memset(p, 0x5A, max(n, 8))
        mem.memset(self.n, 0xFF, 8)
        mem.memset(self.cnt, 0, 3 * NC * 8)
        if ref_bits is not None:
            self.ref = mem.alloc(B * W * 8)
            mem.upload(self.ref, sg.words(ref_bits))

    def read(self):
        mem, B, W, R = self.mem, self.B, self.W, self.R
        words = mem.download(self.best, max(B * W * 8, 8), np.uint64)[:B * W].reshape(B, W)
        flags = mem.download(self.flags, max(B, 8), np.uint8)[:B]
        return {"best_bits": _bits(words, self.K), "crc_pass": (flags & _native.PSCL_FLAG_CRC_PASS) != 0,
                "best_idx": (flags & _native.PSCL_FLAG_IDX_MASK).astype(np.int32),
                "stage": mem.download(self.stage, max(B, 8), np.uint8)[:B].copy(),
                "attempts": mem.download(self.att, max(B * 4, 8), np.int32)[:B].copy(),
                "tried": mem.download(self.tried, max(B * R * 4, 8), np.int32)[:B * R].reshape(B, R).copy(),
                "n_escalated": int(mem.download(self.n, 8, np.int32)[0]),
                "counters": mem.download(self.cnt, 3 * NC * 8, np.int64).reshape(3, NC).copy(), "flags": flags.copy(),
                "words": words.copy()}


def three_stage(dec, b, retries, beta=None, stride=None):
    dec.adaptive_dlscl_device(b.llr, b.B, retries, beta=beta, d_best=b.best, d_flags=b.flags, d_stage=b.stage,
                              d_attempts=b.att, d_tried=b.tried if b.R else 0, tried_stride=b.R if stride is None else stride,
                              d_ref=b.ref, k_payload=dec.K - dec.crc_deg if b.ref else 0, d_counters=b.cnt if b.ref else 0,
                              d_n_escalated=b.n)


def run(dec, rows, retries=8, beta=None, ref_bits=None):
    with _native.DeviceArena(dec) as mem:
        b = Bufs(mem, dec, rows, max(retries, 0), ref_bits)
        three_stage(dec, b, retries, beta)
        dec.sync()
        return b.read()


def check(dec, rows, exp, tag, retries=8, beta=None, sl=slice(None)):
    """One three-stage call with the oracle's final bits as the reference words: every output, the
    escalated count and the three counter rows."""
    n = len(rows)
    e = exp if sl == slice(None) else dc.prefix(exp, n)
    ref = e["best_bits"] ^ _noise(e["best_bits"].shape)
    out = run(dec, rows, retries, beta, ref_bits=ref)
    dc.assert_equals(out, e, tag)
    assert out["n_escalated"] == e["n_escalated"], tag
    np.testing.assert_array_equal(out["counters"], dc.counter_rows(e, ref, dec.K - dec.crc_deg, NC), err_msg=tag)
    return out


def _noise(shape):
    """A fixed sparse bit pattern: the reference words differ from every stage's bits somewhere."""
    return (np.random.default_rng(99).random(shape) < 0.01).astype(np.int8)


@pytest.fixture(scope="module")
def dec8():
    return _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)


@pytest.fixture(scope="module")
def dec4():
    return _native.Decoder(128, ac.info_set(128, 64), 4, ac.POLY24)


@pytest.mark.parametrize("L,with_beta,entries,recovered", [(8, False, 42, 10), (8, True, 42, 7), (4, False, 171, 79),
                                                           (4, True, 171, 38)])
def test_mixed_batch_equals_composition(L, with_beta, entries, recovered, dec8, dec4):
    exp = dc.mixed_case(L, with_beta)
    assert (len(ac.mixed_rows()), exp["n_escalated"], exp["n_entries"], exp["n_recovered"]) == (4099, 1040, entries, recovered)
    out = check(dec8 if L == 8 else dec4, ac.mixed_rows(), exp, f"mixed L={L} beta={with_beta}",
                beta=dc.golden_beta(L) if with_beta else None)
    assert np.count_nonzero(out["stage"] == 3) == entries


def _dlscl(dec, b, retries, beta, d_cs, d_cd):
    dec.dlscl_device(b.llr, b.B, retries, beta=beta, d_best=b.best, d_flags=b.flags, d_attempts=b.att, d_tried=b.tried,
                     tried_stride=b.R, d_ref=b.ref, k_payload=dec.K - dec.crc_deg, d_counters_scl=d_cs, d_counters_dl=d_cd)


@pytest.mark.parametrize("L", [8, 4])
def test_decode_then_retry_equals_dlscl(L, dec8, dec4):
    """pscl_decode_device then pscl_retry_device == pscl_dlscl_device, output for output."""
    dec, rows, beta = (dec8 if L == 8 else dec4), ac.mixed_rows(), dc.golden_beta(L)
    ref = ac.mixed_expected(L)["list_bits"] ^ _noise((4099, 64))
    with _native.DeviceArena(dec) as mem:
        a, b = Bufs(mem, dec, rows, 8, ref), Bufs(mem, dec, rows, 8, ref)
        _dlscl(dec, a, 8, beta, a.cnt, a.cnt + NC * 8)
        dec.decode_device(b.llr, b.B, d_best=b.best, d_flags=b.flags, d_ref=b.ref, k_payload=40, d_counters=b.cnt)
        dec.retry_device(b.llr, b.B, 8, beta=beta, d_best=b.best, d_flags=b.flags, d_stage=b.stage, d_attempts=b.att,
                         d_tried=b.tried, tried_stride=8, d_ref=b.ref, k_payload=40, d_counters_dl=b.cnt + NC * 8)
        dec.sync()
        x, y = a.read(), b.read()
    for k in ("words", "flags", "attempts", "tried"):
        np.testing.assert_array_equal(y[k], x[k], err_msg=f"L={L}: {k}")
    np.testing.assert_array_equal(y["counters"][:2], x["counters"][:2])
    ent = ~ac.mixed_expected(L)["list_ok"]  # the oracle: the frames plain SCL fails enter the chains
    assert ent.sum() > 40 and np.all(y["stage"][ent] == 3) and np.all(y["stage"][~ent] == 0x5A)
    assert np.all(y["attempts"][~ent] == 1) and np.all(y["tried"][~ent] == -1) and np.all(y["attempts"][ent] > 1)


def test_sc_escalate_retry_equals_three_stage(dec8):
    rows, beta, exp = ac.mixed_rows(), dc.golden_beta(8), dc.mixed_case(8, True)
    with _native.DeviceArena(dec8) as mem:
        b = Bufs(mem, dec8, rows, 8)
        dec8.sc_device(b.llr, b.B, d_best=b.best, d_flags=b.flags, d_stage=b.stage)
        assert dec8.escalate_device(b.llr, b.B, d_best=b.best, d_flags=b.flags, d_stage=b.stage) == 1040
        dec8.retry_device(b.llr, b.B, 8, beta=beta, d_best=b.best, d_flags=b.flags, d_stage=b.stage, d_attempts=b.att,
                          d_tried=b.tried, tried_stride=8)
        dec8.sync()
        staged = b.read()
    dc.assert_equals(staged, exp, "sc + escalate + retry")
    dc.assert_equals(run(dec8, rows, 8, beta), exp, "three-stage call")


@pytest.mark.parametrize("L,entries130,recovered130", [(8, 1, 1), (2, 18, 7)])
@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_prefixes_over_sentinels(B, L, entries130, recovered130, dec8):
    """Outputs are sentinel-filled before the call (Bufs): the frames that pass must still get
    attempts 1 and tried -1, and a stage.  L = 2: stage 2 runs on the exact kernel."""
    exp = dc.mixed_case(L)
    full = dc.prefix(exp, 130)
    assert (full["n_entries"], full["n_recovered"]) == (entries130, recovered130)
    dec = dec8 if L == 8 else _native.Decoder(128, ac.info_set(128, 64), 2, ac.POLY24)
    dec.adaptive_stats(reset=True)
    check(dec, ac.mixed_rows()[:B], exp, f"B={B} L={L}", sl=slice(0, B))
    st = dec.adaptive_stats()
    assert (st["exact"], st["screened"]) == ((1, 0) if L == 2 else (0, 1)), st


def test_no_frame_enters(dec8):
    rows, exp = dc.allpass_case()
    assert exp["n_escalated"] == exp["n_entries"] == 0
    before = dec8.path_stats()
    out = check(dec8, rows, exp, "all pass")
    after = dec8.path_stats()
    assert after["post_rounds"] == before["post_rounds"] and after["fused_post_rounds"] == before["fused_post_rounds"]
    assert np.all(out["attempts"] == 1) and np.all(out["stage"] == 1) and np.all(out["tried"] == -1) and out["n_escalated"] == 0


def test_every_frame_enters_two_chains(dec8):
    rows, exp = dc.allfail_case()
    m = re.search(r"constexpr int kMinSplit = (\d+);", (ROOT / "polar_code_amd" / "csrc" / "capi.cpp").read_text())
    assert m and 5000 >= 2 * int(m.group(1)), "5,000 entries no longer reach the two-chain split"
    exp5 = dc.tiled(exp, 5)
    assert exp5["n_entries"] == 5000 and np.all(exp5["attempts"] == 9)
    out = check(dec8, np.tile(rows, (5, 1)), exp5, "all fail x5")
    assert np.all(out["stage"] == 3)


def test_nr_rate_matched():
    rows, exp = dc.nr_case()
    assert (exp["n_escalated"], exp["n_entries"], exp["n_recovered"]) == (1131, 178, 65)
    dec = _native.Decoder(128, ac.info_set(128, 88), 8, ac.POLY24)
    dec.set_rate_match(256)
    check(dec, rows, exp, "NR (128,88) E=256")


def test_runtime_info_set_and_crc16():
    rows, info, exp = dc.crc16_case()
    assert (len(rows), exp["n_escalated"], exp["n_entries"], exp["n_recovered"]) == (1027, 691, 294, 75)
    check(_native.Decoder(128, info, 4, ac.POLY16), rows, exp, "(128,40) CRC-16")


def test_n256_takes_the_long_chain():
    rows, info, exp = dc.n256_case()
    assert (exp["n_escalated"], exp["n_entries"], exp["n_recovered"]) == (199, 105, 17)
    check(_native.Decoder(256, info, 4, ac.POLY24), rows, exp, "(256,128) constructed")


def test_n32():
    rows, info, crc, exp = dc.c32_case()
    assert (exp["n_entries"], exp["n_recovered"]) == (2, 0)
    check(_native.Decoder(32, info, 4, crc), rows, exp, "c32")


def test_n1024():
    rows, info, exp = dc.n1024_case()
    assert len(rows) <= 131 and exp["n_entries"] >= 8 and exp["n_recovered"] >= 1
    check(_native.Decoder(1024, info, 4, ac.POLY24), rows, exp, "pw1024")


def test_retries_3_with_stride_3(dec8):
    exp = dc.mixed_case(8, False, 3)
    assert (exp["n_entries"], exp["n_recovered"]) == (42, 9) and exp["tried"].shape[1] == 3
    check(dec8, ac.mixed_rows(), exp, "retries 3", retries=3)


def test_retries_0_equals_adaptive_async(dec8):
    rows = ac.mixed_rows()
    out = run(dec8, rows, 0)
    ac.assert_equals(out, ac.mixed_expected(8), "retries 0")
    assert np.all(out["attempts"] == 1) and out["n_escalated"] == 1040
    with _native.DeviceArena(dec8) as mem:
        b = Bufs(mem, dec8, rows, 0)
        dec8.adaptive_async_device(b.llr, b.B, d_best=b.best, d_flags=b.flags, d_stage=b.stage, d_n_escalated=b.n)
        dec8.sync()
        plain = b.read()
    for k in ("words", "flags", "stage", "n_escalated"):
        np.testing.assert_array_equal(out[k], plain[k], err_msg=k)


@pytest.mark.parametrize("depth", [1, 2])
def test_pipelined_calls_equal_stream_ordered(depth):
    """Five three-stage calls on two alternating output sets, pipelined against stream-ordered (the
    form of test_pipelined_dlscl_calls_equal_stream_ordered): the last two calls' outputs and the
    counters of all five.  The stream-ordered run is held to the oracle by the other tests; the last
    call's outputs are compared with it here too."""
    info, beta = ac.info_set(128, 64), dc.golden_beta(8)
    batches = [ac.mixed_rows(), np.ascontiguousarray(ac.mixed_rows()[::-1]), ac.mixed_rows(),
               np.ascontiguousarray(ac.mixed_rows()[::-1]), ac.mixed_rows()]
    exp = dc.mixed_case(8, True)
    ref = exp["best_bits"] ^ _noise((4099, 64))
    res = {}
    for pipe in (True, False):
        dec = _native.Decoder(128, info, 8, ac.POLY24)
        dec.set_pipelined(pipe, depth=depth)
        with _native.DeviceArena(dec) as mem:
            ins = [Bufs(mem, dec, r, 8, ref if i % 2 == 0 else np.ascontiguousarray(ref[::-1])) for i, r in enumerate(batches)]
            outs = [Bufs(mem, dec, batches[0][:1], 8) for _ in range(2)]
            d_cnt = mem.alloc(3 * NC * 8)
            mem.memset(d_cnt, 0, 3 * NC * 8)
            for o in outs:  # (output sets of the full batch size)
                o.B, o.best, o.flags, o.stage = 4099, mem.alloc(4099 * 8), mem.alloc(4099), mem.alloc(4099)
                o.att, o.tried = mem.alloc(4099 * 4), mem.alloc(4099 * 8 * 4)
            for i, b in enumerate(ins):
                o = outs[i % 2]
                dec.adaptive_dlscl_device(b.llr, 4099, 8, beta=beta, d_best=o.best, d_flags=o.flags, d_stage=o.stage,
                                          d_attempts=o.att, d_tried=o.tried, tried_stride=8, d_ref=b.ref, k_payload=40,
                                          d_counters=d_cnt, d_n_escalated=o.n)
            dec.join()
            dec.sync()
            res[pipe] = ([o.read() for o in outs], mem.download(d_cnt, 3 * NC * 8, np.int64).reshape(3, NC).copy())
        dec.close()
    for i in range(2):
        for k in ("words", "flags", "stage", "attempts", "tried", "n_escalated"):
            np.testing.assert_array_equal(res[True][0][i][k], res[False][0][i][k], err_msg=f"{k}, set {i}")
    np.testing.assert_array_equal(res[True][1], res[False][1], err_msg="counters")
    dc.assert_equals(res[True][0][0], exp, "pipelined, last call")
    np.testing.assert_array_equal(res[True][1], 5 * dc.counter_rows(exp, ref, 40, NC))


def test_dlscl_after_three_stage_is_unchanged():
    dec, rows, beta = _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24), ac.mixed_rows(), dc.golden_beta(8)
    ref = ac.mixed_expected(8)["list_bits"]
    with _native.DeviceArena(dec) as mem:
        a, b, c = Bufs(mem, dec, rows, 8, ref), Bufs(mem, dec, rows, 8, ref), Bufs(mem, dec, rows, 8, ref)
        _dlscl(dec, a, 8, beta, a.cnt, a.cnt + NC * 8)
        three_stage(dec, c, 8, beta)
        _dlscl(dec, b, 8, beta, b.cnt, b.cnt + NC * 8)
        dec.sync()
        x, y = a.read(), b.read()
    for k in ("words", "flags", "attempts", "tried", "counters"):
        np.testing.assert_array_equal(y[k], x[k], err_msg=k)
    assert (x["attempts"] > 1).sum() > 40


# ---- the sweep

def _sim_expected(dec, info, L, seed, sid, ebno, frame0, B, retries, beta):
    """The rows and messages of the frame range regenerated with channel_device, then the oracle
    composition on the host: the four counter rows."""
    K, W, N = len(info), dec.W, 128
    with _native.DeviceArena(dec) as mem:
        d_llr, d_msg, d_unc = mem.alloc(B * N * 8), mem.alloc(B * W * 8), mem.alloc(8 * NC)
        mem.memset(d_unc, 0, 8 * NC)
        dec.channel_device(seed, sid, ebno, K / N, 40, frame0, B, d_llr, d_msg)
        dec.uncoded_device(seed, sid, ebno, 40, frame0, B, d_unc)
        dec.sync()
        rows = mem.download(d_llr, B * N * 8, np.float64).reshape(B, N)
        msg = _bits(mem.download(d_msg, B * W * 8, np.uint64).reshape(B, W), K)
        unc = mem.download(d_unc, 8 * NC, np.int64)
    exp = dc.compose_dl(rows, info, L, ac.POLY24, retries, beta)
    want = np.zeros((4, NC), np.int64)
    want[:3] = dc.counter_rows(exp, msg, 40, NC)
    want[3] = unc
    return want


def test_simulate_adaptive_dl_two_shards(dec8):
    info, seed, sid, ebno, beta = ac.info_set(128, 64), 2026, 52, 4.0, dc.golden_beta(8)
    shards = [(500, 3000), (3500, 2987)]  # (a frame0 offset; the second no multiple of 64)
    total = np.zeros((4, NC), np.int64)
    dec8.set_beta(beta)
    with _native.DeviceArena(dec8) as mem:
        d_cnt = mem.alloc(4 * NC * 8)
        mem.memset(d_cnt, 0, 4 * NC * 8)
        for f0, B in shards:
            want = _sim_expected(dec8, info, 8, seed, sid, ebno, f0, B, 8, beta)
            total += want
            np.testing.assert_array_equal(dec8.simulate_adaptive_dl(seed, sid, ebno, 0.5, 40, f0, B, 8, True), want)
            np.testing.assert_array_equal(dec8.simulate_adaptive(seed, sid, ebno, 0.5, 40, f0, B, True)[2], want[3])
            dec8.simulate_adaptive_dl_device(seed, sid, ebno, 0.5, 40, f0, B, 8, True, d_cnt)
        dec8.join()
        dec8.sync()
        np.testing.assert_array_equal(mem.download(d_cnt, 4 * NC * 8, np.int64).reshape(4, NC), total)
    one = dec8.simulate_adaptive_dl(seed, sid, ebno, 0.5, 40, 500, 5987, 8, True)
    np.testing.assert_array_equal(one, total)  # shards add up exactly
    dec8.set_beta(None)
    assert total[2, _native.CNT_RETRIES] > 0 and total[2, 1] < total[1, 1] and 0 < total[1, _native.CNT_ESCALATED] < 5987


def test_cli_csv(tmp_path):
    from polar_code_amd import config
    from polar_code_amd.eval import run_adaptive_sweep as ras
    from polar_code_amd.utils.seeding import philox_stream_id

    cfg = config.get_config()
    frames, snr = 3001, 4.0
    base = ["--M", "8", "--frames", str(frames), "--snr_lo", str(snr), "--snr_hi", str(snr), "--snr_step", "0", "--seed", "3",
            "--include_uncoded"]
    beta_path = str(ROOT / "tests" / "golden" / "beta_M8.npy")
    ras.run_sweep(ras.build_argparser().parse_args(base + ["--retries", "8", "--beta", beta_path, "--out_dir", str(tmp_path / "r8")]))
    lines = (tmp_path / "r8" / "fer_adaptive_M8.csv").read_text().splitlines()
    assert lines[0].split(",") == ras.csv_header(True, 8) and len(lines) == 2
    kp = cfg.K - cfg.crc_bits
    dec = _native.Decoder(cfg.N, oracle.construct_info_set(cfg.N, cfg.K), 8, cfg.crc_poly)
    dec.set_beta(dc.golden_beta(8))
    cnt = dec.simulate_adaptive_dl(3, philox_stream_id(snr), snr, cfg.K / cfg.N, kp, 0, frames, 8, True)
    row = ras.row_from_counters(snr, cnt, frames, cfg.K, kp, True, 8)
    assert lines[1] == ",".join(f"{row[k]:.3f}" if k == "snr_db" else f"{row[k]:.6e}" for k in ras.csv_header(True, 8))
    assert cnt[2, _native.CNT_RETRIES] > 0 and row["fer_dl"] <= row["fer_adaptive"]
    # --retries 0: the file written without the flag, byte for byte
    ras.run_sweep(ras.build_argparser().parse_args(base + ["--out_dir", str(tmp_path / "a")]))
    ras.run_sweep(ras.build_argparser().parse_args(base + ["--retries", "0", "--out_dir", str(tmp_path / "b")]))
    assert (tmp_path / "a" / "fer_adaptive_M8.csv").read_bytes() == (tmp_path / "b" / "fer_adaptive_M8.csv").read_bytes()
    assert lines[1].split(",")[:8] == (tmp_path / "a" / "fer_adaptive_M8.csv").read_text().splitlines()[1].split(",")


def test_host_forms(dec8):
    from polar_code_amd.dlscl import flip

    rows, exp, beta = ac.mixed_rows()[:1500], dc.prefix(dc.mixed_case(8, True), 1500), dc.golden_beta(8)
    out = dec8.decode_adaptive(rows, retries=8, beta=beta)
    dc.assert_equals(out, exp, "decode_adaptive(retries=8)")
    assert out["n_escalated"] == exp["n_escalated"]
    assert set(dec8.decode_adaptive(rows)) == {"best_bits", "crc_pass", "best_idx", "stage", "n_escalated"}  # the default
    got = flip.decode_with_retries_device(rows, ac.info_set(128, 64), 8, 8, crc=ac.POLY24, beta=beta, baseline="adaptive",
                                          msg=exp["best_bits"])
    for k, e in (("best_bits", "best_bits"), ("success", "crc_pass"), ("attempts", "attempts"), ("tried", "tried"),
                 ("stage", "stage"), ("base_bits", "base_bits"), ("base_pass", "base_ok")):
        np.testing.assert_array_equal(got[k], exp[e], err_msg=k)
    want = dc.counter_rows(exp, exp["best_bits"], 40, NC)
    for k, r in (("sc", 0), ("scl", 1), ("dl", 2)):
        np.testing.assert_array_equal(got["counters"][k], want[r], err_msg=k)


def test_errors():
    info = ac.info_set(128, 64)
    dec = _native.Decoder(128, info, 8, ac.POLY24)
    nocrc = _native.Decoder(128, info, 8, None)
    with pytest.raises(ValueError):  # no CRC
        nocrc.adaptive_dlscl_device(1, 1, 8, d_best=1, d_flags=1)
    with pytest.raises(ValueError):
        nocrc.retry_device(1, 1, 8, d_best=1, d_flags=1)
    with pytest.raises(ValueError):
        nocrc.simulate_adaptive_dl(1, 1, 4.0, 0.5, 40, 0, 10, 8)
    with pytest.raises(NotImplementedError):  # N = 16
        _native.Decoder(16, ac.info_set(16, 12), 4, sg.POLY8).adaptive_dlscl_device(1, 1, 8, d_best=1, d_flags=1)
    with pytest.raises(NotImplementedError):  # rate matching at N = 256
        d = _native.Decoder(256, ac.info_set(256, 128), 4, ac.POLY24)
        d.set_rate_match(300)
        d.adaptive_dlscl_device(1, 1, 8, d_best=1, d_flags=1)
    for call in (dec.adaptive_dlscl_device, dec.retry_device):
        with pytest.raises(ValueError):  # tried_stride below the rounds
            call(1, 1, 8, d_best=1, d_flags=1, d_tried=1, tried_stride=7)
        with pytest.raises(ValueError):  # d_ref without counters
            call(1, 1, 8, d_best=1, d_flags=1, d_ref=1)
        with pytest.raises(ValueError):
            call(1, -1, 8, d_best=1, d_flags=1)
        call(0, 0, 8, d_best=0, d_flags=0)  # B = 0 is fine
