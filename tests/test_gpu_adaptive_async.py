"""GPU: adaptive decoding without the host wait (pscl_adaptive_async_device,
pscl_simulate_adaptive[_device]).  Stage 2 is a row-list launch sized on the device: bits, CRC flag,
best index, stage and the device escalated count equal the composition of the oracle's sc_decode +
check_crc and decode_batch (adaptive_cases.compose), bit for bit, and pscl_adaptive_stats says
which kernel ran."""
import numpy as np
import pytest

import adaptive_cases as ac
import oracle
import staged_cases as sg
from polar_code_amd import _native

pytestmark = pytest.mark.gpu

NC = _native.PSCL_NCOUNT


def _bits(words, K):
    j = np.arange(K)
    return ((words[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)


def run_async(dec, rows, ref_bits=None, kp=0, prefill=None):
    """One pscl_adaptive_async_device call on host rows: compose()'s keys, the device escalated
    count, and (ref_bits) the counters.  prefill: byte the outputs are filled with first."""
    rows = np.ascontiguousarray(rows, np.float64)
    B, W = len(rows), dec.W
    with _native.DeviceArena(dec) as mem:
        d_llr, d_best, d_flags, d_stage = mem.alloc(max(rows.nbytes, 8)), mem.alloc(max(B * W * 8, 8)), mem.alloc(max(B, 8)), mem.alloc(max(B, 8))
        d_n, d_cnt, d_ref = mem.alloc(8), mem.alloc(8 * NC), 0
        if B:
            mem.upload(d_llr, rows)
        mem.memset(d_n, 0xFF, 8)
        mem.memset(d_cnt, 0, 8 * NC)
        if prefill is not None:
            mem.memset(d_best, prefill, max(B * W * 8, 8))
            mem.memset(d_flags, prefill, max(B, 8))
        if ref_bits is not None:
            d_ref = mem.alloc(B * W * 8)
            mem.upload(d_ref, sg.words(ref_bits))
        dec.adaptive_async_device(d_llr, B, d_best=d_best, d_flags=d_flags, d_stage=d_stage, d_ref=d_ref, k_payload=kp,
                                  d_counters=d_cnt if ref_bits is not None else 0, d_n_escalated=d_n)
        dec.sync()
        words = mem.download(d_best, max(B * W * 8, 8), np.uint64)[:B * W].reshape(B, W)
        flags = mem.download(d_flags, max(B, 8), np.uint8)[:B]
        stage = mem.download(d_stage, max(B, 8), np.uint8)[:B]
        n = int(mem.download(d_n, 8, np.int32)[0])
        cnt = mem.download(d_cnt, 8 * NC, np.int64)
    return {"best_bits": _bits(words, dec.K), "crc_pass": (flags & _native.PSCL_FLAG_CRC_PASS) != 0,
            "best_idx": (flags & _native.PSCL_FLAG_IDX_MASK).astype(np.int32), "stage": stage.copy(), "n_escalated": n,
            "counters": cnt, "words": words, "flags": flags}


def check(dec, rows, exp, tag, sl=slice(None), path="screened"):
    dec.adaptive_stats(reset=True)
    out = run_async(dec, rows)
    ac.assert_equals(out, exp, tag, sl)
    assert out["n_escalated"] == int(np.count_nonzero(exp["stage"][sl] == 2)), tag
    st = dec.adaptive_stats()
    other = "exact" if path == "screened" else "screened"
    assert st[path] == 1 and st[other] == 0, (tag, st)
    return out


@pytest.fixture(scope="module")
def dec8():
    return _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)


@pytest.fixture(scope="module")
def dec4():
    return _native.Decoder(128, ac.info_set(128, 64), 4, ac.POLY24)


@pytest.mark.parametrize("L", [8, 4])
def test_mixed_batch_equals_composition(L, dec8, dec4):
    exp = ac.mixed_expected(L)
    assert len(ac.mixed_rows()) == 4099 and exp["n_escalated"] == 1040  # (the oracle alone)
    check(dec8 if L == 8 else dec4, ac.mixed_rows(), exp, f"mixed L={L}")


@pytest.mark.parametrize("L", [8, 4])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_small_and_ragged_batches(B, L, dec8, dec4):
    check(dec8 if L == 8 else dec4, ac.mixed_rows()[:B], ac.mixed_expected(L), f"B={B} L={L}", slice(0, B))


@pytest.mark.parametrize("L", [8, 4])
def test_ragged_escalated_count(L, dec8, dec4):
    """An escalated count that is no multiple of the frames per wavefront (8 at L = 8, 16 at L = 4):
    the last wavefront of the row-list launch has empty slots."""
    exp = ac.mixed_expected(L)
    B = next(b for b in range(2000, 4099) if np.count_nonzero(exp["stage"][:b] == 2) % 16 not in (0, 8))
    n = int(np.count_nonzero(exp["stage"][:B] == 2))
    assert n % (64 // L) != 0 and n > 64
    out = check(dec8 if L == 8 else dec4, ac.mixed_rows()[:B], exp, f"ragged count {n} L={L}", slice(0, B))
    assert out["n_escalated"] == n


def test_no_frame_escalates(dec8):
    rows, exp = ac.allpass_case()
    assert exp["n_escalated"] == 0
    out = check(dec8, rows, exp, "all pass")
    assert out["n_escalated"] == 0 and np.all(out["stage"] == 1)


def test_every_frame_escalates(dec8):
    rows, exp = ac.allfail_case()
    assert exp["n_escalated"] == len(rows)
    out = check(dec8, rows, exp, "all fail")
    np.testing.assert_array_equal(out["best_bits"], exp["list_bits"])  # plain L = 8 exactly
    np.testing.assert_array_equal(out["best_idx"], exp["list_idx"])
    np.testing.assert_array_equal(out["crc_pass"], exp["list_ok"])


@pytest.fixture(scope="module")
def deferred_case():
    """Rows the screening pass must defer (ties: values of +-1 and small integers, the corner
    construction of test_gpu_adaptive.py) that fail the SC stage's CRC, each followed by two rows
    that pass it: an escalated frame's position in the row list differs from its row number."""
    info = ac.info_set(128, 64)
    rng = np.random.default_rng(4242)
    a = rng.choice([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], size=(96, 128))
    b = rng.choice([-1.0, 1.0], size=(64, 128))
    ties = np.concatenate([a, b])
    good, gexp = ac.allpass_case()
    rows = np.empty((3 * len(ties), 128))
    rows[0::3] = ties
    rows[1::3] = good[:len(ties)]
    rows[2::3] = good[len(ties):2 * len(ties)]
    exp = ac.compose(rows, info, 8, ac.POLY24)
    esc = np.flatnonzero(exp["stage"] == 2)
    assert len(esc) > 100 and np.all(exp["stage"][1::3] == 1)
    assert np.count_nonzero(esc != np.arange(len(esc))) > 100  # list position != row
    return rows, exp


@pytest.mark.parametrize("L", [8, 4])
def test_deferred_frames_are_listed_by_row(L, deferred_case, dec8, dec4):
    rows, exp8 = deferred_case
    dec = dec8 if L == 8 else dec4
    exp = exp8 if L == 8 else ac.compose(rows, ac.info_set(128, 64), 4, ac.POLY24)
    # sentinel outputs: a re-decode that lands on a list position instead of a row leaves rows unwritten
    dec.adaptive_stats(reset=True)
    out = run_async(dec, rows, prefill=0x5A)
    assert dec.screening_count() > 0
    ac.assert_equals(out, exp, f"deferred L={L}")
    assert out["n_escalated"] == exp["n_escalated"]
    assert dec.adaptive_stats()["screened"] == 1


def test_nr_rate_matched():
    rows, exp = ac.nr_case()
    dec = _native.Decoder(128, ac.info_set(128, 88), 8, ac.POLY24)
    dec.set_rate_match(256)
    check(dec, rows, exp, "NR (128,88) E=256")


def test_rate_matched_E100():
    info, B, E = ac.info_set(128, 64), 300, 100
    rows = ac.make_llr(80 + E, B, info, ac.POLY24, 5.0, E=E)
    exp = ac.compose(rows, info, 4, ac.POLY24, E=E)
    dec = _native.Decoder(128, info, 4, ac.POLY24)
    dec.set_rate_match(E)
    # (the (128,64) code on rate-matched rows has no lane-per-path screening kernel: the plain decode
    # of this handle is exact too)
    check(dec, rows, exp, "(128,64) E=100", path="exact")


def test_runtime_info_set_and_crc16():
    """(128,40) + CRC-16 at L = 4: the run-time-set lane kernel at n = 7, its row-list branch."""
    info, B = ac.info_set(128, 40), 2051
    rows = ac.make_llr(78, B, info, ac.POLY16, 3.0)
    exp = ac.compose(rows, info, 4, ac.POLY16)
    assert 0 < exp["n_escalated"] < B
    check(_native.Decoder(128, info, 4, ac.POLY16), rows, exp, "(128,40) CRC-16")


@pytest.mark.parametrize("name,L", [("pw256", 8), ("pw512", 8), ("pw1024", 8), ("pw256", 16)])
def test_long_codes(name, L):
    case = sg.mixed_case(name, L)
    assert 0 < case["exp"]["n_escalated"] < len(case["rows"])
    dec = _native.Decoder(case["N"], case["info"], L, case["crc"])
    check(dec, case["rows"], case["exp"], f"{name} L={L}")


@pytest.mark.parametrize("name", ["c32", "c64"])
def test_short_codes_take_the_exact_kernel(name):
    case = sg.mixed_case(name, 8)
    assert 0 < case["exp"]["n_escalated"] < len(case["rows"])
    dec = _native.Decoder(case["N"], case["info"], 8, case["crc"])
    check(dec, case["rows"], case["exp"], name, path="exact")


def test_list_size_2_takes_the_exact_kernel():
    info = ac.info_set(128, 64)
    rows = ac.mixed_rows()[:1500]
    exp = ac.compose(rows, info, 2, ac.POLY24)
    check(_native.Decoder(128, info, 2, ac.POLY24), rows, exp, "L=2", path="exact")


def test_screening_off_takes_the_exact_kernel():
    dec = _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    dec.set_screening(False)
    check(dec, ac.mixed_rows()[:1500], ac.mixed_expected(8), "screening off", slice(0, 1500), path="exact")


@pytest.mark.parametrize("name", ["n128", "pw256"])
def test_capped_grid_strides_over_the_list(name):
    """The row-list launch is sized for B by default, so no batch here exceeds one grid pass; with
    the workgroup cap of the tuning knob the same kernels stride over the list (8 frames per
    workgroup at L = 8: 16 workgroups take 128 frames per pass, one workgroup 8).  Results do not change."""
    if name == "n128":
        rows, exp = ac.allfail_case()
        dec = _native.Decoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    else:
        case = sg.mixed_case(name, 8)
        rows, exp = case["rows"], case["exp"]
        dec = _native.Decoder(case["N"], case["info"], 8, case["crc"])
    cap = 16 if name == "n128" else 1
    assert exp["n_escalated"] > cap * 8, (exp["n_escalated"], cap)  # (the oracle: 1000 and 10 frames)
    dec.set_tuning(adapt_grid=cap)
    check(dec, rows, exp, f"{name}, {cap} workgroups")


def test_counters_with_reference(dec8):
    rows, exp = ac.mixed_rows(), ac.mixed_expected(8)
    kp = 40
    rng = np.random.default_rng(99)
    ref = exp["list_bits"] ^ (rng.random(exp["list_bits"].shape) < 0.01).astype(np.int8)
    want = sg.host_counts(exp["best_bits"], exp["crc_pass"], ref, kp, NC, escalated=exp["n_escalated"])
    out = run_async(dec8, rows, ref_bits=ref, kp=kp)
    np.testing.assert_array_equal(out["counters"], want)
    assert out["n_escalated"] == exp["n_escalated"]
    np.testing.assert_array_equal(run_async(dec8, rows)["counters"], np.zeros(NC, np.int64))  # untouched without d_ref


def test_scratch_reuse_back_to_back(dec8):
    """Two different batches on one handle with no synchronisation in between."""
    r1, e1 = ac.mixed_rows(), ac.mixed_expected(8)
    r2, e2 = ac.allfail_case()
    with _native.DeviceArena(dec8) as mem:
        bufs = []
        for r in (r1, r2):
            B = len(r)
            d = dict(llr=mem.alloc(r.nbytes), best=mem.alloc(B * 8), flags=mem.alloc(B), stage=mem.alloc(B), n=mem.alloc(8))
            mem.upload(d["llr"], r)
            bufs.append(d)
        for r, d in zip((r1, r2), bufs):
            dec8.adaptive_async_device(d["llr"], len(r), d_best=d["best"], d_flags=d["flags"], d_stage=d["stage"],
                                       d_n_escalated=d["n"])
        dec8.sync()
        for (r, e, d) in ((r1, e1, bufs[0]), (r2, e2, bufs[1])):
            _compare(mem, d, len(r), e, 64, "back to back")


def _compare(mem, d, B, exp, K, tag, cnt=None, want_cnt=None):
    words = mem.download(d["best"], B * 8 * ((K + 63) // 64), np.uint64).reshape(B, -1)
    flags = mem.download(d["flags"], B, np.uint8)
    out = {"best_bits": _bits(words, K), "crc_pass": (flags & 0x80) != 0, "best_idx": (flags & 0x3F).astype(np.int32),
           "stage": mem.download(d["stage"], B, np.uint8)}
    ac.assert_equals(out, exp, tag)
    assert int(mem.download(d["n"], 8, np.int32)[0]) == exp["n_escalated"], tag
    if cnt is not None:
        np.testing.assert_array_equal(mem.download(cnt, 8 * NC, np.int64), want_cnt, err_msg=tag)


def _pipelined_batches(N):
    if N == 128:
        info, crc, K = ac.info_set(128, 64), ac.POLY24, 64
        (r2, e2), (r3, e3) = ac.allfail_case(), ac.allpass_case()
        return info, crc, K, [(ac.mixed_rows(), ac.mixed_expected(8)), (r2, e2), (r3, e3)]
    case = sg.mixed_case("pw256", 8)
    rows, exp = case["rows"], case["exp"]
    h = {k: exp[k][:130] for k in ("best_bits", "crc_pass", "best_idx", "stage")}
    h["n_escalated"] = int(np.count_nonzero(h["stage"] == 2))
    rev = {k: exp[k][::-1] for k in ("best_bits", "crc_pass", "best_idx", "stage")}
    rev["n_escalated"] = exp["n_escalated"]
    return case["info"], case["crc"], 128, [(rows, exp), (rows[:130], h), (np.ascontiguousarray(rows[::-1]), rev)]


@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("depth", [1, 2])
def test_pipelined_equals_plain(depth, N):
    """Three consecutive calls on different batches with distinct buffers on a pipelined handle,
    read after pscl_join: outputs and counters equal the oracle's (the non-pipelined form's)."""
    info, crc, K, batches = _pipelined_batches(N)
    kp = K - 24
    dec = _native.Decoder(N, info, 8, crc)
    with _native.DeviceArena(dec) as mem:
        bufs, wants = [], []
        for r, e in batches:
            B = len(r)
            d = dict(llr=mem.alloc(r.nbytes), best=mem.alloc(B * 8 * dec.W), flags=mem.alloc(B), stage=mem.alloc(B),
                     n=mem.alloc(8), ref=mem.alloc(B * 8 * dec.W), cnt=mem.alloc(8 * NC))
            mem.upload(d["llr"], r)
            mem.upload(d["ref"], sg.words(e["list_bits"] if "list_bits" in e else e["best_bits"]))
            mem.memset(d["cnt"], 0, 8 * NC)
            ref = e["list_bits"] if "list_bits" in e else e["best_bits"]
            wants.append(sg.host_counts(e["best_bits"], e["crc_pass"], ref[:B], kp, NC, escalated=e["n_escalated"]))
            bufs.append(d)
        dec.set_pipelined(True, depth=depth)
        try:
            for (r, e), d in zip(batches, bufs):
                dec.adaptive_async_device(d["llr"], len(r), d_best=d["best"], d_flags=d["flags"], d_stage=d["stage"],
                                          d_ref=d["ref"], k_payload=kp, d_counters=d["cnt"], d_n_escalated=d["n"])
            dec.join()
            dec.sync()
        finally:
            dec.set_pipelined(False)
        for i, ((r, e), d) in enumerate(zip(batches, bufs)):
            _compare(mem, d, len(r), e, K, f"pipelined depth {depth} N={N} call {i}", d["cnt"], wants[i])


def test_no_host_wait_after_warm_up(dec8):
    rows = ac.mixed_rows()
    run_async(dec8, rows)  # warm-up: scratch of this B
    dec8.adaptive_stats(reset=True)
    for _ in range(3):
        run_async(dec8, rows)
    st = dec8.adaptive_stats()
    assert st["host_waits"] == 0 and st["screened"] == 3, st


def test_errors():
    info = ac.info_set(128, 64)
    dec = _native.Decoder(128, info, 8, ac.POLY24)
    with pytest.raises(ValueError):  # no CRC
        _native.Decoder(128, info, 8, None).adaptive_async_device(1, 1, d_best=1, d_flags=1)
    with pytest.raises(ValueError):
        dec.adaptive_async_device(1, -1, d_best=1, d_flags=1)
    with pytest.raises(ValueError):
        dec.adaptive_async_device(1, 1, d_best=1, d_flags=1, d_ref=1, d_counters=0)
    for miss in ("d_llr", "d_best", "d_flags"):
        kw = dict(d_llr=1, d_best=1, d_flags=1)
        kw[miss] = 0
        with pytest.raises(ValueError):
            dec.adaptive_async_device(kw.pop("d_llr"), 1, **kw)
    with pytest.raises(NotImplementedError):
        _native.Decoder(16, ac.info_set(16, 12), 4, sg.POLY8).adaptive_async_device(1, 1, d_best=1, d_flags=1)
    with pytest.raises(NotImplementedError):
        d = _native.Decoder(256, ac.info_set(256, 128), 4, ac.POLY24)
        d.set_rate_match(300)
        d.adaptive_async_device(1, 1, d_best=1, d_flags=1)
    with pytest.raises(NotImplementedError):
        dec.adaptive_async_device(1, 2 ** 31, d_best=1, d_flags=1)
    dec.adaptive_async_device(0, 0, d_best=0, d_flags=0)  # B = 0 is fine


# ---- the sweep

def _sim_expected(dec, info, crc, L, N, seed, sid, ebno, frame0, B, include_uncoded):
    """Regenerate the rows and messages of the frame range with channel_device, then the oracle's
    composition on the host: the three counter rows."""
    K, W = len(info), dec.W
    kp = K - (oracle.poly_int(crc).bit_length() - 1)
    with _native.DeviceArena(dec) as mem:
        d_llr, d_msg, d_unc = mem.alloc(B * N * 8), mem.alloc(B * W * 8), mem.alloc(8 * NC)
        mem.memset(d_unc, 0, 8 * NC)
        dec.channel_device(seed, sid, ebno, K / N, kp, frame0, B, d_llr, d_msg)
        if include_uncoded:
            dec.uncoded_device(seed, sid, ebno, kp, frame0, B, d_unc)
        dec.sync()
        rows = mem.download(d_llr, B * N * 8, np.float64).reshape(B, N)
        msg = _bits(mem.download(d_msg, B * W * 8, np.uint64).reshape(B, W), K)
        unc = mem.download(d_unc, 8 * NC, np.int64)
    exp = ac.compose(rows, info, L, crc, N=N)
    want = np.zeros((3, NC), np.int64)
    want[0] = sg.host_counts(exp["sc_bits"], exp["sc_ok"], msg, kp, NC)
    want[1] = sg.host_counts(exp["best_bits"], exp["crc_pass"], msg, kp, NC, escalated=exp["n_escalated"])
    want[2] = unc
    return want, kp


@pytest.mark.parametrize("ebno", [3.0, 5.0])
def test_simulate_adaptive_two_shards(ebno, dec8):
    info, seed, sid = ac.info_set(128, 64), 2025, 51
    shards = [(0, 3000), (3000, 2987)]  # (the second: an offset, and no multiple of 64)
    total = np.zeros((3, NC), np.int64)
    with _native.DeviceArena(dec8) as mem:
        d_cnt = mem.alloc(3 * NC * 8)
        mem.memset(d_cnt, 0, 3 * NC * 8)
        for f0, B in shards:
            want, kp = _sim_expected(dec8, info, ac.POLY24, 8, 128, seed, sid, ebno, f0, B, True)
            total += want
            np.testing.assert_array_equal(dec8.simulate_adaptive(seed, sid, ebno, 0.5, kp, f0, B, True), want)
            dec8.simulate_adaptive_device(seed, sid, ebno, 0.5, kp, f0, B, True, d_cnt)
        dec8.sync()
        np.testing.assert_array_equal(mem.download(d_cnt, 3 * NC * 8, np.int64).reshape(3, NC), total)
    assert 0 < total[1, _native.CNT_ESCALATED] < total[1, 0] and total[2, 0] == total[0, 0] == 5987


def test_simulate_adaptive_n256():
    info = sg.pw_info_set(256, 128)
    dec = _native.Decoder(256, info, 4, ac.POLY24)
    want, kp = _sim_expected(dec, info, ac.POLY24, 4, 256, 7, 30, 2.5, 500, 1003, False)
    got = dec.simulate_adaptive(7, 30, 2.5, 0.5, kp, 500, 1003, False)
    np.testing.assert_array_equal(got, want)
    assert 0 < want[1, _native.CNT_ESCALATED] < 1003


def test_simulate_adaptive_chunks_add_up(dec8):
    """One call of 2^20 + 77 frames (two chunks) equals the sum of two calls split at 2^20."""
    n0, n1 = 1 << 20, 77
    one = dec8.simulate_adaptive(11, 50, 5.0, 0.5, 40, 0, n0 + n1, True)
    two = dec8.simulate_adaptive(11, 50, 5.0, 0.5, 40, 0, n0, True) + dec8.simulate_adaptive(11, 50, 5.0, 0.5, 40, n0, n1, True)
    np.testing.assert_array_equal(one, two)
    assert one[0, 0] == one[1, 0] == one[2, 0] == n0 + n1 and 0 < one[1, _native.CNT_ESCALATED] < n0


def test_cli_csv_row_equals_counters(tmp_path):
    from polar_code_amd import config
    from polar_code_amd.eval import run_adaptive_sweep as ras
    from polar_code_amd.utils.seeding import philox_stream_id

    cfg = config.get_config()
    frames, snr = 3001, 5.0
    args = ras.build_argparser().parse_args(["--M", "8", "--frames", str(frames), "--snr_lo", str(snr), "--snr_hi", str(snr),
                                             "--snr_step", "0", "--seed", "3", "--include_uncoded", "--out_dir", str(tmp_path)])
    ras.run_sweep(args)
    lines = (tmp_path / "fer_adaptive_M8.csv").read_text().splitlines()
    assert lines[0].split(",") == ras.csv_header(True) and len(lines) == 2
    kp = cfg.K - cfg.crc_bits
    dec = _native.Decoder(cfg.N, oracle.construct_info_set(cfg.N, cfg.K), 8, cfg.crc_poly)
    cnt = dec.simulate_adaptive(3, philox_stream_id(snr), snr, cfg.K / cfg.N, kp, 0, frames, True)
    row = ras.row_from_counters(snr, cnt, frames, cfg.K, kp, True)
    want = ",".join(f"{row[k]:.3f}" if k == "snr_db" else f"{row[k]:.6e}" for k in ras.csv_header(True))
    assert lines[1] == want
    got = dict(zip(lines[0].split(","), map(float, lines[1].split(","))))
    assert got["fer_adaptive"] == pytest.approx(cnt[1, _native.CNT_FRAME_ERR] / frames, rel=1e-6)
    assert got["escalated"] == pytest.approx(cnt[1, _native.CNT_ESCALATED] / frames, rel=1e-6)
    assert got["fer_sc"] == pytest.approx(cnt[0, _native.CNT_FRAME_ERR] / frames, rel=1e-6)


def test_tensor_entry_on_a_side_stream():
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    rows, exp = ac.mixed_rows()[:1500], ac.mixed_expected(8)
    dec = SCLDecoder(128, ac.info_set(128, 64), 8, ac.POLY24)
    host = dec.decode_adaptive(rows)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        llr = torch.from_numpy(rows.copy()).to("cuda")
        best, flags, stage, n_esc = dec.decode_tensor_adaptive_async(llr)
    stream.synchronize()
    flags, stage = flags.cpu().numpy(), stage.cpu().numpy()
    np.testing.assert_array_equal(best.cpu().numpy().view(np.uint64), sg.words(host["bits"]))
    np.testing.assert_array_equal((flags & _native.PSCL_FLAG_CRC_PASS) != 0, host["crc_pass"])
    np.testing.assert_array_equal(flags & _native.PSCL_FLAG_IDX_MASK, host["best_idx"])
    np.testing.assert_array_equal(stage, host["stage"])
    assert n_esc.dtype == torch.int32 and n_esc.shape == (1,) and int(n_esc.cpu()[0]) == host["n_escalated"]
    np.testing.assert_array_equal(host["bits"], exp["best_bits"][:1500])
    dec.native.set_stream(None)
