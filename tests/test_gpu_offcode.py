"""GPU: the decoders and the TX chain off the project's CRC and off constructed information sets.

Part 1 -- the compiled-in (128,64) and (128,88)/E = 256 information sets under CRCs of degree 1, 6,
11, 16, 24 (not the project's polynomial), 32 and under none.  spec_code() picks the compiled-in
kernels (scl_lane_kernel, the scl128_spec instances, sc128_lane, the DL-SCL retry instances, the
fused TX, every float32 form) from K and the information mask alone, so these handles run them with
other syndrome tables, crc_deg, k_payload and has_crc.
Part 2 -- the list decoders on offcode_cases.info_family: position 0, without N - 1, K = N,
16-position blocks, a list that fills at the last phase (K = log2 L) or never (n_paths < L).

Expected values come from the oracle (offcode_cases.py, pinned to the reference by golden g17) and
the host mirrors of the NR front end (encode_cases.expected, test_gpu_channel.host_stream), never
from the code under test.  Outputs of the device paths land in sentinel-filled buffers with a guard
row behind them."""
import numpy as np
import pytest

import adaptive_cases as ac
import offcode_cases as oc
import oracle
from dl_short_cases import host_counts as dl_counts
from encode_cases import crc_degree, info_set, unpack
from polar_code_amd import _native
from polar_code_amd.dlscl.flip import decode_with_retries_device
from staged_cases import host_counts
from test_gpu_encode import Out, check_outputs, reference, run_encode, upload

pytestmark = pytest.mark.gpu

U64 = np.uint64
NC = _native.PSCL_NCOUNT
PLAIN = dict(want_metrics=False, want_cands=False, want_info_llrs=False)
CRC_IDS = dict(ids=oc.crc_id)


def handle(code, L, crc, screening=True):
    K, E = oc.CODES[code]
    dec = _native.Decoder(128, ac.info_set(128, K), L, crc)
    if E:
        dec.set_rate_match(E)
    dec.set_screening(screening)
    return dec


def assert_plain(out, exp, tag, n_paths):
    for k in ("best_bits", "crc_pass", "best_idx"):
        np.testing.assert_array_equal(out[k], exp[k], err_msg=f"{tag}: {k}")
    assert np.all(out["n_paths"] == n_paths), (tag, out["n_paths"])


def run_device(dec, rows, *, f32=False, ref=None, kp=0):
    """decode_device[_f32] on host rows -> (bits [B, K], flags [B], counters [NC] or None)."""
    B = rows.shape[0]
    with _native.DeviceArena(dec) as mem:
        d_llr = upload(mem, rows)
        best, flags = Out(mem, B, dec.W, U64), Out(mem, B, 1, np.uint8)
        d_ref = d_cnt = 0
        if ref is not None:
            d_ref, d_cnt = upload(mem, oc.words(ref)), mem.alloc(NC * 8)
            mem.memset(d_cnt, 0, NC * 8)
        call = dec.decode_device_f32 if f32 else dec.decode_device
        call(d_llr, B, d_best=best.ptr, d_flags=flags.ptr, d_ref=d_ref, k_payload=kp, d_counters=d_cnt)
        dec.sync()
        cnt = mem.download(d_cnt, NC * 8, np.int64) if d_cnt else None
        return unpack(best.get(), dec.K), flags.get()[:, 0], cnt


def assert_flags(bits, flags, exp, tag):
    np.testing.assert_array_equal(bits, exp["best_bits"], err_msg=f"{tag}: best_bits")
    np.testing.assert_array_equal((flags & _native.PSCL_FLAG_CRC_PASS) != 0, exp["crc_pass"], err_msg=f"{tag}: crc_pass")
    np.testing.assert_array_equal(flags & _native.PSCL_FLAG_IDX_MASK, exp["best_idx"], err_msg=f"{tag}: best_idx")


# ------------------------------------------------------------------ part 1: compiled-in sets, other CRCs

@pytest.mark.parametrize("crc", oc.CRCS, **CRC_IDS)
@pytest.mark.parametrize("code", list(oc.CODES))
def test_plain_decode_under_every_crc(code, crc):
    rows = oc.crc_rows(code, crc)[0]
    for L in (1, 2, 4, 8):
        exp = oc.crc_plain(code, crc, L)
        for screening in (True, False):
            dec = handle(code, L, crc, screening)
            tag = f"{code} {oc.crc_id(crc)} L={L} screening={screening}"
            out = dec.decode(rows, **PLAIN)
            assert_plain(out, exp, tag, L)
            if crc is None:
                assert out["crc_pass"].all() and not out["best_idx"].any(), tag
            if screening and L >= 4:  # the lane kernel ran: it defers the exact ties, and little else
                dec.decode(rows[oc.TIES], **PLAIN)
                n_ties = dec.screening_count()
                dec.decode(rows[oc.AWGN], **PLAIN)
                n_awgn = dec.screening_count()
                print(f"{tag}: screening_count {n_ties} of {oc.ROUNDED} rounded rows, {n_awgn} of {3 * oc.PER_POINT} AWGN rows")
                assert n_ties > 0, tag
                assert n_awgn < 3 * oc.PER_POINT // 4, tag
            dec.close()


@pytest.mark.parametrize("crc", oc.CRCS, **CRC_IDS)
@pytest.mark.parametrize("code", list(oc.CODES))
def test_full_outputs_under_every_crc(code, crc):
    dec = handle(code, 8, crc)
    out = dec.decode(oc.crc_rows(code, crc)[0][oc.FULL])
    oc.assert_full(out, oc.crc_full(code, crc), f"{code} {oc.crc_id(crc)}", llr_bits=False)
    best = oc.crc_full(code, crc)["cands"][np.arange(len(oc.FULL)), oc.crc_full(code, crc)["best_idx"]]
    want = np.array([oracle.check_crc(b, crc) if crc else True for b in best], bool)
    np.testing.assert_array_equal(out["crc_pass"], want)
    dec.close()


@pytest.mark.parametrize("crc", oc.CRCS, **CRC_IDS)
@pytest.mark.parametrize("code", list(oc.CODES))
def test_float32_rows_under_every_crc(code, crc):
    for L in (4, 8):
        rows32, exp = oc.crc_f32(code, crc, L)
        dec = handle(code, L, crc)
        assert dec.f32_available(), (code, crc, L)
        bits, flags, _ = run_device(dec, rows32, f32=True)
        assert_flags(bits, flags, exp, f"{code} {oc.crc_id(crc)} L={L} float32")
        dec.close()


@pytest.mark.parametrize("crc", oc.CRCS, **CRC_IDS)
@pytest.mark.parametrize("code", list(oc.CODES))
def test_counters_take_k_payload_from_the_crc_degree(code, crc):
    """d_ref with k_payload = K - degree: frame, bit, payload-frame and payload-bit errors of the
    screened and the exact decode equal counts formed on the host from the oracle's results."""
    K, _ = oc.CODES[code]
    rows, msg, _ = oc.crc_rows(code, crc)
    kp = K - oc.degree(crc)
    for L in (4, 8):
        exp = oc.crc_plain(code, crc, L)
        want = host_counts(exp["best_bits"], exp["crc_pass"], msg, kp, NC)
        assert want[3] > 0 and (crc is None or want[2] > want[4])  # (payload errors, and errors in the CRC bits)
        for screening in (True, False):
            dec = handle(code, L, crc, screening)
            bits, flags, cnt = run_device(dec, rows, ref=msg, kp=kp)
            tag = f"{code} {oc.crc_id(crc)} L={L} screening={screening}"
            assert_flags(bits, flags, exp, tag)
            np.testing.assert_array_equal(cnt[:5], want[:5], err_msg=tag)
            dec.close()


def run_adaptive_async(dec, rows):
    B = rows.shape[0]
    with _native.DeviceArena(dec) as mem:
        d_llr = upload(mem, rows)
        best, flags, stage, n = Out(mem, B, dec.W, U64), Out(mem, B, 1, np.uint8), Out(mem, B, 1, np.uint8), Out(mem, 1, 1, np.int32)
        dec.adaptive_async_device(d_llr, B, d_best=best.ptr, d_flags=flags.ptr, d_stage=stage.ptr, d_n_escalated=n.ptr)
        dec.sync()
        f = flags.get()[:, 0]
        return {"best_bits": unpack(best.get(), dec.K), "crc_pass": (f & _native.PSCL_FLAG_CRC_PASS) != 0,
                "best_idx": (f & _native.PSCL_FLAG_IDX_MASK).astype(np.int32), "stage": stage.get()[:, 0],
                "n_escalated": int(n.get()[0, 0])}


@pytest.mark.parametrize("crc", oc.NONEMPTY)
@pytest.mark.parametrize("code", list(oc.CODES))
def test_adaptive_composition_under_every_crc(code, crc):
    """SC where it passes the CRC, else the list decoder -- also where a 1- or 6-bit CRC passes wrong
    SC results."""
    rows = oc.crc_rows(code, crc)[0]
    for L in (4, 8):
        exp = oc.crc_adaptive(code, crc, L)
        dec = handle(code, L, crc)
        for name, out in (("host", dec.decode_adaptive(rows)), ("async", run_adaptive_async(dec, rows))):
            ac.assert_equals(out, exp, f"{code} {crc} L={L} {name}")
            assert out["n_escalated"] == exp["n_escalated"], (code, crc, L, name)
        dec.close()


@pytest.mark.parametrize("with_beta", [False, True], ids=["none", "beta_M8"])
@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("crc", oc.NONEMPTY)
def test_dl_loop_under_every_crc(crc, L, with_beta):
    rows, msg = oc.dl_rows(crc)
    exp = oc.dl_case(crc, L, with_beta)
    info = ac.info_set(128, 64)
    dev = decode_with_retries_device(rows, info, L, oc.DL_RETRIES, crc=crc, beta=oc.beta_m8() if with_beta else None, msg=msg)
    tag = f"{crc} L={L} beta={with_beta}"
    for k in ("base_pass", "base_bits", "attempts", "success", "best_bits"):
        np.testing.assert_array_equal(np.asarray(dev[k]), exp[k], err_msg=f"{tag}: {k}")
    np.testing.assert_array_equal(dev["tried"][exp["every"]], exp["tried"], err_msg=f"{tag}: tried")
    # (every frame's tried row is as long as its attempts say)
    np.testing.assert_array_equal((dev["tried"] >= 0).sum(axis=1), exp["attempts"] - 1, err_msg=f"{tag}: tried length")
    kp = 64 - oc.degree(crc)
    assert [int(v) for v in dev["counters"]["scl"][:6]] == dl_counts(exp["base_bits"], exp["base_pass"], msg, kp), tag
    assert [int(v) for v in dev["counters"]["dl"][:6]] == dl_counts(exp["best_bits"], exp["success"], msg, kp,
                                                                    int((exp["attempts"] - 1).sum())), tag
    _native.release_decoders()


def test_without_a_crc_the_refusals_stay():
    rows = oc.crc_rows("k64", None)[0][:8]
    dec = handle("k64", 8, None)
    with pytest.raises(ValueError, match="needs a CRC"):
        dec.decode_adaptive(rows)
    with _native.DeviceArena(dec) as mem:
        d_llr, d_best, d_flags = upload(mem, rows), mem.alloc(64), mem.alloc(8)
        mem.memset(d_flags, 0, 8)
        with pytest.raises(ValueError, match="needs a CRC"):
            dec.adaptive_async_device(d_llr, 8, d_best=d_best, d_flags=d_flags)
        with pytest.raises(ValueError, match="needs a CRC"):
            dec.escalate_device(d_llr, 8, d_best=d_best, d_flags=d_flags)
        with pytest.raises(ValueError, match="need a CRC"):
            dec.retry_device(d_llr, 8, 8, d_best=d_best, d_flags=d_flags)
    dec.close()


# ---- TX

ENCODE_CODES = [(128, 64, 0), (128, 88, 0), (128, 88, 201), (256, 140, 0)]


@pytest.mark.parametrize("crc", oc.NONEMPTY)
@pytest.mark.parametrize("N,K,E", ENCODE_CODES)
def test_encode_device_places_every_remainder(N, K, E, crc):
    _, words, msg, tx = reference(N, K, crc, E)
    dec = _native.Decoder(N, info_set(N, K), 2, crc)
    if E:
        dec.set_rate_match(E)
    assert dec.k_payload == K - crc_degree(crc)
    for B in (65, 257):
        check_outputs(dec, run_encode(dec, words, B), B, msg, tx)
    dec.close()


@pytest.mark.parametrize("crc", [None, "0x11021", "0x104C11DB7"], **CRC_IDS)
@pytest.mark.parametrize("N,K", [(128, 64), (256, 128)])
def test_channel_message_words_under_other_crcs(N, K, crc):
    from test_gpu_channel import host_stream

    info = info_set(N, K)
    dec = _native.Decoder(N, info, 2, crc)
    kp = K - oc.degree(crc)
    B, frame0, seed, sid = 67, 987654321, 0x1234ABCD5678, 42
    with _native.DeviceArena(dec) as mem:
        llr, words = Out(mem, B, N, np.float64), Out(mem, B, dec.W, U64)
        dec.channel_device(seed, sid, 3.0, K / N, kp, frame0, B, llr.ptr, words.ptr)
        dec.sync()
        got, rows = unpack(words.get(), K), llr.get()
    msg, _ = host_stream(seed, sid, frame0, B, N, info, K, kp, crc, 3.0, K / N)
    np.testing.assert_array_equal(got, msg)
    assert np.isfinite(rows).all() and rows.std() > 0.5
    dec.close()


@pytest.mark.parametrize("crc", [None, "0x11021"], **CRC_IDS)
def test_fused_tx_simulate_equals_unfused_under_other_crcs(crc):
    kp, B = 64 - oc.degree(crc), 599
    out = {}
    for fused in (1, 0):
        dec = _native.Decoder(128, ac.info_set(128, 64), 8, crc)
        dec.set_tuning(tx_fused=fused)
        out[fused] = dec.simulate(5, 11, 2.0, 0.5, kp, 1000, B, 8 if crc else 0, include_uncoded=True)
        assert (dec.path_stats()["fused_tx_blocks"] > 0) == bool(fused)
        dec.close()
    np.testing.assert_array_equal(out[1], out[0])
    assert out[1][0][0] == B and out[1][0][2] > 0  # (bit errors: the comparison bites)


# ------------------------------------------------------------------ part 2: the information-set family

@pytest.mark.parametrize("N,L", oc.FULL_SHAPES + [(512, 8), (1024, 8)])
def test_family_full_outputs(N, L):
    for name in oc.family_names(N, L):
        c = oc.family_case(N, name, L)
        dec = _native.Decoder(N, c["info"], L, c["crc"])
        out = dec.decode(c["rows"])
        tag = f"N={N} L={L} {name}"
        oc.assert_full(out, c["exp"], tag, llr_bits=False)
        np.testing.assert_array_equal(out["crc_pass"], c["crc_pass"], err_msg=f"{tag}: crc_pass")
        K = len(c["info"])
        assert np.all(out["n_paths"] == oc.expected_paths(K, L)), tag
        if name == "short" or (name == "first_only" and L > 2):  # the list never fills
            assert np.all(out["n_paths"] == 2 ** K) and 2 ** K < L, tag
        dec.close()


@pytest.mark.parametrize("N,L", [(N, L) for N in (128, 256) for L in (4, 8, 16, 32)] + [(512, 8), (1024, 8)])
def test_family_plain_outputs_screened(N, L):
    for name in oc.family_names(N, L, every=True):
        c = oc.family_case(N, name, L)
        dec = _native.Decoder(N, c["info"], L, c["crc"])
        out = dec.decode(c["rows"], **PLAIN)
        n_all = dec.screening_count()
        tag = f"N={N} L={L} {name}"
        exp = {"best_bits": c["best_bits"], "crc_pass": c["crc_pass"], "best_idx": c["exp"]["best_idx"]}
        assert_plain(out, exp, tag, oc.expected_paths(len(c["info"]), L))
        if name == "fills_last":  # the lane kernel took K = log2 L
            dec.decode(c["rows"][oc.family_ties(N)], **PLAIN)
            n_ties = dec.screening_count()
            print(f"{tag}: screening_count {n_ties} of {oc.FAMILY_HALF[N]} rounded rows ({n_all} of the batch)")
            assert n_ties > 0, tag
        elif name == "short":  # K < log2 L: the guard sent it to the exact kernel
            print(f"{tag}: screening_count {n_all}")
            assert n_all == 0, tag
        else:
            print(f"{tag}: screening_count {n_all} of {len(c['rows'])}")
        dec.close()


@pytest.mark.parametrize("name", ["head", "all", "random"])
def test_family_path_llrs_replay(name):
    c = oc.family_case(128, name, 8)
    dec = _native.Decoder(128, c["info"], 8, c["crc"])
    out = dec.decode(c["rows"])
    f = np.arange(len(c["rows"]))
    got = dec.path_llrs(c["rows"], out["best_bits"])
    want = np.ascontiguousarray(out["info_llrs"][f, out["best_idx"]])
    # (by value: the sign of a zero decision LLR is not the reference's, offcode_cases.assert_full)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(want, c["exp"]["info_llrs"][f, c["exp"]["best_idx"]])
    dec.close()
