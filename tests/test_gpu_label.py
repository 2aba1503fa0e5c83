"""pscl_label_device on the GPU against the oracle's composition of its contract (label_cases.py):
every case, both sent_stride forms, the capacity protocol, empty and all-pass batches, a pipelined
handle, scratch reuse across calls, the tensor method and make_dataset --label native."""
import json

import numpy as np
import pytest

from polar_code_amd import _native
from polar_code_amd.train import make_dataset as md

import label_cases as lc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SENT = 0x5A  # byte the output arrays are filled with before a call


def _decoder(name):
    c = lc.CASES[name]
    return _native.get_decoder(c.N, lc.info_of(name), c.L, c.crc, 0, c.E)


def run_device(dec, rows, sent, cap=None, max_flips=8, with_rank=True):
    """One raw pscl_label_device call on sentinel-filled outputs of `cap` rows.  Returns (A or the
    LabelCapacity raised, the raw arrays of cap rows, counts)."""
    rows = np.ascontiguousarray(rows, np.float64)
    B, K = rows.shape[0], dec.K
    words, stride = _native._sent_words(sent, B, K, dec.W)
    cap = B if cap is None else cap
    n = max(cap, 1)
    with _native.DeviceArena(dec) as mem:
        d_llr, d_sent = mem.alloc(max(rows.nbytes, 8)), mem.alloc(words.nbytes)
        if B:
            mem.upload(d_llr, rows)
        mem.upload(d_sent, words)
        size = {"frame": n * 8, "abs_l0": n * K * 4, "flip": n * 4, "rank": n * 4, "counts": 32}
        d = {k: mem.alloc(v) for k, v in size.items()}
        for k in d:
            mem.memset(d[k], SENT, size[k])
        try:
            A = dec.label_device(d_llr, B, d_sent, stride, max_flips, cap, d_frame=d["frame"], d_abs_l0=d["abs_l0"],
                                 d_flip=d["flip"], d_rank=d["rank"] if with_rank else 0, d_counts=d["counts"])
        except _native.LabelCapacity as e:
            A = e
        dec.sync()
        raw = {"frame": mem.download(d["frame"], size["frame"], np.int64),
               "abs_l0": mem.download(d["abs_l0"], size["abs_l0"], np.float32).reshape(n, K),
               "flip": mem.download(d["flip"], size["flip"], np.int32),
               "rank": mem.download(d["rank"], size["rank"], np.int32),
               "counts": mem.download(d["counts"], 32, np.int64)}
    return A, raw


def untouched(a, start=0):
    return bool(np.all(np.ascontiguousarray(a[start:]).view(np.uint8) == SENT))


def sorted_entries(A, raw):
    o = np.argsort(raw["frame"][:A], kind="stable")
    return {"frame": raw["frame"][:A][o], "abs_l0": raw["abs_l0"][:A][o], "flip": raw["flip"][:A][o],
            "rank": raw["rank"][:A][o], "counts": raw["counts"]}


def check(dec, rows, sent, exp, tag, cap=None):
    A, raw = run_device(dec, rows, sent, cap)
    assert isinstance(A, int), f"{tag}: {A}"
    print(tag, "A =", A, "counts =", raw["counts"].tolist(), "expected", exp["counts"].tolist())
    assert A == exp["counts"][0]
    lc.assert_equals(sorted_entries(A, raw), exp, tag)
    for k in ("frame", "abs_l0", "flip", "rank"):  # rows >= A are untouched
        assert untouched(raw[k], A), f"{tag}: {k} written past the entries"
    return A, raw


@pytest.mark.parametrize("name", lc.NAMES)
def test_label_device_matches_oracle(name):
    rows, msg = lc.rows_of(name)
    check(_decoder(name), rows, msg, lc.expected(name), name)


def test_label_device_tie_case():
    rows, msg, exp = lc.tie_case()
    assert exp["tie8"] >= 1
    check(_decoder("n128L4"), rows, msg, exp, "ties")


@pytest.mark.parametrize("name", ["m4_2p5db", "m8_3db"])
def test_label_device_both_sent_forms(name):
    rows, sent, M, exp = lc.g12_case(name)
    dec = _native.get_decoder(128, lc.ac.info_set(128, 64), M, lc.POLY24)
    check(dec, rows, sent, exp, name + " one message")
    check(dec, rows, np.tile(sent, (rows.shape[0], 1)), exp, name + " per frame")


def test_label_device_without_rank_output():
    rows, msg = lc.rows_of("n32k14")
    exp = lc.expected("n32k14")
    A, raw = run_device(_decoder("n32k14"), rows, msg, with_rank=False)
    assert A == exp["counts"][0] and untouched(raw["rank"])
    out = sorted_entries(A, raw)
    np.testing.assert_array_equal(out["flip"], exp["flip"])
    np.testing.assert_array_equal(out["counts"], exp["counts"])


def test_label_device_capacity():
    name = "n128L4"
    rows, msg = lc.rows_of(name)
    exp = lc.expected(name)
    A = int(exp["counts"][0])
    got, raw = run_device(_decoder(name), rows, msg, cap=A - 1)
    assert isinstance(got, _native.LabelCapacity) and got.entries == A
    assert all(untouched(raw[k]) for k in raw), "a short capacity must leave every output untouched"
    check(_decoder(name), rows, msg, exp, "cap = A", cap=A)
    lc.assert_equals(_decoder(name).label(rows, msg), exp, "Decoder.label")
    lc.assert_equals(_decoder(name).label(rows, msg, cap=A - 1), exp, "Decoder.label, repeated with the reported count")


def test_label_device_empty_batch():
    dec = _decoder("n128L4")
    A, raw = run_device(dec, np.zeros((0, 128)), np.zeros(64, np.int8), cap=4)
    assert A == 0 and raw["counts"].tolist() == [0, 0, 0, 0]
    assert all(untouched(raw[k]) for k in ("frame", "abs_l0", "flip", "rank"))


def test_label_device_all_pass_launches_no_round():
    rows, msg, exp = lc.allpass_case()
    assert exp["counts"][0] == 0
    dec = _native.get_decoder(128, lc.ac.info_set(128, 64), 8, lc.POLY24)
    dec.timing_enable(True)
    try:
        A, raw = run_device(dec, rows, msg)
        launches, _ = dec.timing_read()
    finally:
        dec.timing_enable(False)
    assert A == 0 and raw["counts"].tolist() == [0, 0, 0, 0]
    assert launches == 1  # the baseline decode alone
    assert all(untouched(raw[k]) for k in ("frame", "abs_l0", "flip", "rank"))


def test_label_device_after_pipelined_decode():
    name = "n128L4"
    c = lc.CASES[name]
    rows, msg = lc.rows_of(name)
    exp = lc.expected(name)
    dec = _native.Decoder(c.N, lc.info_of(name), c.L, c.crc)
    try:
        dec.set_pipelined(True)
        with _native.DeviceArena(dec) as mem:
            d_llr, d_best, d_flags = mem.alloc(rows.nbytes), mem.alloc(c.B * dec.W * 8), mem.alloc(c.B)
            mem.upload(d_llr, np.ascontiguousarray(rows))
            dec.decode_device(d_llr, c.B, d_best=d_best, d_flags=d_flags)  # (its re-decode is still pending)
            check(dec, rows, msg, exp, "pipelined")
            dec.sync()
            flags = mem.download(d_flags, c.B, np.uint8)
        np.testing.assert_array_equal(np.flatnonzero((flags & _native.PSCL_FLAG_CRC_PASS) == 0), exp["frame"])
    finally:
        dec.close()


def test_label_device_consecutive_calls_of_different_size():
    name = "n256"
    c = lc.CASES[name]
    rows, msg = lc.rows_of(name)
    exp = lc.expected(name)
    dec = _native.Decoder(c.N, lc.info_of(name), c.L, c.crc)
    try:
        for n in (40, c.B, 40):
            check(dec, rows[:n], msg[:n], lc.subset(exp, n), f"{name} first {n}")
    finally:
        dec.close()


def test_label_tensor():
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    name = "n128L4"
    c = lc.CASES[name]
    rows, msg = lc.rows_of(name)
    exp = lc.expected(name)
    dec = SCLDecoder(c.N, lc.info_of(name), c.L, c.crc)
    llr = torch.from_numpy(np.array(rows)).cuda()  # (a writable copy: the case's rows are read-only)
    words = torch.from_numpy(_native.pack_bits(msg, dec.native.W).view(np.int64)).cuda()
    out = dec.label_tensor(llr, words)
    torch.cuda.synchronize()
    assert out["abs_l0"].dtype == torch.float32 and out["flip"].dtype == torch.int32 and out["frame"].dtype == torch.int64
    lc.assert_equals({k: v.cpu().numpy() for k, v in out.items()}, exp, "label_tensor")
    lc.assert_equals(dec.label(rows, msg), exp, "SCLDecoder.label")
    with pytest.raises(ValueError):
        dec.label_tensor(llr.float(), words)
    dec.native.close()


@pytest.mark.parametrize("name", ["m4_2p5db", "m8_3db"])
def test_dataset_label_native_matches_reference(tmp_path, name):
    g = np.load(GOLDEN / "g12_dataset.npz")
    argv = str(g[name + "_argv"]).split()
    shard = md.generate_samples(md.build_argparser().parse_args(
        argv + ["--out", str(tmp_path / "ds"), "--batch", "128", "--label", "native"]))
    z = np.load(shard)
    np.testing.assert_array_equal(z["abs_l0"], g[name + "_abs_l0"])
    np.testing.assert_array_equal(z["flip_idx"], g[name + "_flip_idx"])
    assert json.loads(str(z["meta"])) == json.loads(str(g[name + "_meta"]))


def test_dataset_philox_label_native(tmp_path):
    from polar_code_amd import config
    from polar_code_amd.polar.polar import construct_info_set

    shard = md.generate_samples(md.build_argparser().parse_args(
        ["--M", "4", "--snr_db", "2.5", "--frames", "20000", "--out", str(tmp_path / "p"), "--rng", "philox",
         "--batch", "8192", "--label", "native"]))
    z = np.load(shard)
    meta = json.loads(str(z["meta"]))
    assert z["abs_l0"].shape == (meta["samples"], 64) and z["abs_l0"].dtype == np.float32
    assert z["flip_idx"].dtype == np.int32 and (z["flip_idx"] >= 0).all() and (z["flip_idx"] < 64).all()
    frac = meta["samples"] / 20000
    print("philox native: labelled fraction", frac, "failures", meta["failures"])
    assert 0.18 < frac < 0.36, frac  # (the band of test_make_dataset's philox test: the reference's 79 of 300)
    # the first 2,048 frames: the device chain against the host loop on the same rows, downloaded,
    # with the frames' own messages
    cfg = config.get_config()
    info = construct_info_set(cfg.N, cfg.K)
    kp, n = cfg.K - cfg.crc_bits, 2048
    dec = _native.get_decoder(cfg.N, info, 4, cfg.crc_poly)
    with _native.DeviceArena(dec) as mem:
        d_llr, d_msg = mem.alloc(n * cfg.N * 8), mem.alloc(n * dec.W * 8)
        dec.channel_device(0, 0x7FFF0000 + 25, 2.5, cfg.K / cfg.N, kp, 0, n, d_llr, d_msg)
        llr = mem.download(d_llr, n * cfg.N * 8, np.float64).reshape(n, cfg.N)
        words = mem.download(d_msg, n * dec.W * 8, np.uint64).reshape(n, dec.W)
    msg = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(n, -1)[:, :cfg.K].astype(np.int8)
    a_h, lab_h, nf_h = md.label_batch(llr, info, 4, cfg.crc_poly, msg)
    a_d, lab_d, nf_d = md._philox_label_native(0, 2.5, 0, n, info, 4, cfg.crc_poly, kp)
    np.testing.assert_array_equal(a_d.view(np.uint32), a_h.view(np.uint32))
    np.testing.assert_array_equal(lab_d, lab_h)
    assert nf_d == nf_h
    np.testing.assert_array_equal(z["flip_idx"][:lab_d.size], lab_d)  # (the shard's first frames are these)


def test_label_device_argument_errors():
    dec = _decoder("n32k14")
    rows, msg = lc.rows_of("n32k14")
    with pytest.raises(ValueError):
        dec.label(rows, msg, max_flips=0)
    with pytest.raises(ValueError):
        dec.label(rows, msg, max_flips=33)
    with pytest.raises(ValueError):
        dec.label(rows, msg[:, :13])
    nocrc = _native.Decoder(32, lc.info_of("n32k14"), 4, None)
    try:
        with pytest.raises(ValueError):
            nocrc.label(rows, msg)
    finally:
        nocrc.close()
    with _native.DeviceArena(dec) as mem:
        d = mem.alloc(4096)
        kw = dict(d_frame=d, d_abs_l0=d, d_flip=d, d_counts=d)
        for bad in (dict(B=-1), dict(cap=-1), dict(stride=2), dict(d_sent=0), dict(d_llr=0)):
            a = {"d_llr": d, "B": 4, "d_sent": d, "stride": 0, "cap": 4, **bad}
            with pytest.raises(ValueError):
                dec.label_device(a["d_llr"], a["B"], a["d_sent"], a["stride"], 8, a["cap"], **kw)
        with pytest.raises(NotImplementedError):
            dec.label_device(d, 2 ** 31, d, 0, 8, 4, **kw)
