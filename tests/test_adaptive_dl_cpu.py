"""CPU: DL-SCL retries on an adaptive baseline -- the entry points are declared, bound and
exported; the oracle's counts on the inputs of the GPU tests (so the inputs cannot silently stop
exercising the chains); the sweep CLI's arguments, CSV header and rows with and without --retries;
the three-stage path waits on the host exactly once; the stage-mark kernel spills nothing.  No GPU."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_dl_cases as dc
from polar_code_amd import _native

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "polar_scl.h"
CAPI = ROOT / "polar_code_amd" / "csrc" / "capi.cpp"
LIB = ROOT / "polar_code_amd" / "libpolar_mi355x.so"
READELF = Path("/opt/rocm/lib/llvm/bin/llvm-readelf")

_SIM = ["pscl_handle*", "uint64_t", "uint32_t", "double", "double", "int", "int64_t", "int64_t", "int", "int", "int64_t*"]
NEW = {
    "pscl_retry_device": ["pscl_handle*", "const double*", "int64_t", "int", "uint64_t*", "uint8_t*", "uint8_t*", "int32_t*",
                          "int32_t*", "int", "const uint64_t*", "int", "int64_t*"],
    "pscl_adaptive_dlscl_device": ["pscl_handle*", "const double*", "int64_t", "int", "uint64_t*", "uint8_t*", "uint8_t*",
                                   "int32_t*", "int32_t*", "int", "const uint64_t*", "int", "int64_t*", "int32_t*"],
    "pscl_simulate_adaptive_dl": _SIM,
    "pscl_simulate_adaptive_dl_device": _SIM,
}


def _declared_args(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in polar_scl.h"
    return [re.sub(r"\s*\b\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NEW))
def test_declared_bound_and_exported(name):
    assert _declared_args(name) == NEW[name]
    assert name in _native.EXPORTS
    fn = getattr(_native.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(NEW[name])
    scalar = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}
    for ctype, decl in zip(fn.argtypes, NEW[name]):
        if decl in scalar:
            assert ctype is scalar[decl], (name, decl, ctype)
        else:
            assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, decl, ctype)


def test_python_entry_points_and_abi():
    for method in ("retry_device", "adaptive_dlscl_device", "simulate_adaptive_dl", "simulate_adaptive_dl_device"):
        assert callable(getattr(_native.Decoder, method))
    assert _native.lib().pscl_abi_version() == 1
    import inspect

    from polar_code_amd.dlscl import flip

    assert inspect.signature(flip.decode_with_retries_device).parameters["baseline"].default == "scl"
    sig = inspect.signature(_native.Decoder.decode_adaptive).parameters
    assert sig["retries"].default == 0 and sig["beta"].default is None
    with pytest.raises(ValueError):
        flip.decode_with_retries_device(np.zeros((1, 128)), ac.info_set(128, 64), 8, 8, crc=ac.POLY24, baseline="sc")


def test_null_handle_is_an_argument_error():
    lib = _native.lib()
    assert lib.pscl_retry_device(None, None, 0, 0, None, None, None, None, None, 0, None, 0, None) == -1
    assert lib.pscl_adaptive_dlscl_device(None, None, 0, 0, None, None, None, None, None, 0, None, 0, None, None) == -1
    assert lib.pscl_simulate_adaptive_dl(None, 0, 0, 0.0, 0.5, 0, 0, 0, 0, 0, None) == -1
    assert lib.pscl_simulate_adaptive_dl_device(None, 0, 0, 0.0, 0.5, 0, 0, 0, 0, 0, None) == -1


def _counts(exp):
    return exp["n_escalated"], exp["n_entries"], exp["n_recovered"]


@pytest.mark.parametrize("L,with_beta,want", [(8, False, (1040, 42, 10)), (8, True, (1040, 42, 7)),
                                              (4, False, (1040, 171, 79)), (4, True, (1040, 171, 38))])
def test_pinned_counts_mixed(L, with_beta, want):
    exp = dc.mixed_case(L, with_beta)
    assert len(exp["stage"]) == 4099 and _counts(exp) == want
    ent = exp["stage"] == 3
    assert np.all(exp["attempts"][~ent] == 1) and np.all(exp["tried"][~ent] == -1)
    assert np.all((exp["tried"][ent] >= 0).sum(axis=1) == exp["attempts"][ent] - 1)
    assert np.all(exp["crc_pass"][ent] | (exp["attempts"][ent] == 9))  # a chain ends at a pass or after 8 flips


def test_pinned_counts_other_cases():
    assert _counts(dc.mixed_case(8, False, 3)) == (1040, 42, 9) and dc.mixed_case(8, False, 3)["attempts"].max() == 4
    assert _counts(dc.prefix(dc.mixed_case(8), 130))[1:] == (1, 1)
    assert len(dc.mixed_case(2)["stage"]) == 130 and _counts(dc.mixed_case(2))[1:] == (18, 7)
    assert _counts(dc.allpass_case()[1]) == (0, 0, 0)
    rows, exp = dc.allfail_case()
    assert _counts(exp) == (1000, 1000, 0) and np.all(exp["attempts"] == 9)
    assert _counts(dc.nr_case()[1]) == (1131, 178, 65)
    assert _counts(dc.crc16_case()[2]) == (691, 294, 75)
    assert _counts(dc.n256_case()[2]) == (199, 105, 17)
    assert _counts(dc.c32_case()[3])[1:] == (2, 0)
    rows, _, exp = dc.n1024_case()
    assert len(rows) <= 131 and exp["n_entries"] >= 8 and exp["n_recovered"] >= 1


def test_retries_0_is_the_adaptive_composition():
    exp = dc.compose_dl(ac.mixed_rows(), ac.info_set(128, 64), 8, ac.POLY24, 0, base=ac.mixed_expected(8))
    ac.assert_equals(exp, ac.mixed_expected(8), "retries 0")
    assert exp["n_entries"] == 0 and exp["tried"].shape == (4099, 0) and np.all(exp["attempts"] == 1)


def test_cli_arguments_and_csv_header():
    from polar_code_amd.eval import run_adaptive_sweep as ras

    args = ras.build_argparser().parse_args(["--M", "8"])
    assert (args.retries, args.beta) == (0, None)
    args = ras.build_argparser().parse_args(["--M", "4", "--retries", "8", "--beta", "b.npy"])
    assert (args.retries, args.beta) == (8, "b.npy")
    base = ["fer_sc", "ber_sc", "fer_adaptive", "ber_adaptive", "escalated"]
    assert ras.csv_header(False) == ras.csv_header(False, 0) == ["snr_db"] + base
    assert ras.csv_header(False, 8) == ["snr_db"] + base + ["fer_dl", "ber_dl", "avg_retries"]
    assert ras.csv_header(True, 8) == ["snr_db", "fer_uncoded", "ber_uncoded"] + base + ["fer_dl", "ber_dl", "avg_retries"]


def test_csv_rows_with_and_without_retries(tmp_path):
    from polar_code_amd.eval import run_adaptive_sweep as ras

    cnt = np.zeros((4, _native.PSCL_NCOUNT), np.int64)
    cnt[0, [_native.CNT_FRAMES, _native.CNT_FRAME_ERR, _native.CNT_BIT_ERR]] = (1000, 250, 6400)
    cnt[1, [_native.CNT_FRAMES, _native.CNT_FRAME_ERR, _native.CNT_BIT_ERR, _native.CNT_ESCALATED]] = (1000, 10, 320, 250)
    cnt[2, [_native.CNT_FRAMES, _native.CNT_FRAME_ERR, _native.CNT_BIT_ERR, _native.CNT_RETRIES]] = (1000, 5, 128, 70)
    cnt[3, [_native.CNT_FRAMES, _native.CNT_FRAME_ERR, _native.CNT_BIT_ERR]] = (1000, 500, 400)
    row = ras.row_from_counters(5.0, cnt, 1000, 64, 40, True, 8)
    assert row == {"snr_db": 5.0, "fer_sc": 0.25, "ber_sc": 0.1, "fer_adaptive": 0.01, "ber_adaptive": 0.005,
                   "escalated": 0.25, "fer_dl": 0.005, "ber_dl": 0.002, "avg_retries": 0.07, "fer_uncoded": 0.5,
                   "ber_uncoded": 0.01}
    args = ras.build_argparser().parse_args(["--M", "4", "--include_uncoded", "--retries", "8", "--out_dir", str(tmp_path)])
    lines = ras.write_csv([row], args).read_text().splitlines()
    assert lines[0] == ",".join(ras.csv_header(True, 8))
    assert lines[1] == ("5.000,5.000000e-01,1.000000e-02,2.500000e-01,1.000000e-01,1.000000e-02,5.000000e-03,2.500000e-01,"
                        "5.000000e-03,2.000000e-03,7.000000e-02")
    # without --retries: the three-row counters and the file of before
    old = ras.row_from_counters(5.0, cnt[[0, 1, 3]], 1000, 64, 40, True)
    assert old == {k: v for k, v in row.items() if k not in ("fer_dl", "ber_dl", "avg_retries")}
    args = ras.build_argparser().parse_args(["--M", "4", "--include_uncoded", "--out_dir", str(tmp_path)])
    lines = ras.write_csv([old], args).read_text().splitlines()
    assert lines[0] == ",".join(ras.csv_header(True))
    assert lines[1] == "5.000,5.000000e-01,1.000000e-02,2.500000e-01,1.000000e-01,1.000000e-02,5.000000e-03,2.500000e-01"


# every function of capi.cpp between pscl_adaptive_dlscl_device's entry and its retry chains
THREE_STAGE_PATH = ("pscl_adaptive_dlscl_device", "adaptive_async_args", "dlscl_impl", "adaptive_begin", "launch_sc_stage",
                    "adaptive_escalate_enqueue", "dl_setup", "dl_chain", "dl_enqueue_deferred", "dl_retry_chunk",
                    "dl_retry_long")


def _body(src, name):
    """The brace block of the definition of `name` (at any namespace depth)."""
    m = re.search(r"\b" + name + r"\s*\([^;{}]*\)\s*\{", src)
    assert m, f"{name} not found in capi.cpp"
    depth, j = 0, m.end() - 1
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return src[m.end() - 1:j]
        j += 1


def test_three_stage_path_waits_on_the_host_once():
    spec = importlib.util.spec_from_file_location("stream_order", ROOT / "tests" / "test_stream_order.py")
    so = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(so)
    src = so.strip_comments(CAPI.read_text())
    waits = {n: len(re.findall(r"\bhip\w*Synchronize\s*\(", _body(src, n))) for n in THREE_STAGE_PATH}
    assert sum(waits.values()) == 1 and waits["dl_chain"] == 1, waits  # the failing count, read by dl_chain
    for n in THREE_STAGE_PATH:
        assert not re.search(r"\bhipMemcpy\s*\(", _body(src, n)), f"{n} copies synchronously"
    # the three-stage call and the chain entry are dlscl_impl, not a second driver
    for n in ("pscl_adaptive_dlscl_device", "pscl_retry_device"):
        assert len(re.findall(r"\bdlscl_impl\s*\(", _body(src, n))) == 1, n
    body = _body(src, "dlscl_impl")
    for callee in ("adaptive_begin", "launch_sc_stage", "adaptive_escalate_enqueue"):
        assert len(re.findall(r"\b" + callee + r"\s*\(", body)) == 1, callee


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="needs the built library and llvm-readelf")
def test_stage_mark_kernel_uses_no_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [v for n, v in mod.kernels(LIB).items() if "dl_mark_stage_kernel" in n]
    assert len(ks) == 1, len(ks)
    k = ks[0]
    assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
    assert k["vgpr_count"] <= 32, k
