"""CPU: the adaptive decode without the host wait -- its entry points are declared, bound and
exported; the row-list instances of the lane kernel spill nothing; the functions of the path make
no hip*Synchronize call; the sweep CLI's arguments and CSV header.  No GPU."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import pytest

from polar_code_amd import _native

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "polar_scl.h"
CAPI = ROOT / "polar_code_amd" / "csrc" / "capi.cpp"
LIB = ROOT / "polar_code_amd" / "libpolar_mi355x.so"
READELF = Path("/opt/rocm/lib/llvm/bin/llvm-readelf")

NEW = {
    "pscl_adaptive_async_device": ["pscl_handle*", "const double*", "int64_t", "uint64_t*", "uint8_t*", "uint8_t*",
                                   "const uint64_t*", "int", "int64_t*", "int32_t*"],
    "pscl_simulate_adaptive_device": ["pscl_handle*", "uint64_t", "uint32_t", "double", "double", "int", "int64_t",
                                      "int64_t", "int", "int64_t*"],
    "pscl_simulate_adaptive": ["pscl_handle*", "uint64_t", "uint32_t", "double", "double", "int", "int64_t", "int64_t",
                               "int", "int64_t*"],
    "pscl_adaptive_stats": ["pscl_handle*", "int64_t*", "int64_t*", "int64_t*", "int"],
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
    for ctype, decl in zip(fn.argtypes, NEW[name]):
        scalar = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}
        if decl in scalar:
            assert ctype is scalar[decl], (name, decl, ctype)
        else:  # pointers: void* or a typed pointer
            assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, decl, ctype)
    for method in ("adaptive_async_device", "simulate_adaptive", "simulate_adaptive_device", "adaptive_stats"):
        assert callable(getattr(_native.Decoder, method))


def test_null_handle_is_an_argument_error():
    lib = _native.lib()
    assert lib.pscl_adaptive_async_device(None, None, 0, None, None, None, None, 0, None, None) == -1
    assert lib.pscl_simulate_adaptive_device(None, 0, 0, 0.0, 0.5, 0, 0, 0, 0, None) == -1
    assert lib.pscl_simulate_adaptive(None, 0, 0, 0.0, 0.5, 0, 0, 0, 0, None) == -1
    assert lib.pscl_adaptive_stats(None, None, None, None, 0) == -1


def _waves_per_simd(vgprs):
    """Wavefronts per SIMD by VGPR count (512 per lane, allocated in blocks of 8, at most 8 waves)."""
    return min(8, 512 // (-(-vgprs // 8) * 8))


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="needs the built library and llvm-readelf")
def test_row_list_instances_spill_nothing_and_keep_the_occupancy():
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = mod.kernels(LIB)
    for lmax in (4, 8):
        for code in (1, 2):
            stem = f"scl_lane_kernelILi{lmax}ELi{code}ELb0ELb0ELb0ELb0ELb"
            plain = [v for n, v in ks.items() if stem + "0EE" in n]
            rl = [v for n, v in ks.items() if stem + "1EE" in n]
            assert len(plain) == 1 and len(rl) == 1, (lmax, code, len(plain), len(rl))
            assert rl[0].get("private_segment_fixed_size", 0) == 0, (lmax, code, rl[0])
            assert rl[0].get("vgpr_spill_count", 0) == 0, (lmax, code, rl[0])
            assert _waves_per_simd(rl[0]["vgpr_count"]) >= _waves_per_simd(plain[0]["vgpr_count"]), (lmax, code, rl[0], plain[0])


# the functions of the path without a host wait (the host form pscl_simulate_adaptive waits once,
# at its end, by contract)
ASYNC_FUNCS = ("adaptive_begin", "adaptive_escalate_enqueue", "adaptive_async_args", "pscl_adaptive_async_device",
               "simulate_adaptive_enqueue", "pscl_simulate_adaptive_device", "pscl_adaptive_stats")


def test_async_path_makes_no_host_wait():
    spec = importlib.util.spec_from_file_location("stream_order", ROOT / "tests" / "test_stream_order.py")
    so = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(so)
    src = so.strip_comments(CAPI.read_text())

    def span(name):
        """The brace block of the definition of `name` (at any namespace depth)."""
        m = re.search(r"\b" + name + r"\s*\([^;{}]*\)\s*\{", src)
        assert m, f"{name} not found in capi.cpp"
        depth, j = 0, m.end() - 1
        while True:
            depth += {"{": 1, "}": -1}.get(src[j], 0)
            if depth == 0:
                return m.end() - 1, j
            j += 1

    spans = {n: span(n) for n in ASYNC_FUNCS + ("pscl_simulate_adaptive",)}
    for name in ASYNC_FUNCS:
        a, b = spans[name]
        body = src[a:b]
        assert not re.search(r"\bhip\w*Synchronize\s*\(", body), f"{name} waits on the host"
        assert not re.search(r"\bhipMemcpy\s*\(|\bhipMemcpyAsync\s*\([^;]*DeviceToHost", body), f"{name} copies to the host"
    a, b = spans["pscl_simulate_adaptive"]
    assert len(re.findall(r"\bhip\w*Synchronize\s*\(", src[a:b])) == 1  # the host form's one wait


def test_cli_arguments_and_csv_header():
    from polar_code_amd.eval import run_adaptive_sweep as ras

    args = ras.build_argparser().parse_args(["--M", "8", "--frames", "123", "--snr_lo", "4", "--snr_hi", "5", "--snr_step",
                                             "0.5", "--seed", "7", "--include_uncoded", "--batch", "64", "--out_dir", "x"])
    assert (args.M, args.frames, args.snr_lo, args.snr_hi, args.snr_step, args.seed, args.include_uncoded, args.batch,
            args.out_dir) == (8, 123, 4.0, 5.0, 0.5, 7, True, 64, "x")
    assert list(ras.snr_points(args)) == [4.0, 4.5, 5.0]
    with pytest.raises(SystemExit):
        ras.build_argparser().parse_args([])  # --M is required
    assert ras.csv_header(False) == ["snr_db", "fer_sc", "ber_sc", "fer_adaptive", "ber_adaptive", "escalated"]
    assert ras.csv_header(True) == ["snr_db", "fer_uncoded", "ber_uncoded", "fer_sc", "ber_sc", "fer_adaptive",
                                    "ber_adaptive", "escalated"]


def test_csv_row_from_counters(tmp_path):
    import numpy as np

    from polar_code_amd.eval import run_adaptive_sweep as ras

    cnt = np.zeros((3, _native.PSCL_NCOUNT), np.int64)
    cnt[0, [_native.CNT_FRAMES, _native.CNT_FRAME_ERR, _native.CNT_BIT_ERR]] = (1000, 250, 6400)
    cnt[1, [_native.CNT_FRAMES, _native.CNT_FRAME_ERR, _native.CNT_BIT_ERR, _native.CNT_ESCALATED]] = (1000, 10, 320, 250)
    cnt[2, [_native.CNT_FRAMES, _native.CNT_FRAME_ERR, _native.CNT_BIT_ERR]] = (1000, 500, 400)
    row = ras.row_from_counters(5.0, cnt, 1000, 64, 40, True)
    assert row == {"snr_db": 5.0, "fer_sc": 0.25, "ber_sc": 0.1, "fer_adaptive": 0.01, "ber_adaptive": 0.005,
                   "escalated": 0.25, "fer_uncoded": 0.5, "ber_uncoded": 0.01}
    args = ras.build_argparser().parse_args(["--M", "4", "--include_uncoded", "--out_dir", str(tmp_path)])
    path = ras.write_csv([row], args)
    assert path.name == "fer_adaptive_M4.csv"
    lines = path.read_text().splitlines()
    assert lines[0] == ",".join(ras.csv_header(True))
    assert lines[1] == "5.000,5.000000e-01,1.000000e-02,2.500000e-01,1.000000e-01,1.000000e-02,5.000000e-03,2.500000e-01"
