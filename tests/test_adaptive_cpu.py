"""Adaptive decoding on the host (pscl_decode_adaptive_cpu, CpuDecoder.decode_adaptive): SC first,
the list decoder only where the SC result fails the CRC.  The result is the composition of the
oracle's sc_decode + check_crc and decode_batch, bit for bit (adaptive_cases.compose).  Also the
code-object check of the device stage's SC kernel (no scratch, no spills).  No GPU needed."""
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
from polar_code_amd import _native

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "polar_code_amd" / "libpolar_mi355x.so"
READELF = Path("/opt/rocm/lib/llvm/bin/llvm-readelf")


def _cpu(L, threads=0, N=128, K=64, crc=ac.POLY24):
    return _native.CpuDecoder(N, ac.info_set(N, K), L, crc, threads=threads)


@pytest.mark.parametrize("L", [8, 4])
def test_cpu_mixed_batch_equals_composition(L):
    exp = ac.mixed_expected(L)
    assert 0.15 * 4099 < exp["n_escalated"] < 0.5 * 4099
    out = _cpu(L).decode_adaptive(ac.mixed_rows())
    ac.assert_equals(out, exp, f"cpu mixed L={L}")
    assert out["n_escalated"] == exp["n_escalated"]


def test_cpu_all_pass_and_all_fail():
    rows, exp = ac.allpass_case()
    assert exp["n_escalated"] == 0
    out = _cpu(8).decode_adaptive(rows)
    ac.assert_equals(out, exp, "cpu all-pass")
    assert out["n_escalated"] == 0 and np.all(out["stage"] == 1)
    rows, exp = ac.allfail_case()
    assert exp["n_escalated"] == len(rows)
    out = _cpu(8).decode_adaptive(rows)
    ac.assert_equals(out, exp, "cpu all-fail")
    np.testing.assert_array_equal(out["best_bits"], exp["list_bits"])  # plain L = 8 exactly
    np.testing.assert_array_equal(out["best_idx"], exp["list_idx"])
    assert out["n_escalated"] == len(rows)


def test_cpu_threads_give_identical_output():
    rows = ac.mixed_rows()[:1500]
    a, b = _cpu(8, threads=1).decode_adaptive(rows), _cpu(8, threads=4).decode_adaptive(rows)
    for k in ("best_bits", "crc_pass", "best_idx", "stage"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["n_escalated"] == b["n_escalated"]


def test_cpu_n256():
    info = ac.info_set(256, 128)
    rows = ac.make_llr(79, 300, info, ac.POLY24, 3.0, N=256)
    exp = ac.compose(rows, info, 4, ac.POLY24, N=256)
    assert 0 < exp["n_escalated"] < 300
    out = _cpu(4, N=256, K=128).decode_adaptive(rows)
    ac.assert_equals(out, exp, "cpu N=256")
    assert out["n_escalated"] == exp["n_escalated"]


def test_cpu_requires_a_crc():
    dec = _native.CpuDecoder(128, ac.info_set(128, 64), 8, None)
    with pytest.raises(ValueError):
        dec.decode_adaptive(ac.mixed_rows()[:4])


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="needs the built library and llvm-readelf")
def test_sc_kernel_uses_no_scratch_and_does_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hits = {n: v for n, v in mod.kernels(LIB).items() if re.search(r"sc128_lane_kernelILb[01]E", n)}
    assert len(hits) == 2, sorted(hits)  # the plain and the rate-matched instance
    for n, v in hits.items():
        assert v.get("private_segment_fixed_size", 0) == 0, f"{n} uses {v['private_segment_fixed_size']} B of scratch"
        assert v.get("vgpr_spill_count", 0) == 0, f"{n} spills {v['vgpr_spill_count']} VGPRs"
        assert v.get("sgpr_spill_count", 0) == 0, f"{n} spills {v['sgpr_spill_count']} SGPRs"
