"""Staged decoding without a GPU: the information-set families of the SC kernel's tests, the
code-object check of every sc_lane_kernel instance (no scratch, no spills), and the two entry
points' declarations and bindings."""
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
import staged_cases as sc
from polar_code_amd import _native

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "polar_code_amd" / "libpolar_mi355x.so"
READELF = Path("/opt/rocm/lib/llvm/bin/llvm-readelf")


@pytest.mark.parametrize("N", sc.LENGTHS)
def test_block_family_reaches_every_branch_state(N):
    fam = sc.block_family(N)
    n = N.bit_length() - 1
    assert len(fam) == 2 * n and all(len(info) == N // 2 for _, info in fam)
    reached = set()
    for _, info in fam:
        reached |= ac.sc_branch_states(info, N=N)
    assert reached == ac.all_branch_states(N) and len(reached) == 3 * (N - 1)


@pytest.mark.parametrize("N,K", [(256, 128), (512, 256), (1024, 512), (64, 17)])
def test_polarization_weight_set(N, K):
    info = sc.pw_info_set(N, K)
    assert info.dtype == np.int32 and len(info) == K == len(set(info.tolist())) and np.all(np.diff(info) > 0)
    np.testing.assert_array_equal(info, sc.pw_info_set.__wrapped__(N, K))  # deterministic
    w = sc.pw_weights(N)
    assert w[0] == 0.0 and w[N - 1] == sum(2.0 ** (j / 4) for j in range(N.bit_length() - 1))
    rest = np.setdiff1d(np.arange(N), info)
    assert w[info].min() >= w[rest].max()
    assert N - 1 in info and 0 not in info


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="needs the built library and llvm-readelf")
def test_sc_lane_kernels_use_no_scratch_and_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hits = {}
    for n, v in mod.kernels(LIB).items():
        m = re.search(r"14sc_lane_kernelILi(\d+)E", n)
        if m:
            hits[int(m.group(1))] = v
    assert sorted(hits) == list(sc.LENGTHS), sorted(hits)
    for N, v in hits.items():
        assert v.get("private_segment_fixed_size", 0) == 0, f"N = {N} uses {v['private_segment_fixed_size']} B of scratch"
        assert v.get("vgpr_spill_count", 0) == 0, f"N = {N} spills {v['vgpr_spill_count']} VGPRs"
        assert v.get("sgpr_spill_count", 0) == 0, f"N = {N} spills {v['sgpr_spill_count']} SGPRs"
        assert v.get("vgpr_count", 0) <= 256, f"N = {N}: fewer than two wavefronts per SIMD"


def test_header_declares_and_native_binds_the_entry_points():
    header = (ROOT / "include" / "polar_scl.h").read_text()
    for name in ("pscl_sc_device", "pscl_escalate_device"):
        assert re.search(rf"^int {name}\(pscl_handle\* h, const double\* d_llr, int64_t B,", header, re.M), name
        assert name in _native.EXPORTS
    for method in ("sc_device", "escalate_device", "decode_sc", "decode_staged"):
        assert callable(getattr(_native.Decoder, method))
    from polar_code_amd.polar.scl import SCLDecoder

    for method in ("decode_sc", "decode_staged", "decode_tensor_staged"):
        assert callable(getattr(SCLDecoder, method))


@pytest.mark.skipif(not LIB.exists(), reason="needs the built library")
def test_library_exports_the_entry_points_with_their_signatures():
    L = _native.lib()
    assert len(L.pscl_sc_device.argtypes) == 9 and len(L.pscl_escalate_device.argtypes) == 10
