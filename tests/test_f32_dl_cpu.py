"""CPU: the float32 DL-SCL entry points -- declared with their float64 forms' arguments, bound and
exported; the Python methods exist and validate before any device call; the row type travels with
the call, not the handle; and the cases of test_gpu_f32_dl.py meet the counts stated beside them (the
oracle on the float32-rounded rows), so the GPU tests cannot pass vacuously.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_dl_cases as dc
import f32_dl_cases as fd
from polar_code_amd import _native

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "polar_scl.h"
CSRC = ROOT / "polar_code_amd" / "csrc"

# float64 form -> float32 form: the same arguments but the row pointer
TWINS = {"pscl_dlscl_device": "pscl_dlscl_device_f32", "pscl_retry_device": "pscl_retry_device_f32",
         "pscl_adaptive_dlscl_device": "pscl_adaptive_dlscl_device_f32", "pscl_path_llrs_device": "pscl_path_llrs_device_f32"}
_H, _F, _B, _W, _U8, _I32, _REF, _CNT = ("pscl_handle*", "const float*", "int64_t", "uint64_t*", "uint8_t*", "int32_t*",
                                         "const uint64_t*", "int64_t*")
PROTOTYPES = {
    "pscl_dlscl_device_f32": [_H, _F, _B, "int", _W, _U8, _I32, _I32, "int", _REF, "int", _CNT, _CNT],
    "pscl_retry_device_f32": [_H, _F, _B, "int", _W, _U8, _U8, _I32, _I32, "int", _REF, "int", _CNT],
    "pscl_adaptive_dlscl_device_f32": [_H, _F, _B, "int", _W, _U8, _U8, _I32, _I32, "int", _REF, "int", _CNT, _I32],
    "pscl_path_llrs_device_f32": [_H, _F, _B, _REF, "double*"],
}


def _declared_args(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in polar_scl.h"
    return [re.sub(r"\s*\b\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]


@pytest.mark.parametrize("f64,f32", sorted(TWINS.items()))
def test_declared_bound_and_exported(f64, f32):
    a, b = _declared_args(f64), _declared_args(f32)
    assert b == PROTOTYPES[f32]
    assert a[1] == "const double*" and b[1] == "const float*" and a[:1] + a[2:] == b[:1] + b[2:]
    assert f32 in _native.EXPORTS
    fn, twin = getattr(_native.lib(), f32), getattr(_native.lib(), f64)
    assert fn.restype is C.c_int and list(fn.argtypes) == list(twin.argtypes) and len(fn.argtypes) == len(b)


def test_abi_version_and_null_handle():
    lib = _native.lib()
    assert re.search(r"#define PSCL_ABI_VERSION 1\b", HEADER.read_text()) and lib.pscl_abi_version() == 1  # (additions only)
    assert lib.pscl_f32_available(None) == 0
    assert lib.pscl_dlscl_device_f32(None, None, 0, 8, None, None, None, None, 0, None, 0, None, None) == -1
    assert lib.pscl_retry_device_f32(None, None, 0, 8, None, None, None, None, None, 0, None, 0, None) == -1
    assert lib.pscl_adaptive_dlscl_device_f32(None, None, 0, 8, None, None, None, None, None, 0, None, 0, None, None) == -1
    assert lib.pscl_path_llrs_device_f32(None, None, 0, None, None) == -1


def test_python_methods_exist():
    from polar_code_amd.polar.scl import SCLDecoder

    for m in ("dlscl_device_f32", "retry_device_f32", "adaptive_dlscl_device_f32", "path_llrs_device_f32"):
        assert callable(getattr(_native.Decoder, m)), m
    for m in ("decode_tensor_dlscl", "decode_tensor_retry", "decode_tensor_adaptive_dlscl"):
        assert callable(getattr(SCLDecoder, m)), m


class _NoDevice:
    """Stands in for the native decoder: the row length and nothing else."""
    E, W, crc_deg = 0, 1, 24

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before validation")


@pytest.mark.parametrize("method", ["decode_tensor_dlscl", "decode_tensor_retry", "decode_tensor_adaptive_dlscl"])
def test_tensor_methods_refuse_bad_rows_before_any_device_call(method):
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    dec = SCLDecoder.__new__(SCLDecoder)
    dec.N, dec.L, dec.K, dec._dec = 128, 8, 64, _NoDevice()
    best, flags = torch.zeros((4, 1), dtype=torch.int64), torch.zeros((4,), dtype=torch.uint8)
    args = (best, flags, 8) if method == "decode_tensor_retry" else (8,)
    for bad in (torch.zeros((4, 128), dtype=torch.float16), torch.zeros((4, 128), dtype=torch.int32),
                torch.zeros((4, 256), dtype=torch.float32)[:, ::2], torch.zeros((4, 127), dtype=torch.float32),
                torch.zeros((128,), dtype=torch.float64)):
        with pytest.raises(ValueError):
            getattr(dec, method)(bad, *args)
    for good in (torch.zeros((4, 128), dtype=torch.float32), torch.zeros((4, 128), dtype=torch.float64)):
        with pytest.raises(AssertionError, match="device call"):
            getattr(dec, method)(good, *args)


def test_row_type_travels_with_the_call():
    """The handle has no float32 member; a DL-SCL call keeps its row type with its arguments
    (pscl_dl_call, copied into the handle's deferred-call slot as a whole), and every launch block of
    a chain gets it from there."""
    src = (CSRC / "capi.cpp").read_text()
    handle = re.search(r"struct pscl_handle \{(.*?)\n\};", src, re.S).group(1)
    assert "f32" not in handle and re.search(r"\bpscl_dl_call dl_defer;", handle)
    call = re.search(r"struct pscl_dl_call \{(.*?)\n\};", src, re.S).group(1)
    assert re.search(r"\bbool row_f32 = false;", call)
    assert re.search(r"dl_retry_chunk\([^;]*a\.row_f32\);", src)  # (dl_chain hands the call's own type down)
    chunk = src[src.index("int dl_retry_chunk("):src.index("// long codes (N > PSCL_FAST_N): dense entry state")]
    assert "Q.row_f32 = f32 ? 1 : 0;" in chunk and "pscl_set_row_type(H, f32);" in chunk
    hdr = (CSRC / "scl_kernels.h").read_text()
    for block in ("pscl_post_params", "pscl_replay_params"):
        body = re.sub(r"\s*//[^\n]*", "", re.search(r"struct " + block + r" \{(.*?)\n\};", hdr, re.S).group(1))
        assert re.search(r"int N, n, K, W, rm_E;\s+int row_f32;\s+const int32_t\* rm_src;", body), block
        assert re.search(r"static_assert\(offsetof\(" + block + r", rm_src\) == offsetof\(" + block + r", rm_E\) \+ 8", hdr)


# ---- the cases of the GPU tests meet their stated counts

@pytest.mark.parametrize("L,with_beta,entries,recovered", [(8, False, 42, 10), (8, True, 42, 7), (4, False, 171, 79),
                                                           (4, True, 171, 38)])
def test_mixed_counts(L, with_beta, entries, recovered):
    assert fd.counts(fd.mixed_case(L, with_beta)) == (4099, 1040, entries, recovered)


@pytest.mark.parametrize("L", [8, 4])
@pytest.mark.parametrize("with_beta", [False, True])
def test_tie_counts(L, with_beta):
    rows, exp = fd.tie_case(L, with_beta)
    assert rows.dtype == np.float32 and fd.counts(exp) == (480, 160, 160, 0)
    assert np.all(exp["attempts"][exp["stage"] == 3] == 9)
    # |L0| ties: without beta the first flip of most chains is decided by the lower-index rule
    assert np.count_nonzero(exp["tried"][exp["stage"] == 3, 0] >= 0) == 160


def test_corner_counts():
    rows, exp = fd.corner_case()
    assert rows.dtype == np.float32 and fd.counts(exp) == (229, 224, 192, 0)
    assert np.abs(rows).max() > 3e38 and np.any((rows != 0) & (np.abs(rows) < np.float32(1.1e-38)))


@pytest.mark.parametrize("E,counts", [(256, (263, 147, 18, 2)), (201, (263, 155, 47, 12))])
def test_nr_counts(E, counts):
    rows, exp = fd.nr_case(E)
    assert rows.shape == (263, E) and fd.counts(exp) == counts


def test_allfail_and_allpass_counts():
    exp = fd.allfail_case()[1]
    assert fd.counts(exp) == (1000, 1000, 1000, 0) and np.all(exp["attempts"] == 9)
    assert fd.counts(fd.allpass_case()[1])[:3] == (1000, 0, 0)


@pytest.mark.parametrize("L,base_fail,final_fail", [(8, 7, 6), (4, 44, 34)])
def test_plain_chain_counts(L, base_fail, final_fail):
    rows, exp = fd.plain_case(L)
    assert len(rows) == 1027
    assert (int(np.count_nonzero(~exp["base_ok"])), int(np.count_nonzero(~exp["crc_pass"]))) == (base_fail, final_fail)
    assert exp["attempts"].max() == 9


def test_retries_3_and_crc16_cases():
    exp = fd.mixed_case(8, False, 3)
    assert exp["tried"].shape == (4099, 3) and exp["n_entries"] == 42 and exp["attempts"].max() == 4
    rows, info, e16 = fd.crc16_case()
    assert rows.dtype == np.float32 and len(info) == 40 and len(rows) == 1027
    assert e16["n_entries"] > 100 and e16["n_recovered"] > 10
    assert dc.KEYS == ("best_bits", "crc_pass", "best_idx", "stage", "attempts", "tried")
