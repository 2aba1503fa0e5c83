"""CPU: the caller-payload encode entry points -- declared, bound and exported; pscl_encode_cpu
(the host form of pscl_encode_device) against the oracle's attach_crc and polar_transform and the
host mirrors of the NR interleaver and rate matching on every code of encode_cases.py, and against
the goldens g2 (payload -> attached), g3 (msg -> code) and g8 (rate-matched payloads) directly;
payload bits from k_payload on are ignored; the SCLDecoder methods validate before any device
call.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import oracle
from encode_cases import CODES, POLY24, RATE_MATCHED, crc_degree, expected, info_set, pack, payloads, unpack
from polar_code_amd import _native

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "polar_scl.h"

NEW = {
    "pscl_encode_device": ["pscl_handle*", "const uint64_t*", "int64_t", "uint64_t*", "uint64_t*", "void*", "int"],
    "pscl_channel_payload_device": ["pscl_handle*", "const uint64_t*", "uint64_t", "uint32_t", "double", "double", "int64_t",
                                    "int64_t", "void*", "int", "uint64_t*"],
    "pscl_encode_cpu": ["int", "const int32_t*", "int", "uint64_t", "int", "const uint64_t*", "int64_t", "uint64_t*",
                        "uint64_t*"],
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
    for method in ("encode_device", "channel_payload_device"):
        assert callable(getattr(_native.Decoder, method))
    assert callable(_native.encode_cpu)
    assert re.search(r"#define PSCL_ABI_VERSION 1\b", HEADER.read_text()) and _native.lib().pscl_abi_version() == 1


def test_null_handle_and_payload_are_refused_without_a_device():
    lib = _native.lib()
    assert lib.pscl_encode_device(None, None, 0, None, None, None, 0) == _native.PSCL_EINVAL
    assert "handle" in _native.last_error()
    assert lib.pscl_channel_payload_device(None, None, 0, 0, 0.0, 0.5, 0, 0, None, 0, None) == _native.PSCL_EINVAL
    assert "handle" in _native.last_error()


def test_encode_kernels_use_no_scratch_and_spill_nothing():
    """The eight instances (two kernels x noise x float32 rows) exist under names of their own -- none
    carries the float32 decode instances' `_f32` tag -- with no scratch, no spilled VGPR and no SGPR
    parked in VGPR lanes."""
    import importlib.util

    lib_path = ROOT / "polar_code_amd" / "libpolar_mi355x.so"
    if not lib_path.exists() or not Path("/opt/rocm/lib/llvm/bin/llvm-readelf").exists():
        pytest.skip("needs the built library and llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mine = {n: v for n, v in mod.kernels(lib_path).items() if "encode_kernel" in n or "encode_long_kernel" in n}
    assert len(mine) == 8 and not any("_f32" in n for n in mine), sorted(mine)
    for n, v in mine.items():
        assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
        assert v["vgpr_count"] <= 64, (n, v)  # (eight wavefronts per SIMD)


def _cpu(N, K, crc, E, bits):
    msg, code = _native.encode_cpu(N, info_set(N, K), crc, pack(bits), E)
    return unpack(msg, K), unpack(code, E or N), code


@pytest.mark.parametrize("N,K,crc,E", [c + (0,) for c in CODES] + RATE_MATCHED)
def test_encode_cpu_equals_the_oracle(N, K, crc, E):
    bits = payloads(N, K, crc, 67)
    bits[0], bits[1] = 0, 1  # all-zero and all-one payloads among them
    want_msg, want_tx = expected(N, K, crc, E, bits)
    msg, tx, words = _cpu(N, K, crc, E, bits)
    np.testing.assert_array_equal(msg, want_msg)
    np.testing.assert_array_equal(tx, want_tx)
    Et = E or N
    if Et & 63:  # bits past E in the last code word are zero
        assert not np.any(words[:, -1] >> np.uint64(Et & 63))


def test_encode_cpu_equals_goldens(golden):
    g2, g3, g8 = golden("g2_crc.npz"), golden("g3_encode.npz"), golden("g8_nr.npz")
    # g2: 40 payload bits -> the 64 attached bits (CRC-24), and 8 -> 12 (poly 0x17)
    msg, _, _ = _cpu(128, 64, POLY24, 0, g2["payload"])
    np.testing.assert_array_equal(msg, g2["attached"])
    msg, _, _ = _cpu(16, 12, "0x17", 0, g2["payload8"])
    np.testing.assert_array_equal(msg, g2["attached8_0x17"])
    # g3: 64 message bits -> the codeword of the default (128,64) code, no CRC
    msg, code, _ = _cpu(128, 64, None, 0, g3["msg"])
    np.testing.assert_array_equal(msg, g3["msg"])
    np.testing.assert_array_equal(code, g3["code"])
    # g8: the payloads of the rate-matched (128,88) code at E = 256, through the host mirror that the
    # golden's interleaver and rate-matching vectors pin to the reference
    info = g8["info"]
    np.testing.assert_array_equal(info, info_set(128, 88))
    m, c = _native.encode_cpu(128, info, POLY24, pack(g8["payload"]), 256)
    from polar_code_amd.nr.polar.scl_nr import encode_rate_matched

    want = np.stack([encode_rate_matched(p, POLY24, 128, 256, info) for p in g8["payload"]])
    np.testing.assert_array_equal(unpack(c, 256), want)
    np.testing.assert_array_equal(unpack(m, 88)[:, :64], g8["payload"])


@pytest.mark.parametrize("N,K,crc", [(8, 6, "0xB"), (128, 74, POLY24), (128, 100, POLY24), (256, 140, POLY24)])
def test_bits_from_k_payload_on_are_ignored(N, K, crc):
    kp = K - crc_degree(crc)
    assert kp & 63  # (the last payload word has bits to spare)
    bits = payloads(N, K, crc, 9)
    clean = pack(bits)
    dirty = clean.copy()
    dirty[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(kp & 63)
    info = info_set(N, K)
    a, b = _native.encode_cpu(N, info, crc, clean), _native.encode_cpu(N, info, crc, dirty)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_encode_cpu_refusals():
    info = info_set(128, 64)
    pw = np.zeros((3, 1), np.uint64)
    with pytest.raises(ValueError):
        _native.encode_cpu(100, [1, 2], None, pw)                      # N not a power of two
    with pytest.raises(ValueError):
        _native.encode_cpu(128, info[:10], POLY24, np.zeros((3, 0), np.uint64))  # K <= CRC degree
    with pytest.raises(ValueError):
        _native.encode_cpu(128, info, POLY24, np.zeros((3, 2), np.uint64))  # [B, Wp] with Wp = 1
    with pytest.raises(ValueError):
        _native.encode_cpu(128, info[::-1], POLY24, pw)                # info set not ascending
    with pytest.raises(NotImplementedError):
        _native.encode_cpu(8, info_set(8, 6), "0xB", pw, E=12)         # repetition needs N >= 32
    lib = _native.lib()
    ip = np.ascontiguousarray(info, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros((3, 2), np.uint64)
    assert lib.pscl_encode_cpu(128, ip, 64, 0x1864CFB, 0, None, 3, out.ctypes.data, None) == _native.PSCL_EINVAL
    assert lib.pscl_encode_cpu(128, ip, 64, 0x1864CFB, 0, pw.ctypes.data, 3, None, None) == _native.PSCL_EINVAL
    assert lib.pscl_encode_cpu(128, ip, 64, 0x1864CFB, 0, pw.ctypes.data, -1, out.ctypes.data, None) == _native.PSCL_EINVAL
    assert lib.pscl_encode_cpu(128, ip, 64, 0x1864CFB, -5, pw.ctypes.data, 3, out.ctypes.data, None) == _native.PSCL_EINVAL
    assert lib.pscl_encode_cpu(128, ip, 64, 0x1864CFB, 0, pw.ctypes.data, 0, out.ctypes.data, None) == _native.PSCL_OK


def test_sclDecoder_encode_on_the_host():
    """device="cpu": the host-array convenience packs, calls pscl_encode_cpu and unpacks."""
    from polar_code_amd.polar.scl import SCLDecoder

    N, K, crc = 128, 88, POLY24
    dec = SCLDecoder(N, info_set(N, K), 4, crc, device="cpu")
    assert dec.k_payload == 64 and dec.payload_words == 1
    bits = payloads(N, K, crc, 21)
    want_msg, want_tx = expected(N, K, crc, 0, bits)
    out = dec.encode(bits)
    np.testing.assert_array_equal(out["msg"], want_msg)
    np.testing.assert_array_equal(out["code"], want_tx)
    assert out["msg"].dtype == np.int8 and out["code"].dtype == np.int8
    assert all(oracle.check_crc(m, crc) for m in out["msg"])
    with pytest.raises(ValueError):
        dec.encode(bits[:, :-1])
    with pytest.raises(ValueError):
        dec.encode(bits + 2)
    with pytest.raises(ValueError):
        dec.encode_tensor(None)


# ---- the torch methods validate before any device call

class _NoDevice:
    """Stands in for the native decoder: the row lengths and nothing else."""
    E, W, code_words = 0, 2, 2

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before validation")


def _stub():
    from polar_code_amd.polar.scl import SCLDecoder

    dec = SCLDecoder.__new__(SCLDecoder)
    dec.N, dec.L, dec.K, dec.device, dec._dec = 128, 8, 100, 0, _NoDevice()
    dec.k_payload, dec.payload_words = 76, 2
    return dec


def test_tensor_methods_refuse_bad_payloads_before_any_device_call():
    import torch

    dec = _stub()
    bad = (torch.zeros((4, 2), dtype=torch.int32),
           torch.zeros((4, 2), dtype=torch.float64),
           torch.zeros((4, 2), dtype=torch.uint8),
           torch.zeros((4, 4), dtype=torch.int64)[:, ::2],  # not contiguous
           torch.zeros((2, 4), dtype=torch.int64).t(),      # not contiguous
           torch.zeros((4, 1), dtype=torch.int64),
           torch.zeros((4, 3), dtype=torch.int64),
           torch.zeros((2,), dtype=torch.int64),
           torch.zeros((4, 2), dtype=torch.int64),          # a host tensor: not on this decoder's GPU
           np.zeros((4, 2), np.int64))
    for p in bad:
        with pytest.raises(ValueError):
            dec.encode_tensor(p)
        with pytest.raises(ValueError):
            dec.encode_tensor(p, symbols=torch.float32)
        with pytest.raises(ValueError):
            dec.transmit_tensor(p, 3.0, seed=1)
    good_shape = torch.zeros((4, 2), dtype=torch.int64)
    for sym in (torch.float16, torch.int64, "float32"):
        with pytest.raises(ValueError):
            dec.encode_tensor(good_shape, symbols=sym)
    with pytest.raises(ValueError):
        dec.transmit_tensor(good_shape, 3.0, seed=1, dtype=torch.float16)
    with pytest.raises(ValueError):
        dec.transmit_tensor(good_shape, 3.0, seed=1, frame0=-1)


def test_tensor_methods_reach_the_device_layer_with_good_payloads(monkeypatch):
    """(a payload that passes every check reaches the device layer: the stand-in objects to the
    first call.  The device check is stood in for, since no GPU tensor exists here.)"""
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    dec = _stub()
    monkeypatch.setattr(SCLDecoder, "_payload_tensor", lambda self, p: p.shape[0])
    good = torch.zeros((4, 2), dtype=torch.int64)
    with pytest.raises(AssertionError, match="device call"):
        dec.encode_tensor(good)
    with pytest.raises(AssertionError, match="device call"):
        dec.transmit_tensor(good, 3.0, seed=1, dtype=torch.float32)
    with pytest.raises(ValueError):  # (rate is checked before the first call too)
        dec.transmit_tensor(good, 3.0, seed=1, rate=0.0)
