"""ctypes binding of libpolar_mi355x.so (include/polar_scl.h).

There is deliberately no fallback: if the HIP library is missing or no GPU is visible,
every decode raises.  Argument errors are mapped back to the reference's exception types
(ValueError / RuntimeError, dl_scl_polar/polar/scl.py:117-131,171-172).
"""
from __future__ import annotations

import ctypes as C
import functools
import importlib.util
import os
import sys
import threading
from pathlib import Path

import numpy as np

LIB_PATH = Path(os.environ.get("PSCL_LIB_PATH") or Path(__file__).resolve().parent / "libpolar_mi355x.so")

PSCL_OK = 0
PSCL_EINVAL = -1
PSCL_EDEVICE = -2
PSCL_ENOMEM = -3
PSCL_EPRUNED = -4
PSCL_EUNSUP = -5
PSCL_MAX_N = 1024
PSCL_REPLAY_MAX_N = 1024  # pscl_path_llrs_device (decision-LLR replay) on float64 rows; the float32 form takes N = 128 only
PSCL_MAX_L = 32
PSCL_FLAG_CRC_PASS = 0x80
PSCL_FLAG_IDX_MASK = 0x3F
PSCL_NCOUNT = 8
CNT_FRAMES, CNT_FRAME_ERR, CNT_BIT_ERR, CNT_PAYLOAD_ERR, CNT_PAYLOAD_BIT, CNT_RETRIES, CNT_ESCALATED = range(7)

# every symbol the header declares (tests/test_capi_symbols.py checks the .so exports them)
EXPORTS = (
    "pscl_last_error", "pscl_abi_version", "pscl_device_count", "pscl_create", "pscl_destroy",
    "pscl_set_stream", "pscl_get_stream", "pscl_sync", "pscl_decode", "pscl_sc_decode",
    "pscl_decode_device", "pscl_channel_device", "pscl_device_alloc", "pscl_device_free",
    "pscl_memcpy_htod", "pscl_memcpy_dtoh", "pscl_memset_device", "pscl_timing_enable",
    "pscl_timing_read", "pscl_launch_info", "pscl_set_rate_match", "pscl_set_beta", "pscl_dlscl_device",
    "pscl_path_llrs_device", "pscl_uncoded_device", "pscl_simulate", "pscl_set_screening", "pscl_build_hash",
    "pscl_screening_count", "pscl_softplus_tails_device", "pscl_set_pipelined", "pscl_join",
    "pscl_tail_abs_scan_device", "pscl_tail2_scan_device", "pscl_set_tuning", "pscl_timing_read_split", "pscl_decode_cpu",
    "pscl_host_stats", "pscl_path_stats",
    "pscl_simulate_device", "pscl_adaptive_device", "pscl_decode_adaptive_cpu",
    "pscl_sc_device", "pscl_escalate_device",
    "pscl_adaptive_async_device", "pscl_simulate_adaptive", "pscl_simulate_adaptive_device", "pscl_adaptive_stats",
    "pscl_retry_device", "pscl_adaptive_dlscl_device", "pscl_simulate_adaptive_dl", "pscl_simulate_adaptive_dl_device",
    "pscl_f32_available", "pscl_decode_device_f32", "pscl_sc_device_f32", "pscl_escalate_device_f32",
    "pscl_adaptive_async_device_f32",
    "pscl_dlscl_device_f32", "pscl_retry_device_f32", "pscl_adaptive_dlscl_device_f32", "pscl_path_llrs_device_f32",
    "pscl_encode_device", "pscl_channel_payload_device", "pscl_encode_cpu",
    "pscl_derate_match_device", "pscl_set_rate_match_staged", "pscl_rm_staged_stats",
    "pscl_path_llrs_cpu", "pscl_replay_stats",
    "pscl_label_device", "pscl_label_cpu",
)

# pscl_label_device / pscl_label_cpu counts (int64[PSCL_NLABEL])
PSCL_NLABEL = 4
LBL_ENTRIES, LBL_LABELLED, LBL_UNREPAIRED, LBL_DECODES = range(4)

# pscl_set_tuning knobs (include/polar_scl.h)
TUNE = {"dl_screen": 1, "dl_chunks": 2, "dl_split": 3, "side_priority": 4, "post_grid": 5, "retry_wpg": 6, "dl_lane": 7, "dl_screen_min": 8, "dl_retry_lane": 9, "post_pairs": 10, "dl_streams": 11, "tx_fused": 12,
        "dl_fused_post": 13, "post_epw": 14, "lane_exact": 15, "dl_warm_apx": 16, "dl_tail": 17, "adapt_grid": 18, "dl_long_replay": 19}

_vp, _i32, _i64, _u64, _dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double


class PolarNativeError(RuntimeError):
    """Device/runtime failure inside libpolar_mi355x.so."""


def _bind_hip_runtime() -> None:
    """Keep ONE HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so.7; if
    this library loaded /opt/rocm's copy first, torch would later load a second runtime and
    see no GPU.  Preloading torch's copy (same soname) makes both bind to it.  Set
    PSCL_HIP_RUNTIME=system to keep /opt/rocm's runtime (processes that never use torch)."""
    if os.environ.get("PSCL_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    cand = Path(spec.origin).parent / "lib" / "libamdhip64.so"
    if cand.exists():
        C.CDLL(str(cand), mode=C.RTLD_GLOBAL)


def _check_fresh() -> None:
    """Refuse a library built from other sources than the ones in this tree (its embedded
    build hash, polar_code_amd/build.py).  Skipped where the sources are absent."""
    from . import build

    if not all((build.CSRC / s).exists() for s in build.HIP_DEPS):
        return
    want, got = build.source_hash(), build.library_hash(LIB_PATH)
    if got != want:
        raise PolarNativeError(
            f"{LIB_PATH} is stale (built from sources {got}, tree has {want}): "
            "run `python -m polar_code_amd.build`")


@functools.lru_cache(maxsize=1)
def lib() -> C.CDLL:
    _bind_hip_runtime()
    if not LIB_PATH.exists():
        raise PolarNativeError(
            f"{LIB_PATH} not built: run `python -m polar_code_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the decoder.")
    if not os.environ.get("PSCL_LIB_PATH"):
        _check_fresh()
    L = C.CDLL(str(LIB_PATH))
    P = C.POINTER
    sig = {
        "pscl_last_error": (C.c_char_p, []),
        "pscl_abi_version": (C.c_int, []),
        "pscl_build_hash": (C.c_char_p, []),
        "pscl_screening_count": (C.c_int, [_vp, P(_i64)]),
        "pscl_set_pipelined": (C.c_int, [_vp, C.c_int]),
        "pscl_join": (C.c_int, [_vp]),
        "pscl_softplus_tails_device": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
        "pscl_tail_abs_scan_device": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
        "pscl_tail2_scan_device": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
        "pscl_set_tuning": (C.c_int, [_vp, C.c_int, _i64]),
        "pscl_simulate_device": (C.c_int, [_vp, _u64, C.c_uint32, _dbl, _dbl, C.c_int, _i64, _i64, C.c_int, C.c_int,
                                           _vp]),
        "pscl_decode_cpu": (C.c_int, [C.c_int, P(_i32), C.c_int, C.c_int, _u64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, C.c_int]),
        "pscl_adaptive_device": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, C.c_int, _vp, P(_i64)]),
        "pscl_sc_device": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, C.c_int, _vp]),
        "pscl_escalate_device": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, C.c_int, _vp, P(_i64)]),
        "pscl_decode_adaptive_cpu": (C.c_int, [C.c_int, P(_i32), C.c_int, C.c_int, _u64, _vp, _i64, _vp, _vp, _vp, _vp,
                                               C.c_int]),
        "pscl_adaptive_async_device": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp]),
        "pscl_f32_available": (C.c_int, [_vp]),
        "pscl_decode_device_f32": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, C.c_int, _vp]),
        "pscl_sc_device_f32": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, C.c_int, _vp]),
        "pscl_escalate_device_f32": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, C.c_int, _vp, P(_i64)]),
        "pscl_adaptive_async_device_f32": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp]),
        "pscl_dlscl_device_f32": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp,
                                            _vp]),
        "pscl_retry_device_f32": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int,
                                            _vp]),
        "pscl_adaptive_dlscl_device_f32": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp,
                                                     C.c_int, _vp, _vp]),
        "pscl_path_llrs_device_f32": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
        "pscl_encode_device": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, C.c_int]),
        "pscl_channel_payload_device": (C.c_int, [_vp, _vp, _u64, C.c_uint32, _dbl, _dbl, _i64, _i64, _vp, C.c_int, _vp]),
        "pscl_encode_cpu": (C.c_int, [C.c_int, P(_i32), C.c_int, _u64, C.c_int, _vp, _i64, _vp, _vp]),
        "pscl_simulate_adaptive_device": (C.c_int, [_vp, _u64, C.c_uint32, _dbl, _dbl, C.c_int, _i64, _i64, C.c_int, _vp]),
        "pscl_simulate_adaptive": (C.c_int, [_vp, _u64, C.c_uint32, _dbl, _dbl, C.c_int, _i64, _i64, C.c_int, _vp]),
        "pscl_adaptive_stats": (C.c_int, [_vp, P(_i64), P(_i64), P(_i64), C.c_int]),
        "pscl_retry_device": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp]),
        "pscl_adaptive_dlscl_device": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int,
                                                 _vp, _vp]),
        "pscl_simulate_adaptive_dl_device": (C.c_int, [_vp, _u64, C.c_uint32, _dbl, _dbl, C.c_int, _i64, _i64, C.c_int,
                                                       C.c_int, _vp]),
        "pscl_simulate_adaptive_dl": (C.c_int, [_vp, _u64, C.c_uint32, _dbl, _dbl, C.c_int, _i64, _i64, C.c_int, C.c_int,
                                                _vp]),
        "pscl_timing_read_split": (C.c_int, [_vp, P(_i64), P(_dbl), P(_i64), P(_dbl)]),
        "pscl_host_stats": (C.c_int, [_vp, P(_dbl), P(_dbl), P(_i64), C.c_int]),
        "pscl_path_stats": (C.c_int, [_vp, P(_i64), P(_i64), P(_i64), P(_i64), P(_i64)]),
        "pscl_device_count": (C.c_int, []),
        "pscl_create": (C.c_int, [P(_vp), C.c_int, C.c_int, P(_i32), C.c_int, C.c_int, _u64]),
        "pscl_destroy": (C.c_int, [_vp]),
        "pscl_set_stream": (C.c_int, [_vp, _vp]),
        "pscl_get_stream": (_vp, [_vp]),
        "pscl_sync": (C.c_int, [_vp]),
        "pscl_decode": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "pscl_sc_decode": (C.c_int, [_vp, _vp, _i64, _vp]),
        "pscl_decode_device": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp]),
        "pscl_channel_device": (C.c_int, [_vp, _u64, C.c_uint32, _dbl, _dbl, C.c_int, _i64, _i64, _vp, _vp]),
        "pscl_device_alloc": (C.c_int, [_vp, P(_vp), _i64]),
        "pscl_device_free": (C.c_int, [_vp, _vp]),
        "pscl_memcpy_htod": (C.c_int, [_vp, _vp, _vp, _i64]),
        "pscl_memcpy_dtoh": (C.c_int, [_vp, _vp, _vp, _i64]),
        "pscl_memset_device": (C.c_int, [_vp, _vp, C.c_int, _i64]),
        "pscl_timing_enable": (C.c_int, [_vp, C.c_int]),
        "pscl_set_screening": (C.c_int, [_vp, C.c_int]),
        "pscl_timing_read": (C.c_int, [_vp, P(_i64), P(_dbl)]),
        "pscl_launch_info": (C.c_int, [_vp, _i64, P(C.c_int), P(_i64), P(C.c_int)]),
        "pscl_set_rate_match": (C.c_int, [_vp, C.c_int]),
        "pscl_derate_match_device": (C.c_int, [_vp, _vp, _i64, _vp]),
        "pscl_set_rate_match_staged": (C.c_int, [_vp, C.c_int]),
        "pscl_rm_staged_stats": (C.c_int, [_vp, P(_i64), P(_i64), C.c_int]),
        "pscl_replay_stats": (C.c_int, [_vp, P(_i64), P(_i64), C.c_int]),
        "pscl_path_llrs_cpu": (C.c_int, [C.c_int, P(_i32), C.c_int, _vp, _i64, _vp, _vp, C.c_int]),
        "pscl_label_device": (C.c_int, [_vp, _vp, _i64, _vp, _i64, C.c_int, _i64, _vp, _vp, _vp, _vp, _vp, P(_i64)]),
        "pscl_label_cpu": (C.c_int, [C.c_int, P(_i32), C.c_int, C.c_int, _u64, _vp, _i64, _vp, _i64, C.c_int, _vp, _vp, _vp,
                                     _vp, _vp, C.c_int]),
        "pscl_set_beta": (C.c_int, [_vp, _vp]),
        "pscl_path_llrs_device": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
        "pscl_uncoded_device": (C.c_int, [_vp, _u64, C.c_uint32, _dbl, C.c_int, _i64, _i64, _vp]),
        "pscl_simulate": (C.c_int, [_vp, _u64, C.c_uint32, _dbl, _dbl, C.c_int, _i64, _i64, C.c_int, C.c_int, _vp]),
        "pscl_dlscl_device": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp,
                                        _vp]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("PSCL_LIB_PATH") and not hasattr(L, name):
            continue  # an older variant library under A/B timing (tools/ab_bench.sh)
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def build_hash() -> str:
    """The loaded library's embedded source hash ("" for variant libraries without one)."""
    fn = getattr(lib(), "pscl_build_hash", None)
    return fn().decode() if fn is not None else ""


def last_error() -> str:
    return lib().pscl_last_error().decode(errors="replace")


def check(rc: int) -> None:
    if rc == PSCL_OK:
        return
    msg = last_error()
    if rc == PSCL_EINVAL:
        raise ValueError(msg)
    if rc == PSCL_EPRUNED:
        raise RuntimeError("All paths pruned during decoding")
    if rc == PSCL_EUNSUP:
        raise NotImplementedError(msg)
    raise PolarNativeError(f"libpolar_mi355x error {rc}: {msg}")


def device_count() -> int:
    n = lib().pscl_device_count()
    if n < 0:
        raise PolarNativeError(last_error())
    return n


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data


class LabelCapacity(ValueError):
    """pscl_label_device found more entries than the output arrays hold; `entries` is the count."""

    def __init__(self, msg: str, entries: int):
        super().__init__(msg)
        self.entries = int(entries)


def pack_bits(bits: np.ndarray, W: int) -> np.ndarray:
    """[B, K] 0/1 -> [B, W] uint64 words, bit j at word j >> 6, bit j & 63 (include/polar_scl.h)."""
    bits = np.asarray(bits)
    B, K = bits.shape
    pad = np.zeros((B, W * 64), np.uint8)
    pad[:, :K] = bits
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view(np.uint64).reshape(B, W)


def label_capacity(B: int, K: int) -> int:
    """First capacity of a label call's output arrays: every frame while the |L0| rows stay under
    256 MiB (no repeat is then possible), else a quarter of the batch, grown to the count the call
    reports if that was short."""
    B = int(B)
    return max(B if B * K * 4 <= (1 << 28) else 1024 + B // 4, 1)


def _sent_bits(sent, B: int, K: int) -> np.ndarray:
    """The labeller's sent messages as int8 [1, K] (one for all frames) or [B, K]."""
    s = np.asarray(sent)
    if s.ndim == 1:
        s = s[None, :]
    elif s.ndim != 2 or s.shape[0] != B:
        raise ValueError(f"sent must be [{K}] or [B, {K}]")
    if s.shape[1] != K:
        raise ValueError(f"sent must be [{K}] or [B, {K}]")
    if np.any((s != 0) & (s != 1)):
        raise ValueError("sent entries must be 0 or 1")
    return np.ascontiguousarray(s, dtype=np.int8)


def _sent_words(sent, B: int, K: int, W: int):
    """(words, sent_stride) of pscl_label_device for sent [K] (stride 0) or [B, K] (stride W)."""
    one = np.asarray(sent).ndim == 1
    s = _sent_bits(sent, B, K)
    return pack_bits(s, W), 0 if one else W


def poly_value(crc) -> int:
    """The reference's CRC polynomial hex string (crc.py:10-16) as an integer (0 = no CRC)."""
    if crc is None:
        return 0
    if isinstance(crc, (int, np.integer)):
        return int(crc)
    if not crc:
        raise ValueError("CRC polynomial string must be non-empty")
    return int(str(crc), 16)


class Decoder:
    """One pscl_handle: a polar code (N, info set, list size, CRC) bound to one device."""

    def __init__(self, N: int, info_set, L: int, crc=None, device: int = 0):
        info = np.ascontiguousarray(np.asarray(info_set).astype(np.int32).ravel())
        self.N, self.K, self.L = int(N), int(info.size), int(L)
        self.info_set = info
        self.crc_poly = poly_value(crc)
        self.crc_deg = max(self.crc_poly.bit_length() - 1, 0)
        self.W = (self.K + 63) // 64 if self.K else 1
        self.device = int(device)
        h = _vp()
        check(lib().pscl_create(C.byref(h), self.device, self.N, info.ctypes.data_as(C.POINTER(_i32)), self.K,
                                self.L, self.crc_poly))
        self._hraw = h
        self._lock = threading.Lock()
        self.E = 0
        self._beta = None

    def set_rate_match(self, E: int) -> None:
        """NR: decode inputs become [B, E] received LLRs (de-rate-match + de-interleave on GPU)."""
        check(lib().pscl_set_rate_match(self._h, int(E)))
        self.E = int(E)

    def set_rate_match_staged(self, on: bool = True) -> None:
        """Staged de-rate-matching (pscl_set_rate_match_staged, default off): decode_device, sc_device,
        escalate_device and adaptive_async_device of a rate-matched handle run the de-rate-matching
        pass once and then the plain-row screening and SC kernels; results are bit-identical."""
        check(lib().pscl_set_rate_match_staged(self._h, 1 if on else 0))

    def derate_match_device(self, d_llr: int, B: int, d_out: int) -> None:
        """[B][E] received LLRs -> the [B][N] decoder-internal rows, enqueued without a host wait
        (pscl_derate_match_device; a rate-matched handle)."""
        with self._lock:
            check(lib().pscl_derate_match_device(self._h, d_llr or None, int(B), d_out or None))

    def rm_staged_stats(self, reset: bool = False) -> dict:
        """Passes the staged mode launched and the rows they staged (pscl_rm_staged_stats)."""
        a, b = _i64(), _i64()
        check(lib().pscl_rm_staged_stats(self._h, C.byref(a), C.byref(b), 1 if reset else 0))
        return {"passes": int(a.value), "rows": int(b.value)}

    def replay_stats(self, reset: bool = False) -> dict:
        """Launches of the long replay kernel (N = 256..1024) and the rows they were sized for
        (pscl_replay_stats): pscl_path_llrs_device's and the DL-SCL chains' under dl_long_replay."""
        a, b = _i64(), _i64()
        check(lib().pscl_replay_stats(self._h, C.byref(a), C.byref(b), 1 if reset else 0))
        return {"launches": int(a.value), "rows": int(b.value)}

    @property
    def _h(self):
        h = getattr(self, "_hraw", None)
        if h is None:
            raise RuntimeError("Decoder is closed (close(), or release_decoders() on a get_decoder() handle)")
        return h

    @property
    def handle(self):
        return self._h

    @property
    def closed(self) -> bool:
        return getattr(self, "_hraw", None) is None

    def close(self) -> None:
        if getattr(self, "_hraw", None):
            lib().pscl_destroy(self._hraw)
            self._hraw = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    # ---------------------------------------------------------------- host buffers
    def decode(self, llr: np.ndarray, forced: np.ndarray | None = None, *, want_metrics=True,
               want_cands=True, want_info_llrs=True):
        """Batched decode_scl on host arrays.  llr: [B, N] float64."""
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        B = llr.shape[0]
        if llr.shape[1] != (self.E or self.N):
            raise ValueError("Channel LLR length must be a power of two" if not self.E
                             else f"expected {self.E} rate-matched LLRs per frame")
        if forced is not None:
            forced = np.ascontiguousarray(forced, dtype=np.int8).reshape(B, self.K)
        out = {
            "n_paths": np.zeros(B, np.int32),
            "best_bits": np.zeros((B, self.K), np.int8),
            "crc_pass": np.zeros(B, np.uint8),
            "best_idx": np.zeros(B, np.int32),
            "metrics": np.full((B, self.L), np.nan) if want_metrics else None,
            "cands": np.zeros((B, self.L, self.K), np.int8) if want_cands else None,
            "info_llrs": np.full((B, self.L, self.K), np.nan) if want_info_llrs else None,
        }
        with self._lock:
            check(lib().pscl_decode(self._h, _ptr(llr), B, _ptr(forced), _ptr(out["n_paths"]),
                                    _ptr(out["best_bits"]), _ptr(out["crc_pass"]), _ptr(out["best_idx"]),
                                    _ptr(out["metrics"]), _ptr(out["cands"]), _ptr(out["info_llrs"])))
        out["crc_pass"] = out["crc_pass"].astype(bool)
        return out

    def sc_decode(self, llr: np.ndarray) -> np.ndarray:
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        bits = np.zeros((llr.shape[0], self.K), np.int8)
        with self._lock:
            check(lib().pscl_sc_decode(self._h, _ptr(llr), llr.shape[0], _ptr(bits)))
        return bits

    # -------------------------------------------------------------- device buffers
    def set_stream(self, stream_ptr: int | None) -> None:
        check(lib().pscl_set_stream(self._h, stream_ptr))

    def decode_device(self, d_llr: int, B: int, *, d_force=0, d_best=0, d_flags=0, d_metrics=0, d_cands=0,
                      d_info_llrs=0, d_ref=0, k_payload=0, d_counters=0) -> None:
        check(lib().pscl_decode_device(self._h, d_llr, B, d_force or None, d_best or None, d_flags or None,
                                       d_metrics or None, d_cands or None, d_info_llrs or None, d_ref or None,
                                       int(k_payload), d_counters or None))

    def adaptive_device(self, d_llr: int, B: int, *, d_best: int, d_flags: int, d_stage=0, d_ref=0, k_payload=0,
                        d_counters=0) -> int:
        """SC first, the list decode only for the frames whose SC result fails the CRC
        (pscl_adaptive_device; N = 128, a CRC required).  Returns the escalated count."""
        n = _i64()
        with self._lock:
            check(lib().pscl_adaptive_device(self._h, d_llr, int(B), d_best, d_flags, d_stage or None, d_ref or None,
                                             int(k_payload), d_counters or None, C.byref(n)))
        return int(n.value)

    def decode_adaptive(self, llr: np.ndarray, retries: int = 0, beta=None) -> dict:
        """Host form of adaptive_device: llr [B, N] (or [B, E]) float64 -> dict(best_bits [B, K] int8,
        crc_pass [B] bool, best_idx [B] int32, stage [B] uint8 (1 SC, 2 list), n_escalated).
        retries > 0: the three-stage decode (adaptive_dlscl_device, flip metric beta) -- stage 3 where
        flips were tried, and the keys attempts [B] int32 and tried [B, retries] int32 (-1 padded)."""
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        B = llr.shape[0]
        if llr.shape[1] != (self.E or self.N):
            raise ValueError("Channel LLR length must be a power of two" if not self.E
                             else f"expected {self.E} rate-matched LLRs per frame")
        if retries > 0:
            return self._decode_three_stage(llr, B, int(retries), beta)
        with DeviceArena(self) as mem:
            d_llr = mem.alloc(max(llr.nbytes, 8))
            d_best = mem.alloc(max(B * self.W * 8, 8))
            d_flags = mem.alloc(max(B, 8))
            d_stage = mem.alloc(max(B, 8))
            if B:
                mem.upload(d_llr, llr)
            n = self.adaptive_device(d_llr, B, d_best=d_best, d_flags=d_flags, d_stage=d_stage)
            words = mem.download(d_best, max(B * self.W * 8, 8), np.uint64)[:B * self.W].reshape(B, self.W)
            flags = mem.download(d_flags, max(B, 8), np.uint8)[:B]
            stage = mem.download(d_stage, max(B, 8), np.uint8)[:B]
        j = np.arange(self.K)
        bits = ((words[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)
        return {"best_bits": bits, "crc_pass": (flags & PSCL_FLAG_CRC_PASS) != 0,
                "best_idx": (flags & PSCL_FLAG_IDX_MASK).astype(np.int32), "stage": stage.copy(), "n_escalated": n}

    def _decode_three_stage(self, llr: np.ndarray, B: int, R: int, beta) -> dict:
        with DeviceArena(self) as mem:
            d_llr = mem.alloc(max(llr.nbytes, 8))
            d_best = mem.alloc(max(B * self.W * 8, 8))
            d_flags = mem.alloc(max(B, 8))
            d_stage = mem.alloc(max(B, 8))
            d_att = mem.alloc(max(B * 4, 8))
            d_tried = mem.alloc(max(B * R * 4, 8))
            d_n = mem.alloc(8)
            mem.memset(d_n, 0, 8)
            if B:
                mem.upload(d_llr, llr)
            self.adaptive_dlscl_device(d_llr, B, R, beta=beta, d_best=d_best, d_flags=d_flags, d_stage=d_stage,
                                       d_attempts=d_att, d_tried=d_tried, tried_stride=R, d_n_escalated=d_n)
            self.sync()
            words = mem.download(d_best, max(B * self.W * 8, 8), np.uint64)[:B * self.W].reshape(B, self.W)
            flags = mem.download(d_flags, max(B, 8), np.uint8)[:B]
            stage = mem.download(d_stage, max(B, 8), np.uint8)[:B]
            att = mem.download(d_att, max(B * 4, 8), np.int32)[:B]
            tried = mem.download(d_tried, max(B * R * 4, 8), np.int32)[:B * R].reshape(B, R)
            n = int(mem.download(d_n, 8, np.int32)[0])
        j = np.arange(self.K)
        bits = ((words[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)
        return {"best_bits": bits, "crc_pass": (flags & PSCL_FLAG_CRC_PASS) != 0,
                "best_idx": (flags & PSCL_FLAG_IDX_MASK).astype(np.int32), "stage": stage.copy(), "n_escalated": n,
                "attempts": att.copy(), "tried": tried.copy()}

    def sc_device(self, d_llr: int, B: int, *, d_best: int, d_flags: int, d_stage=0, d_ref=0, k_payload=0,
                  d_counters=0) -> None:
        """sc_decode + check_crc on every frame of a device batch, enqueued without a host wait
        (pscl_sc_device; N = 32 .. 1024, rate-matched rows at N = 128 only)."""
        with self._lock:
            check(lib().pscl_sc_device(self._h, d_llr, int(B), d_best, d_flags, d_stage or None, d_ref or None,
                                       int(k_payload), d_counters or None))

    def escalate_device(self, d_llr: int, B: int, *, d_best: int, d_flags: int, d_stage=0, d_ref=0, k_payload=0,
                        d_counters=0) -> int:
        """The list decode of the frames whose d_flags lack the CRC-pass bit, in place
        (pscl_escalate_device; a CRC required).  Returns the escalated count."""
        n = _i64()
        with self._lock:
            check(lib().pscl_escalate_device(self._h, d_llr, int(B), d_best, d_flags, d_stage or None, d_ref or None,
                                             int(k_payload), d_counters or None, C.byref(n)))
        return int(n.value)

    def adaptive_async_device(self, d_llr: int, B: int, *, d_best: int, d_flags: int, d_stage=0, d_ref=0, k_payload=0,
                              d_counters=0, d_n_escalated=0) -> None:
        """The adaptive decode enqueued without a host wait (pscl_adaptive_async_device; N = 32 ..
        1024, a CRC required): SC, the compaction of the failing frames, the list decode of the
        listed rows, the statistics.  d_n_escalated: a device int32 that receives the escalated
        count.  On a pipelined handle stage 2 runs on the side stream (join() / sync() order it back)."""
        with self._lock:
            check(lib().pscl_adaptive_async_device(self._h, d_llr or None, int(B), d_best or None, d_flags or None,
                                                   d_stage or None, d_ref or None, int(k_payload), d_counters or None,
                                                   d_n_escalated or None))

    # ---- float32 rows: d_llr points at [B][N or E] float32; outputs equal the float64 calls' on the
    # widened rows (include/polar_scl.h)
    def f32_available(self) -> bool:
        """Whether decode_device_f32, escalate_device_f32 and adaptive_async_device_f32 have native
        kernels on this handle (pscl_f32_available); where not, they raise (PSCL_EUNSUP)."""
        return bool(lib().pscl_f32_available(self._h))

    def decode_device_f32(self, d_llr: int, B: int, *, d_best=0, d_flags=0, d_ref=0, k_payload=0, d_counters=0) -> None:
        """The plain list decode of float32 rows (pscl_decode_device_f32)."""
        check(lib().pscl_decode_device_f32(self._h, d_llr or None, int(B), d_best or None, d_flags or None, d_ref or None,
                                           int(k_payload), d_counters or None))

    def sc_device_f32(self, d_llr: int, B: int, *, d_best: int, d_flags: int, d_stage=0, d_ref=0, k_payload=0,
                      d_counters=0) -> None:
        """sc_device on float32 rows (pscl_sc_device_f32; N = 128, any information set)."""
        with self._lock:
            check(lib().pscl_sc_device_f32(self._h, d_llr or None, int(B), d_best or None, d_flags or None, d_stage or None,
                                           d_ref or None, int(k_payload), d_counters or None))

    def escalate_device_f32(self, d_llr: int, B: int, *, d_best: int, d_flags: int, d_stage=0, d_ref=0, k_payload=0,
                            d_counters=0) -> int:
        """escalate_device on float32 rows (pscl_escalate_device_f32).  Returns the escalated count."""
        n = _i64()
        with self._lock:
            check(lib().pscl_escalate_device_f32(self._h, d_llr or None, int(B), d_best or None, d_flags or None,
                                                 d_stage or None, d_ref or None, int(k_payload), d_counters or None,
                                                 C.byref(n)))
        return int(n.value)

    def adaptive_async_device_f32(self, d_llr: int, B: int, *, d_best: int, d_flags: int, d_stage=0, d_ref=0,
                                  k_payload=0, d_counters=0, d_n_escalated=0) -> None:
        """adaptive_async_device on float32 rows (pscl_adaptive_async_device_f32)."""
        with self._lock:
            check(lib().pscl_adaptive_async_device_f32(self._h, d_llr or None, int(B), d_best or None, d_flags or None,
                                                       d_stage or None, d_ref or None, int(k_payload),
                                                       d_counters or None, d_n_escalated or None))

    def adaptive_stats(self, reset: bool = False) -> dict:
        """Paths of the adaptive calls without a host wait (pscl_adaptive_stats): stage-2 launches on
        a row-list screening kernel, on an exact kernel, and the times a call blocked the host."""
        a, b, c = _i64(), _i64(), _i64()
        check(lib().pscl_adaptive_stats(self._h, C.byref(a), C.byref(b), C.byref(c), 1 if reset else 0))
        return {"screened": int(a.value), "exact": int(b.value), "host_waits": int(c.value)}

    def _staged_host(self, llr: np.ndarray, escalate: bool) -> dict:
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        B = llr.shape[0]
        if llr.shape[1] != (self.E or self.N):
            raise ValueError("Channel LLR length must be a power of two" if not self.E
                             else f"expected {self.E} rate-matched LLRs per frame")
        n = 0
        with DeviceArena(self) as mem:
            d_llr = mem.alloc(max(llr.nbytes, 8))
            d_best = mem.alloc(max(B * self.W * 8, 8))
            d_flags = mem.alloc(max(B, 8))
            d_stage = mem.alloc(max(B, 8))
            if B:
                mem.upload(d_llr, llr)
            self.sc_device(d_llr, B, d_best=d_best, d_flags=d_flags, d_stage=d_stage)
            if escalate:
                n = self.escalate_device(d_llr, B, d_best=d_best, d_flags=d_flags, d_stage=d_stage)
            words = mem.download(d_best, max(B * self.W * 8, 8), np.uint64)[:B * self.W].reshape(B, self.W)
            flags = mem.download(d_flags, max(B, 8), np.uint8)[:B]
            stage = mem.download(d_stage, max(B, 8), np.uint8)[:B]
        j = np.arange(self.K)
        bits = ((words[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)
        return {"best_bits": bits, "crc_pass": (flags & PSCL_FLAG_CRC_PASS) != 0,
                "best_idx": (flags & PSCL_FLAG_IDX_MASK).astype(np.int32), "stage": stage.copy(), "n_escalated": n}

    def decode_sc(self, llr: np.ndarray):
        """Host form of sc_device: llr [B, N] float64 -> (best_bits [B, K] int8, crc_pass [B] bool)."""
        out = self._staged_host(llr, escalate=False)
        return out["best_bits"], out["crc_pass"]

    def decode_staged(self, llr: np.ndarray) -> dict:
        """sc_device then escalate_device on host rows: decode_adaptive's dict, at any N >= 32."""
        return self._staged_host(llr, escalate=True)

    def channel_device(self, seed: int, stream_id: int, ebno_db: float, rate: float, k_payload: int, frame0: int,
                       B: int, d_llr: int, d_msg: int = 0) -> None:
        check(lib().pscl_channel_device(self._h, int(seed) & (2**64 - 1), int(stream_id) & 0xFFFFFFFF,
                                        float(ebno_db), float(rate), int(k_payload), int(frame0), int(B), d_llr,
                                        d_msg or None))

    # ---- caller payloads: d_payload points at [B][Wp] uint64, Wp = payload_words (include/polar_scl.h)
    @property
    def k_payload(self) -> int:
        return self.K - self.crc_deg

    @property
    def payload_words(self) -> int:
        return (self.k_payload + 63) // 64

    @property
    def code_words(self) -> int:
        return ((self.E or self.N) + 63) // 64

    def encode_device(self, d_payload: int, B: int, *, d_msg=0, d_code=0, d_sym=0, sym_f32: bool = False) -> None:
        """payload -> message words, packed transmitted bits and BPSK symbols, any subset, enqueued
        without a host wait (pscl_encode_device)."""
        check(lib().pscl_encode_device(self._h, d_payload or None, int(B), d_msg or None, d_code or None, d_sym or None,
                                       int(sym_f32)))

    def channel_payload_device(self, d_payload: int, seed: int, stream_id: int, ebno_db: float, rate: float, frame0: int,
                               B: int, *, d_llr=0, llr_f32: bool = False, d_msg=0) -> None:
        """channel_device on the caller's payloads: the same noise stream, float64 or float32 rows
        (pscl_channel_payload_device)."""
        check(lib().pscl_channel_payload_device(self._h, d_payload or None, int(seed) & (2**64 - 1),
                                                int(stream_id) & 0xFFFFFFFF, float(ebno_db), float(rate), int(frame0),
                                                int(B), d_llr or None, int(llr_f32), d_msg or None))

    def path_llrs_device(self, d_llr: int, B: int, d_bits: int, d_out: int) -> None:
        """Decision LLRs [B, K] of the paths with information bits d_bits [B, W] (replay)."""
        with self._lock:
            check(lib().pscl_path_llrs_device(self._h, d_llr, int(B), d_bits, d_out))

    def path_llrs_device_f32(self, d_llr: int, B: int, d_bits: int, d_out: int) -> None:
        """path_llrs_device on float32 rows (pscl_path_llrs_device_f32; N = 128, any information set);
        d_out stays float64."""
        with self._lock:
            check(lib().pscl_path_llrs_device_f32(self._h, d_llr, int(B), d_bits, d_out))

    def path_llrs(self, llr: np.ndarray, bits: np.ndarray) -> np.ndarray:
        """Host form of path_llrs_device: llr [B, N] (or [B, E]), bits [B, K] 0/1."""
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        B = llr.shape[0]
        words = np.zeros((B, self.W), np.uint64)
        bits = np.asarray(bits, dtype=np.uint64).reshape(B, self.K)
        for j in range(self.K):
            words[:, j >> 6] |= bits[:, j] << np.uint64(j & 63)
        with DeviceArena(self) as mem:
            d_llr = mem.alloc(llr.nbytes)
            d_bits = mem.alloc(words.nbytes)
            d_out = mem.alloc(max(B * self.K * 8, 8))
            mem.upload(d_llr, llr)
            mem.upload(d_bits, words)
            self.path_llrs_device(d_llr, B, d_bits, d_out)
            return mem.download(d_out, B * self.K * 8, np.float64).reshape(B, self.K)

    def label_device(self, d_llr: int, B: int, d_sent: int, sent_stride: int, max_flips: int, cap: int, *, d_frame: int,
                     d_abs_l0: int, d_flip: int, d_rank=0, d_counts: int) -> int:
        """Flip labels of B device-resident frames (pscl_label_device): baseline decode, |L0| order,
        forced retries on the baseline's prefix, labels.  Returns A, the number of entries; raises
        LabelCapacity (a ValueError carrying A) where A exceeds cap and nothing was written."""
        n = _i64()
        with self._lock:
            rc = lib().pscl_label_device(self._h, d_llr or None, int(B), d_sent or None, int(sent_stride), int(max_flips),
                                         int(cap), d_frame or None, d_abs_l0 or None, d_flip or None, d_rank or None,
                                         d_counts or None, C.byref(n))
        if rc == PSCL_EINVAL and n.value > int(cap):
            raise LabelCapacity(last_error(), int(n.value))
        check(rc)
        return int(n.value)

    def label(self, llr: np.ndarray, sent: np.ndarray, max_flips: int = 8, cap: int | None = None) -> dict:
        """Host form of label_device: llr [B, N] (or [B, E]) float64, sent [K] or [B, K] 0/1 ->
        dict(frame [A] int64, abs_l0 [A, K] float32, flip [A] int32, rank [A] int32, counts
        int64[PSCL_NLABEL]), entries sorted by frame.  cap: the first capacity of the output arrays
        (default label_capacity); the call is repeated once, with the count it reported, where that was short."""
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        B = llr.shape[0]
        if llr.shape[1] != (self.E or self.N):
            raise ValueError("Channel LLR length must be a power of two" if not self.E
                             else f"expected {self.E} rate-matched LLRs per frame")
        words, stride = _sent_words(sent, B, self.K, self.W)
        K = self.K
        with DeviceArena(self) as mem:
            d_llr = mem.alloc(max(llr.nbytes, 8))
            d_sent = mem.alloc(max(words.nbytes, 8))
            d_counts = mem.alloc(PSCL_NLABEL * 8)
            if B:
                mem.upload(d_llr, llr)
            mem.upload(d_sent, words)
            cap = label_capacity(B, K) if cap is None else max(int(cap), 1)
            for _ in range(2):
                d_frame, d_abs = mem.alloc(cap * 8), mem.alloc(cap * K * 4)
                d_flip, d_rank = mem.alloc(cap * 4), mem.alloc(cap * 4)
                try:
                    A = self.label_device(d_llr, B, d_sent, stride, max_flips, cap, d_frame=d_frame, d_abs_l0=d_abs,
                                          d_flip=d_flip, d_rank=d_rank, d_counts=d_counts)
                    break
                except LabelCapacity as e:  # (allocate for the count the call reported, and repeat)
                    if cap >= e.entries:
                        raise
                    cap = e.entries
            self.sync()
            counts = mem.download(d_counts, PSCL_NLABEL * 8, np.int64)
            frame = mem.download(d_frame, cap * 8, np.int64)[:A]
            abs_l0 = mem.download(d_abs, cap * K * 4, np.float32)[:A * K].reshape(A, K)
            flip = mem.download(d_flip, cap * 4, np.int32)[:A]
            rank = mem.download(d_rank, cap * 4, np.int32)[:A]
        o = np.argsort(frame, kind="stable")
        return {"frame": frame[o], "abs_l0": abs_l0[o], "flip": flip[o], "rank": rank[o], "counts": counts}

    def set_beta(self, beta: np.ndarray | None) -> None:
        """DL-SCL flip metric matrix [K, K] (None: rank by |L0|); widened to float64 exactly."""
        if beta is None:
            if self._beta is not None:
                check(lib().pscl_set_beta(self._h, None))
            self._beta = None
            return
        b = np.asarray(beta)
        if b.ndim != 2 or b.shape[0] != b.shape[1] or b.shape[0] != self.K:
            raise ValueError("beta must be a square matrix matching abs_l0 length")
        b = np.ascontiguousarray(b, dtype=np.float64)
        if self._beta is not None and np.array_equal(self._beta, b):
            return
        check(lib().pscl_set_beta(self._h, _ptr(b)))
        self._beta = b.copy()

    def dlscl_device(self, d_llr: int, B: int, retries: int, *, beta=None, d_best: int, d_flags: int,
                     d_attempts=0, d_tried=0, tried_stride=0, d_ref=0, k_payload=0, d_counters_scl=0,
                     d_counters_dl=0) -> None:
        """SCL + DL-SCL retries of B device-resident frames (pscl_dlscl_device)."""
        self.set_beta(beta)
        with self._lock:
            check(lib().pscl_dlscl_device(self._h, d_llr, int(B), int(retries), d_best, d_flags, d_attempts or None,
                                          d_tried or None, int(tried_stride), d_ref or None, int(k_payload),
                                          d_counters_scl or None, d_counters_dl or None))

    def retry_device(self, d_llr: int, B: int, retries: int, *, beta=None, d_best: int, d_flags: int, d_stage=0,
                     d_attempts=0, d_tried=0, tried_stride=0, d_ref=0, k_payload=0, d_counters_dl=0) -> None:
        """DL-SCL retry rounds on the baseline already in d_best / d_flags (pscl_retry_device): the
        frames without the CRC-pass bit enter the chains, d_stage gets 3 there, the others are left alone."""
        self.set_beta(beta)
        with self._lock:
            check(lib().pscl_retry_device(self._h, d_llr or None, int(B), int(retries), d_best or None, d_flags or None,
                                          d_stage or None, d_attempts or None, d_tried or None, int(tried_stride),
                                          d_ref or None, int(k_payload), d_counters_dl or None))

    def adaptive_dlscl_device(self, d_llr: int, B: int, retries: int, *, beta=None, d_best: int, d_flags: int,
                              d_stage=0, d_attempts=0, d_tried=0, tried_stride=0, d_ref=0, k_payload=0, d_counters=0,
                              d_n_escalated=0) -> None:
        """The three-stage decode (pscl_adaptive_dlscl_device): SC, the list decoder where SC fails the
        CRC, DL-SCL flips where the list decoder fails it too.  d_counters: device int64
        [3, PSCL_NCOUNT] (SC, adaptive, final), ADDED with d_ref.  On a pipelined handle the retry
        chains are deferred (join() / sync() order them back), as dlscl_device's."""
        self.set_beta(beta)
        with self._lock:
            check(lib().pscl_adaptive_dlscl_device(self._h, d_llr or None, int(B), int(retries), d_best or None,
                                                   d_flags or None, d_stage or None, d_attempts or None, d_tried or None,
                                                   int(tried_stride), d_ref or None, int(k_payload), d_counters or None,
                                                   d_n_escalated or None))

    def dlscl_device_f32(self, d_llr: int, B: int, retries: int, *, beta=None, d_best: int, d_flags: int,
                         d_attempts=0, d_tried=0, tried_stride=0, d_ref=0, k_payload=0, d_counters_scl=0,
                         d_counters_dl=0) -> None:
        """dlscl_device on float32 rows (pscl_dlscl_device_f32): native where f32_available(), else it
        raises (PSCL_EUNSUP)."""
        self.set_beta(beta)
        with self._lock:
            check(lib().pscl_dlscl_device_f32(self._h, d_llr or None, int(B), int(retries), d_best or None,
                                              d_flags or None, d_attempts or None, d_tried or None, int(tried_stride),
                                              d_ref or None, int(k_payload), d_counters_scl or None,
                                              d_counters_dl or None))

    def retry_device_f32(self, d_llr: int, B: int, retries: int, *, beta=None, d_best: int, d_flags: int, d_stage=0,
                         d_attempts=0, d_tried=0, tried_stride=0, d_ref=0, k_payload=0, d_counters_dl=0) -> None:
        """retry_device on float32 rows (pscl_retry_device_f32)."""
        self.set_beta(beta)
        with self._lock:
            check(lib().pscl_retry_device_f32(self._h, d_llr or None, int(B), int(retries), d_best or None,
                                              d_flags or None, d_stage or None, d_attempts or None, d_tried or None,
                                              int(tried_stride), d_ref or None, int(k_payload), d_counters_dl or None))

    def adaptive_dlscl_device_f32(self, d_llr: int, B: int, retries: int, *, beta=None, d_best: int, d_flags: int,
                                  d_stage=0, d_attempts=0, d_tried=0, tried_stride=0, d_ref=0, k_payload=0,
                                  d_counters=0, d_n_escalated=0) -> None:
        """adaptive_dlscl_device on float32 rows (pscl_adaptive_dlscl_device_f32)."""
        self.set_beta(beta)
        with self._lock:
            check(lib().pscl_adaptive_dlscl_device_f32(self._h, d_llr or None, int(B), int(retries), d_best or None,
                                                       d_flags or None, d_stage or None, d_attempts or None,
                                                       d_tried or None, int(tried_stride), d_ref or None,
                                                       int(k_payload), d_counters or None, d_n_escalated or None))

    def uncoded_device(self, seed: int, stream_id: int, ebno_db: float, k_payload: int, frame0: int, B: int,
                       d_counters: int) -> None:
        check(lib().pscl_uncoded_device(self._h, int(seed) & (2**64 - 1), int(stream_id) & 0xFFFFFFFF,
                                        float(ebno_db), int(k_payload), int(frame0), int(B), d_counters))

    def sync(self) -> None:
        check(lib().pscl_sync(self._h))

    def simulate(self, seed: int, stream_id: int, ebno_db: float, rate: float, k_payload: int, frame0: int, B: int,
                 retries: int, include_uncoded: bool = False) -> np.ndarray:
        """One SNR point in one call (pscl_simulate): int64 counters [3, PSCL_NCOUNT], rows
        SCL, DL-SCL, uncoded."""
        out = np.zeros((3, PSCL_NCOUNT), np.int64)
        with self._lock:
            check(lib().pscl_simulate(self._h, int(seed) & (2**64 - 1), int(stream_id) & 0xFFFFFFFF, float(ebno_db),
                                      float(rate), int(k_payload), int(frame0), int(B), int(retries),
                                      int(bool(include_uncoded)), out.ctypes.data))
        return out

    def simulate_device(self, seed: int, stream_id: int, ebno_db: float, rate: float, k_payload: int, frame0: int,
                        B: int, retries: int, include_uncoded: bool, d_counters: int) -> None:
        """pscl_simulate enqueued, counters ADDED into device int64 [3, PSCL_NCOUNT] at d_counters
        (complete after join()/sync(); on a pipelined handle the retry chains overlap the next call)."""
        with self._lock:
            check(lib().pscl_simulate_device(self._h, int(seed) & (2**64 - 1), int(stream_id) & 0xFFFFFFFF,
                                             float(ebno_db), float(rate), int(k_payload), int(frame0), int(B),
                                             int(retries), int(bool(include_uncoded)), d_counters))

    def simulate_adaptive(self, seed: int, stream_id: int, ebno_db: float, rate: float, k_payload: int, frame0: int,
                          B: int, include_uncoded: bool = False) -> np.ndarray:
        """One SNR point with adaptive decoding in one call (pscl_simulate_adaptive): int64 counters
        [3, PSCL_NCOUNT], rows SC, adaptive (with CNT_ESCALATED), uncoded."""
        out = np.zeros((3, PSCL_NCOUNT), np.int64)
        with self._lock:
            check(lib().pscl_simulate_adaptive(self._h, int(seed) & (2**64 - 1), int(stream_id) & 0xFFFFFFFF,
                                               float(ebno_db), float(rate), int(k_payload), int(frame0), int(B),
                                               int(bool(include_uncoded)), out.ctypes.data))
        return out

    def simulate_adaptive_device(self, seed: int, stream_id: int, ebno_db: float, rate: float, k_payload: int,
                                 frame0: int, B: int, include_uncoded: bool, d_counters: int) -> None:
        """pscl_simulate_adaptive enqueued without a host wait, counters ADDED into device int64
        [3, PSCL_NCOUNT] at d_counters (complete after sync())."""
        with self._lock:
            check(lib().pscl_simulate_adaptive_device(self._h, int(seed) & (2**64 - 1), int(stream_id) & 0xFFFFFFFF,
                                                      float(ebno_db), float(rate), int(k_payload), int(frame0), int(B),
                                                      int(bool(include_uncoded)), d_counters or None))

    def simulate_adaptive_dl(self, seed: int, stream_id: int, ebno_db: float, rate: float, k_payload: int, frame0: int,
                             B: int, retries: int, include_uncoded: bool = False) -> np.ndarray:
        """One SNR point with the three-stage decoder in one call (pscl_simulate_adaptive_dl): int64
        counters [4, PSCL_NCOUNT], rows SC, adaptive (CNT_ESCALATED), final (CNT_RETRIES), uncoded."""
        out = np.zeros((4, PSCL_NCOUNT), np.int64)
        with self._lock:
            check(lib().pscl_simulate_adaptive_dl(self._h, int(seed) & (2**64 - 1), int(stream_id) & 0xFFFFFFFF,
                                                  float(ebno_db), float(rate), int(k_payload), int(frame0), int(B),
                                                  int(retries), int(bool(include_uncoded)), out.ctypes.data))
        return out

    def simulate_adaptive_dl_device(self, seed: int, stream_id: int, ebno_db: float, rate: float, k_payload: int,
                                    frame0: int, B: int, retries: int, include_uncoded: bool, d_counters: int) -> None:
        """pscl_simulate_adaptive_dl enqueued, counters ADDED into device int64 [4, PSCL_NCOUNT] at
        d_counters (complete after join() / sync())."""
        with self._lock:
            check(lib().pscl_simulate_adaptive_dl_device(self._h, int(seed) & (2**64 - 1), int(stream_id) & 0xFFFFFFFF,
                                                         float(ebno_db), float(rate), int(k_payload), int(frame0), int(B),
                                                         int(retries), int(bool(include_uncoded)), d_counters or None))

    def screening_count(self) -> int:
        """Frames the last screening decode handed to the exact re-decode (synchronizes)."""
        n = _i64()
        check(lib().pscl_screening_count(self._h, C.byref(n)))
        return int(n.value)

    def softplus_tails(self, v: np.ndarray):
        """(exact, screening) metric tails log1p(exp(-|v|)) of v as the kernels evaluate them."""
        v = np.ascontiguousarray(v, dtype=np.float64).ravel()
        with DeviceArena(self) as mem:
            d_v, d_e, d_a = mem.alloc(v.nbytes), mem.alloc(v.nbytes), mem.alloc(v.nbytes)
            mem.upload(d_v, v)
            check(lib().pscl_softplus_tails_device(self._h, d_v, v.size, d_e, d_a))
            return mem.download(d_e, v.nbytes, np.float64), mem.download(d_a, v.nbytes, np.float64)

    def tail_abs_scan(self, lo: int = 0, hi: int = 0x7F800000, bits: bool = False):
        """Largest |screening tail - exact tail| over the fp32 bit patterns [lo, hi] and the x32
        where it occurs (pscl_tail_abs_scan_device; the default range is every x32 >= 0).  bits:
        the bits form of the lane kernels' plain decodes (pscl_tail2_scan_device)."""
        fn = lib().pscl_tail2_scan_device if bits else lib().pscl_tail_abs_scan_device
        with DeviceArena(self) as mem:
            d = mem.alloc(16)
            mem.memset(d, 0, 16)
            check(fn(self._h, int(lo), int(hi), d))
            out = mem.download(d, 16, np.uint64)
        err = float(out[:1].view(np.float64)[0])
        x32 = float(np.array([int(out[1]) & 0xFFFFFFFF], np.uint32).view(np.float32)[0])
        return err, x32

    def set_pipelined(self, on: bool = True, depth: int = 2) -> None:
        """Throughput mode for streams of plain decodes (include/polar_scl.h): a screening
        decode's exact re-decode overlaps the next decode; join() / sync() order it back.  depth
        (1..4): a DL-SCL call's buffers are free again at the depth-th following call -- at the
        second at the earliest, so depth 1 behaves as 2 (a call's chains always overlap the next
        call's baseline)."""
        if not 1 <= int(depth) <= 4:
            raise ValueError(f"pipelined depth must be 1..4 (got {depth})")
        check(lib().pscl_set_pipelined(self._h, (int(depth) if depth > 2 else 1) if on else 0))

    def join(self) -> None:
        """Order pending pipelined work into the handle's stream: the plain decodes' re-decodes
        without a host wait; a pending pipelined DL-SCL call's chains are enqueued here, which
        waits on the host for that call's baseline decode (its failing-frame count)."""
        check(lib().pscl_join(self._h))

    def set_tuning(self, **knobs) -> None:
        """Schedule knobs of this handle (pscl_set_tuning; 0 = default): dl_screen, dl_chunks,
        dl_split, side_priority, post_grid, retry_wpg.  Results never depend on them."""
        for k, v in knobs.items():
            if k not in TUNE:
                raise ValueError(f"unknown tuning knob {k!r}")
            check(lib().pscl_set_tuning(self._h, TUNE[k], int(v)))
            tun = self.__dict__.setdefault("_tuning", {})
            tun[k] = int(v)

    def get_tuning(self) -> dict:
        """The knobs set on this handle through set_tuning (0 = default for any other knob)."""
        return dict(self.__dict__.get("_tuning", {}))

    def set_screening(self, on: bool = True) -> None:
        """Screening decode for plain decodes (default on; include/polar_scl.h)."""
        check(lib().pscl_set_screening(self._h, 1 if on else 0))

    def timing_enable(self, on: bool = True) -> None:
        check(lib().pscl_timing_enable(self._h, 1 if on else 0))

    def timing_read(self):
        n, ms = _i64(), _dbl()
        check(lib().pscl_timing_read(self._h, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def timing_read_split(self):
        """((launches, ms) on the handle's stream, (launches, ms) on its side streams)."""
        n0, t0, n1, t1 = _i64(), _dbl(), _i64(), _dbl()
        check(lib().pscl_timing_read_split(self._h, C.byref(n0), C.byref(t0), C.byref(n1), C.byref(t1)))
        return (int(n0.value), float(t0.value)), (int(n1.value), float(t1.value))

    def host_stats(self, reset: bool = False):
        """(call ms, wait ms, calls) of the DL-SCL calls on the host (pscl_host_stats)."""
        c, w, n = _dbl(), _dbl(), _i64()
        check(lib().pscl_host_stats(self._h, C.byref(c), C.byref(w), C.byref(n), 1 if reset else 0))
        return float(c.value), float(w.value), int(n.value)

    def path_stats(self) -> dict:
        """Schedules enqueued so far (pscl_path_stats): fused-post rounds, separate-post rounds,
        fused-TX blocks, 4-entry-form post launches, exact lane-per-path launches."""
        a, b, c, d, x = _i64(), _i64(), _i64(), _i64(), _i64()
        check(lib().pscl_path_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(x)))
        return {"fused_post_rounds": int(a.value), "post_rounds": int(b.value), "fused_tx_blocks": int(c.value),
                "post_epw4_launches": int(d.value), "lane_exact_launches": int(x.value)}

    def launch_info(self, B: int):
        w, g, lds = C.c_int(), _i64(), C.c_int()
        check(lib().pscl_launch_info(self._h, int(B), C.byref(w), C.byref(g), C.byref(lds)))
        return int(w.value), int(g.value), int(lds.value)


class CpuDecoder:
    """The product's host decoder (pscl_decode_cpu): Decoder.decode's contract and outputs, bit for
    bit, with no GPU -- the reference's CPU-only runs (BASELINE config 1).  device = "cpu"."""

    def __init__(self, N: int, info_set, L: int, crc=None, threads: int = 0):
        info = np.ascontiguousarray(np.asarray(info_set).astype(np.int32).ravel())
        self.N, self.K, self.L = int(N), int(info.size), int(L)
        self.info_set = info
        self.crc_poly = poly_value(crc)
        self.crc_deg = max(self.crc_poly.bit_length() - 1, 0)
        self.W = (self.K + 63) // 64 if self.K else 1
        self.E = 0
        self.device = "cpu"
        self.threads = int(threads or os.environ.get("PSCL_CPU_THREADS", "0") or 0)
        if self.N < 2 or self.N & (self.N - 1) or self.N > PSCL_MAX_N:
            raise ValueError("Channel LLR length must be a power of two")
        if self.crc_poly and self.K <= self.crc_deg:
            raise ValueError("Message too short for the provided CRC polynomial")

    def decode(self, llr: np.ndarray, forced: np.ndarray | None = None, *, want_metrics=True,
               want_cands=True, want_info_llrs=True):
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        B = llr.shape[0]
        if llr.shape[1] != self.N:
            raise ValueError("Channel LLR length must be a power of two")
        if forced is not None:
            forced = np.ascontiguousarray(forced, dtype=np.int8).reshape(B, self.K)
            if np.any((forced < -1) | (forced > 1)):
                raise ValueError("force_info_bits entries must be -1, 0, or 1")
        out = {
            "n_paths": np.zeros(B, np.int32),
            "best_bits": np.zeros((B, self.K), np.int8),
            "crc_pass": np.zeros(B, np.uint8),
            "best_idx": np.zeros(B, np.int32),
            "metrics": np.full((B, self.L), np.nan) if want_metrics else None,
            "cands": np.zeros((B, self.L, self.K), np.int8) if want_cands else None,
            "info_llrs": np.full((B, self.L, self.K), np.nan) if want_info_llrs else None,
        }
        check(lib().pscl_decode_cpu(self.N, self.info_set.ctypes.data_as(C.POINTER(_i32)), self.K, self.L,
                                    self.crc_poly, _ptr(llr), B, _ptr(forced), _ptr(out["n_paths"]),
                                    _ptr(out["best_bits"]), _ptr(out["crc_pass"]), _ptr(out["best_idx"]),
                                    _ptr(out["metrics"]), _ptr(out["cands"]), _ptr(out["info_llrs"]), self.threads))
        out["crc_pass"] = out["crc_pass"].astype(bool)
        return out

    def decode_adaptive(self, llr: np.ndarray) -> dict:
        """Decoder.decode_adaptive on the host (pscl_decode_adaptive_cpu), same keys."""
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        B = llr.shape[0]
        if llr.shape[1] != self.N:
            raise ValueError("Channel LLR length must be a power of two")
        bits = np.zeros((B, self.K), np.int8)
        ok, idx, stage = np.zeros(B, np.uint8), np.zeros(B, np.int32), np.zeros(B, np.uint8)
        check(lib().pscl_decode_adaptive_cpu(self.N, self.info_set.ctypes.data_as(C.POINTER(_i32)), self.K, self.L,
                                             self.crc_poly, _ptr(llr), B, _ptr(bits), _ptr(ok), _ptr(idx), _ptr(stage),
                                             self.threads))
        return {"best_bits": bits, "crc_pass": ok.astype(bool), "best_idx": idx, "stage": stage,
                "n_escalated": int(np.count_nonzero(stage == 2))}

    def path_llrs(self, llr: np.ndarray, bits: np.ndarray) -> np.ndarray:
        """Decoder.path_llrs on the host (pscl_path_llrs_cpu): llr [B, N], bits [B, K] 0/1 ->
        decision LLRs [B, K] of the paths with those information bits."""
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        B = llr.shape[0]
        if llr.shape[1] != self.N:
            raise ValueError("Channel LLR length must be a power of two")
        bits = np.ascontiguousarray(np.asarray(bits).reshape(B, self.K), dtype=np.int8)
        out = np.zeros((B, self.K), np.float64)
        if B:
            check(lib().pscl_path_llrs_cpu(self.N, self.info_set.ctypes.data_as(C.POINTER(_i32)), self.K, _ptr(llr), B,
                                           _ptr(bits), _ptr(out), self.threads))
        return out

    def label(self, llr: np.ndarray, sent: np.ndarray, max_flips: int = 8) -> dict:
        """Decoder.label on the host (pscl_label_cpu), same keys; entries in frame order."""
        llr = np.ascontiguousarray(llr, dtype=np.float64)
        if llr.ndim == 1:
            llr = llr[None, :]
        B, K = llr.shape[0], self.K
        if llr.shape[1] != self.N:
            raise ValueError("Channel LLR length must be a power of two")
        one = np.asarray(sent).ndim == 1
        s = _sent_bits(sent, B, K)
        frame, abs_l0 = np.zeros(B, np.int64), np.zeros((B, K), np.float32)
        flip, rank = np.zeros(B, np.int32), np.zeros(B, np.int32)
        counts = np.zeros(PSCL_NLABEL, np.int64)
        rc = lib().pscl_label_cpu(self.N, self.info_set.ctypes.data_as(C.POINTER(_i32)), K, self.L, self.crc_poly, _ptr(llr),
                                  B, _ptr(s), 0 if one else K, int(max_flips), _ptr(frame), _ptr(abs_l0), _ptr(flip),
                                  _ptr(rank), _ptr(counts), self.threads)
        if rc == PSCL_EINVAL:
            raise ValueError("invalid code, CRC (one is required), max_flips (1..32) or shapes for pscl_label_cpu")
        check(rc)
        A = int(counts[LBL_ENTRIES])
        return {"frame": frame[:A].copy(), "abs_l0": abs_l0[:A].copy(), "flip": flip[:A].copy(), "rank": rank[:A].copy(),
                "counts": counts}

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass


def encode_cpu(N: int, info_set, crc, payload_words: np.ndarray, E: int = 0):
    """Decoder.encode_device's message and code words on the host (pscl_encode_cpu; no GPU):
    payload_words [B, Wp] uint64 -> (msg [B, W] uint64, code [B, ceil((E or N) / 64)] uint64)."""
    info = np.ascontiguousarray(np.asarray(info_set).astype(np.int32).ravel())
    N, K, E, poly = int(N), int(info.size), int(E), poly_value(crc)
    kp = K - max(poly.bit_length() - 1, 0)
    pw = np.ascontiguousarray(payload_words, dtype=np.uint64)
    if pw.ndim != 2 or pw.shape[1] != (max(kp, 0) + 63) // 64:
        raise ValueError(f"payload_words must be [B, {(max(kp, 0) + 63) // 64}] uint64 words")
    B = pw.shape[0]
    msg = np.zeros((B, (K + 63) // 64 if K > 64 else 1), np.uint64)
    code = np.zeros((B, (max(E or N, 1) + 63) // 64), np.uint64)
    rc = lib().pscl_encode_cpu(N, info.ctypes.data_as(C.POINTER(_i32)), K, poly, E, _ptr(pw), B, _ptr(msg), _ptr(code))
    if rc == PSCL_EINVAL:
        raise ValueError("invalid code, CRC or rate-matched length for pscl_encode_cpu")
    if rc == PSCL_EUNSUP:
        raise NotImplementedError("repetition (E > N) needs N >= 32; CRC degree <= 32")
    return msg, code


_CACHE: dict = {}
_CACHE_LOCK = threading.Lock()


def get_decoder(N: int, info_set, L: int, crc=None, device: int = 0, E: int = 0, slot: int = 0) -> Decoder:
    """Cached Decoder per (N, info set, L, CRC, device, rate-matched length E, slot).  Distinct
    slots are distinct handles (own streams and scratch), for concurrent host threads."""
    info = np.asarray(info_set).astype(np.int64).ravel()
    cpu = isinstance(device, str) and device == "cpu"
    key = (int(N), info.tobytes(), int(L), poly_value(crc), "cpu" if cpu else int(device), int(E), int(slot))
    with _CACHE_LOCK:
        dec = _CACHE.get(key)
        if dec is None:
            if len(_CACHE) > 64:
                _CACHE.clear()
            if cpu:
                if E:
                    raise NotImplementedError("the CPU decoder takes internal (de-rate-matched) LLRs")
                dec = _CACHE[key] = CpuDecoder(N, info, L, crc)
                return dec
            dec = Decoder(N, info, L, crc, device)
            if E:
                dec.set_rate_match(E)
            _CACHE[key] = dec
        return dec


def release_decoders() -> None:
    """Close every cached decoder (get_decoder): their handles, streams and device scratch go.  A
    long-lived process that is done with a workload calls this so that the next one's streams are
    not spread over hardware queues shared with idle ones.  Every Decoder an earlier get_decoder()
    returned is closed too (flip.decode_with_retries_device and the sweeps share them): using one
    afterwards raises RuntimeError; call get_decoder() again for a fresh handle."""
    with _CACHE_LOCK:
        decs = list(_CACHE.values())
        _CACHE.clear()
    for d in decs:
        d.close()


class DeviceArena:
    """Device buffers owned through the C ABI (pscl_device_alloc), freed on exit.  Lets the
    host layer drive the device path without PyTorch."""

    def __init__(self, dec: Decoder):
        self.dec = dec
        self.ptrs: list[int] = []

    def __enter__(self) -> "DeviceArena":
        return self

    def __exit__(self, *exc) -> None:
        self.dec.sync()
        for p in self.ptrs:
            lib().pscl_device_free(self.dec.handle, p)
        self.ptrs.clear()

    def alloc(self, nbytes: int) -> int:
        p = _vp()
        check(lib().pscl_device_alloc(self.dec.handle, C.byref(p), int(nbytes)))
        self.ptrs.append(p.value)
        return p.value

    def memset(self, d_ptr: int, value: int, nbytes: int) -> None:
        check(lib().pscl_memset_device(self.dec.handle, d_ptr, int(value), int(nbytes)))

    def upload(self, d_ptr: int, arr: np.ndarray) -> None:
        arr = np.ascontiguousarray(arr)
        check(lib().pscl_memcpy_htod(self.dec.handle, d_ptr, arr.ctypes.data, arr.nbytes))

    def download(self, d_ptr: int, nbytes: int, dtype) -> np.ndarray:
        out = np.empty(int(nbytes) // np.dtype(dtype).itemsize, dtype=dtype)
        check(lib().pscl_memcpy_dtoh(self.dec.handle, out.ctypes.data, d_ptr, out.nbytes))
        return out
