"""Successive-cancellation list decoding on the MI355X (mirror of dl_scl_polar/polar/scl.py).

`decode_scl` keeps the reference signature and return dict (scl.py:108-209) and runs one
frame through libpolar_mi355x.so.  `SCLDecoder` is the batch API the reference lacks: it
decodes [B, N] LLRs per call, on host arrays or on device-resident torch tensors.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import _native


def _validate(llr, info_set, M, force_info_bits):
    if M <= 0:
        raise ValueError("List size M must be positive")
    info_set = np.asarray(info_set)
    if info_set.ndim != 1:
        raise ValueError("info_set must be a 1D array")
    if force_info_bits is not None:
        force_info_bits = np.asarray(force_info_bits)
        if force_info_bits.ndim != 1:
            raise ValueError("force_info_bits must be 1D when provided")
        if force_info_bits.size != info_set.size:
            raise ValueError("force_info_bits length must match info_set")
        force_info_bits = force_info_bits.astype(np.int8)
    llr = np.asarray(llr).astype(float).ravel()
    N = llr.size
    if N <= 0 or (N & (N - 1)):
        raise ValueError("Channel LLR length must be a power of two")
    return llr, info_set, force_info_bits


def decode_scl(
    llr: np.ndarray,
    info_set: np.ndarray,
    M: int,
    crc: Optional[str] = None,
    *,
    force_info_bits: Optional[np.ndarray] = None,
    device: int = 0,
) -> dict:
    """Decode one frame with SCL (list size M) and optional CRC selection (scl.py:108-209).

    Returns the reference's dict: candidates (list of int8[K], list order), metrics
    (list of float), best_path_bits (first CRC-passing candidate, else the first),
    info_llrs (decision LLR at each information phase, per candidate) and
    best_path_info_llrs.
    """
    llr, info_set, force = _validate(llr, info_set, M, force_info_bits)
    dec = _native.get_decoder(llr.size, info_set, int(M), crc, device)
    out = dec.decode(llr[None, :], None if force is None else force[None, :])
    n = int(out["n_paths"][0])
    candidates = [out["cands"][0, i].copy() for i in range(n)]
    metrics = [float(m) for m in out["metrics"][0, :n]]
    info_llrs = [out["info_llrs"][0, i].copy() for i in range(n)]
    b = int(out["best_idx"][0]) if n else None
    return {
        "candidates": candidates,
        "metrics": metrics,
        "best_path_bits": candidates[b] if b is not None else None,
        "info_llrs": info_llrs,
        "best_path_info_llrs": info_llrs[b] if b is not None else None,
    }


class SCLDecoder:
    """Frame-batched SCL decoder bound to one GPU.

    SCLDecoder(N, info_set, L, crc_poly="0x1864CFB", device=0).decode(llr[B, N]) returns a
    dict with bits [B, K] int8 (best_path_bits), crc_pass [B] bool, best_idx [B],
    n_paths [B], and, when requested, metrics [B, L], cands [B, L, K], info_llrs [B, L, K].
    """

    def __init__(self, N: int, info_set, L: int, crc_poly: Optional[str] = "0x1864CFB", device: int = 0):
        if L <= 0:
            raise ValueError("List size M must be positive")
        self.N, self.L, self.crc_poly, self.device = int(N), int(L), crc_poly, int(device)
        self.info_set = np.asarray(info_set).astype(np.int32)
        self.K = self.info_set.size
        self._dec = _native.Decoder(self.N, self.info_set, self.L, crc_poly, self.device)

    @property
    def native(self) -> _native.Decoder:
        return self._dec

    def decode(self, llr: np.ndarray, forced: Optional[np.ndarray] = None, *, metrics: bool = False,
               candidates: bool = False, info_llrs: bool = False) -> dict:
        out = self._dec.decode(llr, forced, want_metrics=metrics, want_cands=candidates,
                               want_info_llrs=info_llrs)
        out["bits"] = out.pop("best_bits")
        return {k: v for k, v in out.items() if v is not None}

    @staticmethod
    def _f32_rows(llr, row: int) -> bool:
        """Validate llr for the tensor methods -- a contiguous [B, row] tensor of float64 or float32;
        anything else raises ValueError before any device call -- and say whether it is float32."""
        import torch

        if llr.dtype not in (torch.float64, torch.float32) or not llr.is_contiguous() or llr.dim() != 2 or llr.shape[1] != row:
            raise ValueError("llr must be a contiguous float64 or float32 [B, N] tensor")
        return llr.dtype == torch.float32

    def decode_tensor(self, llr, forced_words=None, ref_words=None, k_payload: int = 0, counters=None):
        """Device path: llr is a contiguous float64 or float32 torch tensor [B, N] on this GPU.
        Returns (best_words [B, W] int64, flags [B] uint8) tensors; when ref_words is given,
        error statistics are added into `counters` (int64[8] tensor).

        float32 rows take the native float32 decode (pscl_decode_device_f32) where the handle has
        one (native.f32_available(): N = 128, L = 4 or 8, screening on, a compiled-in code) and no
        forced bits are given; elsewhere they are widened with llr.double() and take the float64
        call.  Either way the result is the float64 result on the widened rows.  (The widened copy
        is a temporary of this call: on a pipelined handle the fallback joins the side-stream work
        back into the stream before it returns, so nothing reads the copy after torch frees it.)"""
        import torch

        f32 = self._f32_rows(llr, self.N)
        B = llr.shape[0]
        W = self._dec.W
        best = torch.empty((B, W), dtype=torch.int64, device=llr.device)
        flags = torch.empty((B,), dtype=torch.uint8, device=llr.device)
        self._dec.set_stream(torch.cuda.current_stream(llr.device).cuda_stream)
        if f32 and forced_words is None and self._dec.f32_available():
            self._dec.decode_device_f32(
                llr.data_ptr(), B, d_best=best.data_ptr(), d_flags=flags.data_ptr(),
                d_ref=ref_words.data_ptr() if ref_words is not None else 0, k_payload=k_payload,
                d_counters=counters.data_ptr() if counters is not None else 0)
            return best, flags
        if f32:
            llr = llr.double()
        self._dec.decode_device(
            llr.data_ptr(), B,
            d_force=forced_words.data_ptr() if forced_words is not None else 0,
            d_best=best.data_ptr(), d_flags=flags.data_ptr(),
            d_ref=ref_words.data_ptr() if ref_words is not None else 0, k_payload=k_payload,
            d_counters=counters.data_ptr() if counters is not None else 0)
        if f32:
            self._dec.join()  # (the widened temporary: see above)
        return best, flags

    def decode_adaptive(self, llr: np.ndarray) -> dict:
        """SC first, the list decode only for the frames whose SC result fails the CRC
        (pscl_adaptive_device): bits [B, K] int8, crc_pass [B] bool, best_idx [B], stage [B]
        (1 SC, 2 list) and n_escalated.  N = 128 and a CRC are required."""
        out = self._dec.decode_adaptive(llr)
        out["bits"] = out.pop("best_bits")
        return out

    def decode_tensor_adaptive(self, llr, ref_words=None, k_payload: int = 0, counters=None):
        """Device path of decode_adaptive on the caller's current torch stream, mirroring
        decode_tensor: returns (best_words [B, W] int64, flags [B] uint8, stage [B] uint8) tensors;
        with ref_words the final outputs' error statistics and the escalated count are added
        into `counters` (int64[8] tensor).  The call waits once on the host, after the SC stage."""
        import torch

        row = self._dec.E or self.N
        if llr.dtype != torch.float64 or not llr.is_contiguous() or llr.dim() != 2 or llr.shape[1] != row:
            raise ValueError("llr must be a contiguous float64 [B, N] tensor")
        B = llr.shape[0]
        W = self._dec.W
        best = torch.empty((B, W), dtype=torch.int64, device=llr.device)
        flags = torch.empty((B,), dtype=torch.uint8, device=llr.device)
        stage = torch.empty((B,), dtype=torch.uint8, device=llr.device)
        self._dec.set_stream(torch.cuda.current_stream(llr.device).cuda_stream)
        self._dec.adaptive_device(
            llr.data_ptr(), B, d_best=best.data_ptr(), d_flags=flags.data_ptr(), d_stage=stage.data_ptr(),
            d_ref=ref_words.data_ptr() if ref_words is not None else 0, k_payload=k_payload,
            d_counters=counters.data_ptr() if counters is not None else 0)
        return best, flags, stage

    def decode_tensor_adaptive_async(self, llr, ref_words=None, k_payload: int = 0, counters=None):
        """decode_tensor_adaptive without the host wait (pscl_adaptive_async_device, N = 32 .. 1024):
        everything is enqueued on the caller's current torch stream and the call returns.  Returns
        (best_words [B, W] int64, flags [B] uint8, stage [B] uint8, n_escalated [1] int32) tensors;
        with ref_words the final outputs' error statistics and the escalated count are added into
        `counters` (int64[8] tensor).  float32 rows: pscl_adaptive_async_device_f32 where
        native.f32_available(), else widened with llr.double() (see decode_tensor)."""
        import torch

        f32 = self._f32_rows(llr, self._dec.E or self.N)
        call = self._dec.adaptive_async_device
        if f32 and self._dec.f32_available():
            call = self._dec.adaptive_async_device_f32
        elif f32:
            llr = llr.double()
        B = llr.shape[0]
        W = self._dec.W
        best = torch.empty((B, W), dtype=torch.int64, device=llr.device)
        flags = torch.empty((B,), dtype=torch.uint8, device=llr.device)
        stage = torch.empty((B,), dtype=torch.uint8, device=llr.device)
        n_esc = torch.empty((1,), dtype=torch.int32, device=llr.device)
        self._dec.set_stream(torch.cuda.current_stream(llr.device).cuda_stream)
        call(
            llr.data_ptr(), B, d_best=best.data_ptr(), d_flags=flags.data_ptr(), d_stage=stage.data_ptr(),
            d_ref=ref_words.data_ptr() if ref_words is not None else 0, k_payload=k_payload,
            d_counters=counters.data_ptr() if counters is not None else 0, d_n_escalated=n_esc.data_ptr())
        if f32 and call == self._dec.adaptive_async_device:
            self._dec.join()  # (the widened temporary: see decode_tensor)
        return best, flags, stage, n_esc

    def decode_sc(self, llr: np.ndarray):
        """sc_decode + check_crc on every frame (pscl_sc_device, N = 32 .. 1024): (bits [B, K] int8,
        crc_pass [B] bool)."""
        return self._dec.decode_sc(llr)

    def decode_tensor_sc(self, llr, ref_words=None, k_payload: int = 0, counters=None):
        """Device path of decode_sc on the caller's current torch stream, without a host wait: returns
        (best_words [B, W] int64, flags [B] uint8, stage [B] uint8) tensors.  float32 rows:
        pscl_sc_device_f32 at N = 128 (any information set), else widened with llr.double()."""
        import torch

        f32 = self._f32_rows(llr, self._dec.E or self.N)
        sc = self._dec.sc_device
        if f32 and self.N == 128:
            sc = self._dec.sc_device_f32
        elif f32:
            llr = llr.double()
        B = llr.shape[0]
        best = torch.empty((B, self._dec.W), dtype=torch.int64, device=llr.device)
        flags = torch.empty((B,), dtype=torch.uint8, device=llr.device)
        stage = torch.empty((B,), dtype=torch.uint8, device=llr.device)
        self._dec.set_stream(torch.cuda.current_stream(llr.device).cuda_stream)
        sc(llr.data_ptr(), B, d_best=best.data_ptr(), d_flags=flags.data_ptr(), d_stage=stage.data_ptr(),
           d_ref=ref_words.data_ptr() if ref_words is not None else 0, k_payload=k_payload,
           d_counters=counters.data_ptr() if counters is not None else 0)
        return best, flags, stage

    def decode_staged(self, llr: np.ndarray) -> dict:
        """decode_adaptive's result at any N >= 32, as the SC stage followed by the escalation
        (pscl_sc_device, pscl_escalate_device)."""
        out = self._dec.decode_staged(llr)
        out["bits"] = out.pop("best_bits")
        return out

    def decode_tensor_staged(self, llr, ref_words=None, k_payload: int = 0, counters=None):
        """Device path of decode_staged on the caller's current torch stream: returns
        decode_tensor_adaptive's tensors.  The call waits once on the host, inside the escalation.
        float32 rows: pscl_sc_device_f32 and pscl_escalate_device_f32 where native.f32_available(),
        else widened with llr.double() (see decode_tensor)."""
        import torch

        f32 = self._f32_rows(llr, self._dec.E or self.N)
        sc, esc = self._dec.sc_device, self._dec.escalate_device
        if f32 and self._dec.f32_available():
            sc, esc = self._dec.sc_device_f32, self._dec.escalate_device_f32
        elif f32:
            llr = llr.double()
        B = llr.shape[0]
        W = self._dec.W
        best = torch.empty((B, W), dtype=torch.int64, device=llr.device)
        flags = torch.empty((B,), dtype=torch.uint8, device=llr.device)
        stage = torch.empty((B,), dtype=torch.uint8, device=llr.device)
        self._dec.set_stream(torch.cuda.current_stream(llr.device).cuda_stream)
        out = dict(d_best=best.data_ptr(), d_flags=flags.data_ptr(), d_stage=stage.data_ptr())
        sc(llr.data_ptr(), B, **out)
        esc(
            llr.data_ptr(), B, **out, d_ref=ref_words.data_ptr() if ref_words is not None else 0, k_payload=k_payload,
            d_counters=counters.data_ptr() if counters is not None else 0)
        return best, flags, stage


__all__ = ["decode_scl", "SCLDecoder"]
