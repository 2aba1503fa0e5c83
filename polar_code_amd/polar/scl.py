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

    def __init__(self, N: int, info_set, L: int, crc_poly: Optional[str] = "0x1864CFB", device=0):
        if L <= 0:
            raise ValueError("List size M must be positive")
        cpu = isinstance(device, str) and device == "cpu"
        self.N, self.L, self.crc_poly, self.device = int(N), int(L), crc_poly, "cpu" if cpu else int(device)
        self.info_set = np.asarray(info_set).astype(np.int32)
        self.K = self.info_set.size
        # device="cpu": the host decoder and encoder (pscl_decode_cpu, pscl_encode_cpu); no tensor methods
        self._dec = (_native.CpuDecoder(self.N, self.info_set, self.L, crc_poly) if cpu
                     else _native.Decoder(self.N, self.info_set, self.L, crc_poly, self.device))
        self.k_payload = self.K - self._dec.crc_deg
        self.payload_words = (self.k_payload + 63) // 64

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

    # ---- DL-SCL on tensors: the retry chains after a list decode, an adaptive decode or the caller's baseline
    def _dl_call(self, llr, name):
        """The float64 or float32 form of the native DL-SCL call `name` for llr (validated first), the
        rows it takes and whether they are a widened temporary: float32 rows natively where
        native.f32_available(), else widened with llr.double() (see decode_tensor)."""
        f32 = self._f32_rows(llr, self._dec.E or self.N)
        if f32 and self._dec.f32_available():
            return getattr(self._dec, name + "_f32"), llr, False
        return getattr(self._dec, name), (llr.double() if f32 else llr), f32

    def _dl_outputs(self, llr, retries: int):
        import torch

        B, rounds = llr.shape[0], max(0, min(int(retries), self.K)) if self._dec.crc_deg else 0
        attempts = torch.empty((B,), dtype=torch.int32, device=llr.device)
        tried = torch.empty((B, rounds), dtype=torch.int32, device=llr.device)
        return attempts, tried, dict(d_attempts=attempts.data_ptr(), d_tried=tried.data_ptr() if rounds else 0,
                                     tried_stride=rounds)

    def decode_tensor_dlscl(self, llr, retries: int, beta=None, ref_words=None, k_payload: int = 0, counters=None):
        """SCL + DL-SCL retries (pscl_dlscl_device; flip.py:65-141 per frame) on the caller's current
        torch stream: llr is a contiguous float64 or float32 [B, N] (or [B, E]) tensor on this GPU,
        beta the [K, K] flip metric matrix or None (rank by |L0|).  Returns (best_words [B, W] int64,
        flags [B] uint8, attempts [B] int32 = 1 + flips tried, tried [B, min(retries, K)] int32 = the
        flip indices in order, -1 padded).  With ref_words the baseline's statistics are added into
        counters[0] and the final outputs' into counters[1] (`counters`: int64 [2, 8] tensor).
        float32 rows: pscl_dlscl_device_f32 where native.f32_available(), else widened with
        llr.double(); either way the result is the float64 result on the widened rows.  On a
        pipelined handle the retry chains are deferred: native.join() orders them back."""
        import torch

        call, rows, widened = self._dl_call(llr, "dlscl_device")
        B, W = rows.shape[0], self._dec.W
        best = torch.empty((B, W), dtype=torch.int64, device=rows.device)
        flags = torch.empty((B,), dtype=torch.uint8, device=rows.device)
        attempts, tried, out = self._dl_outputs(rows, retries)
        self._dec.set_stream(torch.cuda.current_stream(rows.device).cuda_stream)
        call(rows.data_ptr(), B, int(retries), beta=beta, d_best=best.data_ptr(), d_flags=flags.data_ptr(), **out,
             d_ref=ref_words.data_ptr() if ref_words is not None else 0, k_payload=k_payload,
             d_counters_scl=counters.data_ptr() if counters is not None else 0,
             d_counters_dl=counters.data_ptr() + 8 * _native.PSCL_NCOUNT if counters is not None else 0)
        if widened:
            self._dec.join()  # (the widened temporary: see decode_tensor)
        return best, flags, attempts, tried

    def decode_tensor_retry(self, llr, best, flags, retries: int, beta=None, stage=None, ref_words=None,
                            k_payload: int = 0, counters=None):
        """DL-SCL retry rounds on a baseline the caller holds (pscl_retry_device): `best` [B, W] int64
        and `flags` [B] uint8 are what this decoder's list decode left (decode_tensor, the adaptive and
        staged methods); the frames without the CRC-pass bit enter the chains, and best, flags and
        `stage` ([B] uint8 or None: 3 at those frames) are updated in place.  Returns (attempts [B]
        int32, tried [B, min(retries, K)] int32).  With ref_words the final outputs' statistics are
        added into `counters` (int64[8] tensor).  float32 rows as decode_tensor_dlscl."""
        import torch

        call, rows, widened = self._dl_call(llr, "retry_device")
        B, W = rows.shape[0], self._dec.W
        if (best.dtype != torch.int64 or not best.is_contiguous() or tuple(best.shape) != (B, W)
                or flags.dtype != torch.uint8 or not flags.is_contiguous() or tuple(flags.shape) != (B,)
                or (stage is not None and (stage.dtype != torch.uint8 or not stage.is_contiguous()
                                           or tuple(stage.shape) != (B,)))):
            raise ValueError("best must be a contiguous int64 [B, W] tensor, flags and stage contiguous uint8 [B]")
        attempts, tried, out = self._dl_outputs(rows, retries)
        self._dec.set_stream(torch.cuda.current_stream(rows.device).cuda_stream)
        call(rows.data_ptr(), B, int(retries), beta=beta, d_best=best.data_ptr(), d_flags=flags.data_ptr(),
             d_stage=stage.data_ptr() if stage is not None else 0, **out,
             d_ref=ref_words.data_ptr() if ref_words is not None else 0, k_payload=k_payload,
             d_counters_dl=counters.data_ptr() if counters is not None else 0)
        if widened:
            self._dec.join()  # (the widened temporary: see decode_tensor)
        return attempts, tried

    def decode_tensor_adaptive_dlscl(self, llr, retries: int, beta=None, ref_words=None, k_payload: int = 0,
                                     counters=None):
        """The three-stage decode (pscl_adaptive_dlscl_device): SC, the list decoder where SC fails the
        CRC, DL-SCL flips where the list decoder fails it too, on the caller's current torch stream.
        Returns (best_words [B, W] int64, flags [B] uint8, stage [B] uint8 = 1, 2 or 3, attempts [B]
        int32, tried [B, min(retries, K)] int32, n_escalated [1] int32).  With ref_words the
        statistics are added into `counters` (int64 [3, 8] tensor: SC, adaptive, final).  float32 rows
        as decode_tensor_dlscl (pscl_adaptive_dlscl_device_f32 where native.f32_available())."""
        import torch

        call, rows, widened = self._dl_call(llr, "adaptive_dlscl_device")
        B, W = rows.shape[0], self._dec.W
        best = torch.empty((B, W), dtype=torch.int64, device=rows.device)
        flags = torch.empty((B,), dtype=torch.uint8, device=rows.device)
        stage = torch.empty((B,), dtype=torch.uint8, device=rows.device)
        n_esc = torch.zeros((1,), dtype=torch.int32, device=rows.device)
        attempts, tried, out = self._dl_outputs(rows, retries)
        self._dec.set_stream(torch.cuda.current_stream(rows.device).cuda_stream)
        call(rows.data_ptr(), B, int(retries), beta=beta, d_best=best.data_ptr(), d_flags=flags.data_ptr(),
             d_stage=stage.data_ptr(), **out, d_ref=ref_words.data_ptr() if ref_words is not None else 0,
             k_payload=k_payload, d_counters=counters.data_ptr() if counters is not None else 0,
             d_n_escalated=n_esc.data_ptr())
        if widened:
            self._dec.join()  # (the widened temporary: see decode_tensor)
        return best, flags, stage, attempts, tried, n_esc

    def path_llrs_tensor(self, llr, best_words):
        """Decision LLRs of known paths (pscl_path_llrs_device; scl.py:158,166) on the caller's current
        torch stream: llr a contiguous float64 or float32 [B, N] (or [B, E]) tensor on this GPU,
        best_words a contiguous int64 [B, W] tensor of the paths' information bits (decode_tensor's
        best_words).  Returns a [B, K] float64 tensor, bit for bit the decoder's info_llrs of those
        paths.  float64 rows at any N <= 1024; float32 rows natively at N = 128
        (pscl_path_llrs_device_f32), elsewhere widened with llr.double() (see decode_tensor)."""
        import torch

        if self.device == "cpu":
            raise ValueError("the tensor methods need a GPU decoder")
        f32 = self._f32_rows(llr, self._dec.E or self.N)
        B, W = llr.shape[0], self._dec.W
        if (not isinstance(best_words, torch.Tensor) or best_words.dtype != torch.int64 or not best_words.is_contiguous()
                or tuple(best_words.shape) != (B, W)):
            raise ValueError(f"best_words must be a contiguous int64 [B, {W}] tensor")
        if llr.device.type != "cuda" or llr.device.index != self.device or best_words.device != llr.device:
            raise ValueError(f"llr and best_words must be on GPU {self.device}")
        out = torch.empty((B, self.K), dtype=torch.float64, device=llr.device)
        self._dec.set_stream(torch.cuda.current_stream(llr.device).cuda_stream)
        if f32 and self.N == 128:
            self._dec.path_llrs_device_f32(llr.data_ptr(), B, best_words.data_ptr(), out.data_ptr())
            return out
        if f32:
            llr = llr.double()
        self._dec.path_llrs_device(llr.data_ptr(), B, best_words.data_ptr(), out.data_ptr())
        if f32:
            self._dec.join()  # (the widened temporary: see decode_tensor)
        return out

    def label(self, llr: np.ndarray, sent: np.ndarray, max_flips: int = 8) -> dict:
        """Flip labels for beta training (pscl_label_device, or pscl_label_cpu on a device="cpu"
        decoder): llr [B, N] float64, sent [K] or [B, K] 0/1 -> dict(frame, abs_l0, flip, rank,
        counts), one row per frame whose baseline fails the CRC, sorted by frame."""
        return self._dec.label(llr, sent, max_flips)

    def label_tensor(self, llr, sent_words, max_flips: int = 8):
        """label on the caller's current torch stream: llr a contiguous float64 [B, N] (or [B, E])
        tensor on this GPU, sent_words a contiguous int64 [W] (one message for all frames) or [B, W]
        tensor of the sent message words (transmit_tensor's msg).  Returns dict(frame [A] int64,
        abs_l0 [A, K] float32, flip [A] int32, rank [A] int32, counts int64[4]) of tensors, entries
        sorted by frame.  The call waits once on the host, for the entry count."""
        import torch

        if self.device == "cpu":
            raise ValueError("the tensor methods need a GPU decoder")
        dec = self._dec
        if self._f32_rows(llr, dec.E or self.N):
            raise ValueError("label_tensor takes float64 rows")
        B, W, K = llr.shape[0], dec.W, self.K
        if (not isinstance(sent_words, torch.Tensor) or sent_words.dtype != torch.int64 or not sent_words.is_contiguous()
                or tuple(sent_words.shape) not in ((W,), (B, W))):
            raise ValueError(f"sent_words must be a contiguous int64 [{W}] or [B, {W}] tensor")
        if llr.device.type != "cuda" or llr.device.index != self.device or sent_words.device != llr.device:
            raise ValueError(f"llr and sent_words must be on GPU {self.device}")
        stride = 0 if sent_words.dim() == 1 else W
        counts = torch.zeros((_native.PSCL_NLABEL,), dtype=torch.int64, device=llr.device)
        dec.set_stream(torch.cuda.current_stream(llr.device).cuda_stream)
        cap = _native.label_capacity(B, K)
        for _ in range(2):
            frame = torch.empty((cap,), dtype=torch.int64, device=llr.device)
            abs_l0 = torch.empty((cap, K), dtype=torch.float32, device=llr.device)
            flip = torch.empty((cap,), dtype=torch.int32, device=llr.device)
            rank = torch.empty((cap,), dtype=torch.int32, device=llr.device)
            try:
                A = dec.label_device(llr.data_ptr(), B, sent_words.data_ptr(), stride, max_flips, cap,
                                     d_frame=frame.data_ptr(), d_abs_l0=abs_l0.data_ptr(), d_flip=flip.data_ptr(),
                                     d_rank=rank.data_ptr(), d_counts=counts.data_ptr())
                break
            except _native.LabelCapacity as e:
                if cap >= e.entries:
                    raise
                cap = e.entries
        o = torch.argsort(frame[:A], stable=True)
        return {"frame": frame[:A][o], "abs_l0": abs_l0[:A][o], "flip": flip[:A][o], "rank": rank[:A][o], "counts": counts}

    # ---- caller payloads: payload -> CRC -> codeword (-> symbols or AWGN LLR rows) on the device
    def encode(self, payload_bits: np.ndarray, device=None) -> dict:
        """payload_bits [B, k_payload] 0/1 (k_payload = K - CRC degree) -> dict(msg [B, K] int8 =
        attach_crc(payload), code [B, E] int8 = the transmitted bits: the codeword, or with rate
        matching (native.set_rate_match) the interleaved, truncated or repeated codeword).  Host
        arrays in and out; packs, calls pscl_encode_device and unpacks.  On a device="cpu" decoder,
        or with device="cpu" here, the host form pscl_encode_cpu computes the same words."""
        bits = np.asarray(payload_bits)
        if bits.ndim == 1:
            bits = bits[None, :]
        if bits.ndim != 2 or bits.shape[1] != self.k_payload:
            raise ValueError(f"payload_bits must be [B, {self.k_payload}]")
        if np.any((bits != 0) & (bits != 1)):
            raise ValueError("payload_bits entries must be 0 or 1")
        B, E = bits.shape[0], self._dec.E or self.N
        words = _pack_words(bits, self.payload_words)
        if self.device == "cpu" or device == "cpu":
            msg, code = _native.encode_cpu(self.N, self.info_set, self.crc_poly, words, self._dec.E)
        else:
            dec = self._dec
            with _native.DeviceArena(dec) as mem:
                d_pay = mem.alloc(max(words.nbytes, 8))
                d_msg = mem.alloc(max(B * dec.W * 8, 8))
                d_code = mem.alloc(max(B * dec.code_words * 8, 8))
                if B:
                    mem.upload(d_pay, words)
                dec.encode_device(d_pay, B, d_msg=d_msg, d_code=d_code)
                msg = mem.download(d_msg, max(B * dec.W * 8, 8), np.uint64)[:B * dec.W].reshape(B, dec.W)
                code = mem.download(d_code, max(B * dec.code_words * 8, 8), np.uint64)[:B * dec.code_words]
                code = code.reshape(B, dec.code_words)
        return {"msg": _unpack_words(msg, self.K), "code": _unpack_words(code, E)}

    def derate_match_tensor(self, llr):
        """The NR front end alone on the caller's current torch stream, without a host wait
        (pscl_derate_match_device; native.set_rate_match(E) first): llr, a contiguous float64 [B, E]
        tensor of received LLRs on this decoder's GPU -> the [B, N] float64 decoder-internal rows,
        subblock_deinterleave(derate_match_polar(row, N), N) bit for bit.  A plain decoder of the same
        code decodes them to this decoder's results on llr."""
        import torch

        if self.device == "cpu":
            raise ValueError("the tensor methods need a GPU decoder")
        E = self._dec.E
        if not E:
            raise ValueError("the decoder has no rate matching (native.set_rate_match)")
        if (not isinstance(llr, torch.Tensor) or llr.dtype != torch.float64 or not llr.is_contiguous() or llr.dim() != 2
                or llr.shape[1] != E):
            raise ValueError(f"llr must be a contiguous float64 [B, {E}] tensor")
        if llr.device.type != "cuda" or llr.device.index != self.device:
            raise ValueError(f"llr must be on GPU {self.device}")
        B = llr.shape[0]
        out = torch.empty((B, self.N), dtype=torch.float64, device=llr.device)
        self._dec.set_stream(torch.cuda.current_stream(llr.device).cuda_stream)
        self._dec.derate_match_device(llr.data_ptr(), B, out.data_ptr())
        return out

    def _payload_tensor(self, payload_words):
        """Validate payload_words for the tensor methods -- a contiguous int64 [B, payload_words]
        tensor on this decoder's GPU; anything else raises ValueError before any device call."""
        import torch

        if self.device == "cpu":
            raise ValueError("the tensor methods need a GPU decoder (device='cpu' has encode())")
        if (not isinstance(payload_words, torch.Tensor) or payload_words.dtype != torch.int64
                or not payload_words.is_contiguous() or payload_words.dim() != 2
                or payload_words.shape[1] != self.payload_words):
            raise ValueError(f"payload_words must be a contiguous int64 [B, {self.payload_words}] tensor")
        if payload_words.device.type != "cuda" or payload_words.device.index != self.device:
            raise ValueError(f"payload_words must be on GPU {self.device}")
        return payload_words.shape[0]

    def encode_tensor(self, payload_words, symbols=None):
        """Device path of encode on the caller's current torch stream, without a host wait:
        payload_words [B, payload_words] int64 (the uint64 words' bits; bits from k_payload on are
        ignored) -> (msg_words [B, W] int64, code_words [B, ceil(E / 64)] int64), and with symbols =
        torch.float32 or torch.float64 also the BPSK symbols 1 - 2 code [B, E] of that dtype
        (pscl_encode_device).  msg_words is what decode_tensor takes as ref_words."""
        import torch

        if symbols not in (None, torch.float32, torch.float64):
            raise ValueError("symbols must be None, torch.float32 or torch.float64")
        B = self._payload_tensor(payload_words)
        dec, dev = self._dec, payload_words.device
        msg = torch.empty((B, dec.W), dtype=torch.int64, device=dev)
        code = torch.empty((B, dec.code_words), dtype=torch.int64, device=dev)
        sym = None if symbols is None else torch.empty((B, dec.E or self.N), dtype=symbols, device=dev)
        dec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dec.encode_device(payload_words.data_ptr(), B, d_msg=msg.data_ptr(), d_code=code.data_ptr(),
                          d_sym=0 if sym is None else sym.data_ptr(), sym_f32=symbols == torch.float32)
        return (msg, code) if sym is None else (msg, code, sym)

    def transmit_tensor(self, payload_words, ebno_db: float, *, seed: int, stream_id: int = 0, frame0: int = 0,
                        rate: Optional[float] = None, dtype=None):
        """encode_tensor's message sent over BPSK/AWGN at Eb/N0 = ebno_db (pscl_channel_payload_device):
        returns (llr [B, E] of dtype torch.float64 (default) or torch.float32, msg_words [B, W] int64).
        The noise of frame b is pscl_channel_device's for frame counter frame0 + b under (seed,
        stream_id); rate defaults to k_payload / E (run_ber_sweep's convention).  float32 rows are
        what decode_tensor decodes natively where native.f32_available()."""
        import torch

        dtype = torch.float64 if dtype is None else dtype
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        if frame0 < 0:
            raise ValueError("frame0 must be >= 0")
        B = self._payload_tensor(payload_words)
        dec, dev = self._dec, payload_words.device
        E = dec.E or self.N
        rate = self.k_payload / E if rate is None else float(rate)
        if not rate > 0:
            raise ValueError("rate must be positive")
        llr = torch.empty((B, E), dtype=dtype, device=dev)
        msg = torch.empty((B, dec.W), dtype=torch.int64, device=dev)
        dec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dec.channel_payload_device(payload_words.data_ptr(), seed, stream_id, ebno_db, rate, frame0, B,
                                   d_llr=llr.data_ptr(), llr_f32=dtype == torch.float32, d_msg=msg.data_ptr())
        return llr, msg


def _pack_words(bits: np.ndarray, words: int) -> np.ndarray:
    """[B, n] 0/1 -> [B, words] uint64, bit j at word j // 64, bit j % 64."""
    out = np.zeros((bits.shape[0], words * 8), np.uint8)
    packed = np.packbits(bits.astype(np.uint8), axis=1, bitorder="little")
    out[:, :packed.shape[1]] = packed
    return out.view("<u8").astype(np.uint64).reshape(bits.shape[0], words)


def _unpack_words(words: np.ndarray, n: int) -> np.ndarray:
    """The inverse of _pack_words: the first n bits of each row as int8."""
    by = np.ascontiguousarray(words.astype("<u8")).view(np.uint8).reshape(words.shape[0], -1)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :n].astype(np.int8)


__all__ = ["decode_scl", "SCLDecoder"]
