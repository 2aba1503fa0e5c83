"""Inputs and expected values of the float32 DL-SCL tests (test_f32_dl_cpu.py, test_gpu_f32_dl.py): the
float32 rows of f32_cases, widened on the host (exact), through the oracle composition of
adaptive_dl_cases.compose_dl -- SC, the list decoder, DL-SCL flips -- and, for the plain chain,
oracle.dl_batch with the per-frame tried lists of oracle.decode_with_retries.  Expected values come
from the oracle alone on the widened rows.  Each case is computed once per session and shared
read-only."""
import functools

import numpy as np

import adaptive_cases as ac
import adaptive_dl_cases as dc
import f32_cases as fc
import oracle

RETRIES = 8


def _beta(L, with_beta):
    return dc.golden_beta(L) if with_beta else None


@functools.lru_cache(maxsize=None)
def mixed_case(L, with_beta=False, retries=RETRIES):
    """f32_cases.mixed_rows() (4,099 frames, 1,040 escalated) at list size 8 or 4."""
    return dc.compose_dl(fc.widen(fc.mixed_rows()), fc.INFO64(), L, ac.POLY24, retries, _beta(L, with_beta),
                         base=fc.mixed_expected(L))


@functools.lru_cache(maxsize=None)
def tie_case(L, with_beta=False):
    """f32_cases.tie_case(): 160 rows of +-1 and small integers -- |L0| ties everywhere, every list
    decode fails and every retry chain runs all 8 flips -- each followed by two rows SC passes."""
    rows, base = fc.tie_case()
    return rows, dc.compose_dl(fc.widen(rows), fc.INFO64(), L, ac.POLY24, RETRIES, _beta(L, with_beta), base=base[L])


@functools.lru_cache(maxsize=None)
def corner_case():
    """f32_cases.corner_rows() at L = 8: +-0, subnormals of both signs, values near 3e38."""
    rows, _ = fc.corner_rows()
    return rows, dc.compose_dl(fc.widen(rows), fc.INFO64(), 8, ac.POLY24, RETRIES)


@functools.lru_cache(maxsize=None)
def nr_case(E):
    """f32_cases.nr_rows(E): (128,88)+CRC-24 through E received values, L = 8.  E = 201: rows of an odd
    length start on 4-byte boundaries only."""
    rows = fc.nr_rows(E)
    return rows, dc.compose_dl(fc.widen(rows), fc.INFO88(), 8, ac.POLY24, RETRIES, E=E, base=fc.nr_expected(E, 8))


@functools.lru_cache(maxsize=None)
def allfail_case():
    rows, base = fc.allfail_case()
    return rows, dc.compose_dl(fc.widen(rows), fc.INFO64(), 8, ac.POLY24, RETRIES, base=base)


@functools.lru_cache(maxsize=None)
def allpass_case():
    rows, base = fc.allpass_case()
    return rows, dc.compose_dl(fc.widen(rows), fc.INFO64(), 8, ac.POLY24, RETRIES, base=base)


PLAIN_B = 1027


@functools.lru_cache(maxsize=None)
def plain_case(L):
    """pscl_dlscl_device's contract on the first 1,027 mixed rows, with beta_M<L>: the baseline list
    decode (base_*), and decode_with_retries' final bits, success, attempts, tried lists and the final
    attempt's best index."""
    rows = np.ascontiguousarray(fc.mixed_rows()[:PLAIN_B])
    rows.setflags(write=False)
    x, info, beta, base = fc.widen(rows), fc.INFO64(), dc.golden_beta(L), fc.mixed_expected(L)
    bits, succ, att = oracle.dl_batch(x, info, L, RETRIES, crc=ac.POLY24, beta=beta)
    out = {"base_bits": base["list_bits"][:PLAIN_B], "base_ok": np.asarray(base["list_ok"][:PLAIN_B], bool),
           "best_bits": bits, "crc_pass": succ.astype(bool), "attempts": att.astype(np.int32),
           "best_idx": base["list_idx"][:PLAIN_B].copy(), "tried": np.full((PLAIN_B, RETRIES), -1, np.int32)}
    for f in np.flatnonzero(~out["base_ok"]):
        r = oracle.decode_with_retries(x[f], info, L, RETRIES, crc=ac.POLY24, beta=beta)
        assert np.array_equal(r["bits"], bits[f]) and r["success"] == succ[f] and r["attempts"] == att[f] == 1 + len(r["tried"])
        out["tried"][f, :len(r["tried"])] = r["tried"]
        out["best_idx"][f], last = dc._final_index(x[f], info, L, ac.POLY24, out["base_bits"][f], r["tried"])
        assert np.array_equal(last, bits[f])
    assert np.array_equal(bits[out["base_ok"]], out["base_bits"][out["base_ok"]]) and np.all(att[out["base_ok"]] == 1)
    for v in out.values():
        v.setflags(write=False)
    return rows, out


PLAIN_KEYS = ("best_bits", "crc_pass", "best_idx", "attempts", "tried")


@functools.lru_cache(maxsize=None)
def crc16_case():
    """adaptive_dl_cases.crc16_case's rows ((128,40)+CRC-16, 3 dB, 1,027 frames, L = 4) rounded to
    float32: a handle without native float32 kernels."""
    rows64, info, _ = dc.crc16_case()
    rows = fc.f32(rows64)
    return rows, info, dc.compose_dl(fc.widen(rows), info, 4, ac.POLY16, RETRIES)


def counts(exp):
    """(rows, escalated, entries, recovered) of a compose_dl result."""
    return len(exp["stage"]), exp["n_escalated"], exp["n_entries"], exp["n_recovered"]
