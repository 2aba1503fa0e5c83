"""Inputs and expected values of the three-stage decoding tests (test_adaptive_dl_cpu.py,
test_gpu_adaptive_dl.py): SC, the list decoder where SC fails the CRC, DL-SCL flips where the list
decoder fails it too.  Expected values come from the oracle alone: adaptive_cases.compose for
stages 1 and 2, oracle.dl_batch for the final bits / success / attempts of the frames that enter a
retry chain, oracle.decode_with_retries for their tried lists, and oracle.decode_scl with the forced
prefix of the last attempt for the final best index.  Each case is computed once per session and
shared read-only."""
import functools

import numpy as np

import adaptive_cases as ac
import oracle
import staged_cases as sg

from conftest import GOLDEN


def golden_beta(L):
    return np.load(GOLDEN / f"beta_M{L}.npy")


def _final_index(x, info, L, crc, base_bits, tried):
    """Best index of the last attempt: the attempts replayed with oracle.decode_scl (flip.py:30-34,
    88-100: prefix of the reference bits forced, the tried bit flipped).  Returns (index, bits)."""
    ref, idx = base_bits, 0
    for t in tried:
        force = np.full(len(info), -1, np.int8)
        force[:t] = ref[:t]
        force[t] = 1 - ref[t]
        _, cands, _, _, idx = oracle.decode_scl(x, info, L, crc=crc, force=force)
        ref = cands[idx]
    return idx, ref


def compose_dl(rows, info, L, crc, retries, beta=None, N=128, E=0, base=None):
    """The contract of pscl_adaptive_dlscl_device.  base: compose() of the same rows (else computed).
    Keys: best_bits, crc_pass, best_idx, stage (1, 2, 3), attempts, tried [B, max(retries, 0)] (-1
    padded), n_escalated, n_entries, n_recovered, and the earlier stages' sc_bits / sc_ok (SC) and
    base_bits / base_ok (adaptive baseline) for the counter rows."""
    base = base or ac.compose(rows, info, L, crc, N=N, E=E)
    x = ac.internal_rows(rows, N, E)
    B, R = len(rows), max(retries, 0)
    out = {"best_bits": base["best_bits"].copy(), "crc_pass": np.asarray(base["crc_pass"], bool).copy(),
           "best_idx": base["best_idx"].copy(), "stage": base["stage"].copy(), "attempts": np.ones(B, np.int32),
           "tried": np.full((B, R), -1, np.int32), "n_escalated": base["n_escalated"],
           "sc_bits": base["sc_bits"], "sc_ok": base["sc_ok"], "base_bits": base["best_bits"],
           "base_ok": np.asarray(base["crc_pass"], bool)}
    ent = np.flatnonzero(~out["base_ok"]) if R else np.zeros(0, np.int64)
    if len(ent):
        bits, succ, att = oracle.dl_batch(x[ent], info, L, retries, crc=crc, beta=beta)
        for k, f in enumerate(ent):
            r = oracle.decode_with_retries(x[f], info, L, retries, crc=crc, beta=beta)
            assert np.array_equal(r["bits"], bits[k]) and r["success"] == succ[k] and r["attempts"] == att[k] == 1 + len(r["tried"])
            idx, last = _final_index(x[f], info, L, crc, base["best_bits"][f], r["tried"])
            assert np.array_equal(last, bits[k]), f"frame {f}: the replayed attempts end elsewhere"
            out["tried"][f, :len(r["tried"])] = r["tried"]
            out["best_idx"][f] = idx
        out["best_bits"][ent], out["crc_pass"][ent], out["attempts"][ent], out["stage"][ent] = bits, succ, att, 3
    out["n_entries"] = len(ent)
    out["n_recovered"] = int(np.count_nonzero(out["crc_pass"][ent]))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


KEYS = ("best_bits", "crc_pass", "best_idx", "stage", "attempts", "tried")


def assert_equals(out, exp, tag, sl=slice(None), keys=KEYS):
    for k in keys:
        np.testing.assert_array_equal(np.asarray(out[k]), exp[k][sl], err_msg=f"{tag}: {k}")


def prefix(exp, B):
    """The expected values of the first B rows of a case (every frame decodes on its own)."""
    out = {k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in exp.items()}
    out["n_escalated"] = int(np.count_nonzero(out["stage"] >= 2))
    out["n_entries"] = int(np.count_nonzero(out["stage"] == 3))
    out["n_recovered"] = int(np.count_nonzero(out["crc_pass"][out["stage"] == 3]))
    return out


def tiled(exp, reps):
    out = {k: (np.tile(v, (reps, 1) if v.ndim == 2 else reps) if isinstance(v, np.ndarray) else reps * v)
           for k, v in exp.items()}
    return out


def counter_rows(exp, ref, kp, ncount):
    """The three counter rows of pscl_adaptive_dlscl_device against the reference bits ref."""
    want = np.zeros((3, ncount), np.int64)
    want[0] = sg.host_counts(exp["sc_bits"], exp["sc_ok"], ref, kp, ncount)
    want[1] = sg.host_counts(exp["base_bits"], exp["base_ok"], ref, kp, ncount, escalated=exp["n_escalated"])
    want[2] = sg.host_counts(exp["best_bits"], exp["crc_pass"], ref, kp, ncount)
    want[2, 5] = int((exp["attempts"] - 1).sum())  # PSCL_CNT_RETRIES
    return want


@functools.lru_cache(maxsize=None)
def _mixed_base(L):
    return ac.mixed_expected(L) if L in (4, 8) else ac.compose(ac.mixed_rows()[:130], ac.info_set(128, 64), L, ac.POLY24)


@functools.lru_cache(maxsize=None)
def mixed_case(L, with_beta=False, retries=8):
    """adaptive_cases.mixed_rows() (4,099 frames, 1,040 escalated) at list size L; L = 2: the first 130."""
    rows = ac.mixed_rows() if L in (4, 8) else ac.mixed_rows()[:130]
    return compose_dl(rows, ac.info_set(128, 64), L, ac.POLY24, retries, golden_beta(L) if with_beta else None,
                      base=_mixed_base(L))


@functools.lru_cache(maxsize=None)
def allpass_case():
    rows, base = ac.allpass_case()
    return rows, compose_dl(rows, ac.info_set(128, 64), 8, ac.POLY24, 8, base=base)


@functools.lru_cache(maxsize=None)
def allfail_case():
    rows, base = ac.allfail_case()
    return rows, compose_dl(rows, ac.info_set(128, 64), 8, ac.POLY24, 8, base=base)


@functools.lru_cache(maxsize=None)
def nr_case():
    """(128,88)+CRC-24 through E = 256, L = 8."""
    rows, base = ac.nr_case()
    return rows, compose_dl(rows, ac.info_set(128, 88), 8, ac.POLY24, 8, E=256, base=base)


@functools.lru_cache(maxsize=None)
def crc16_case():
    """(128,40)+CRC-16 at 3 dB, seed 4040, B = 1,027, L = 4: the runtime-mask kernels."""
    info = ac.info_set(128, 40)
    rows = ac.make_llr(4040, 1027, info, ac.POLY16, 3.0)
    rows.setflags(write=False)
    return rows, info, compose_dl(rows, info, 4, ac.POLY16, 8)


@functools.lru_cache(maxsize=None)
def n256_case():
    """Constructed (256,128)+CRC-24 at 4 dB, L = 4: SC fails most frames, the dl_retry_long path."""
    info = ac.info_set(256, 128)
    rows = ac.make_llr(4256, 259, info, ac.POLY24, 4.0, N=256)
    rows.setflags(write=False)
    return rows, info, compose_dl(rows, info, 4, ac.POLY24, 8, N=256)


@functools.lru_cache(maxsize=None)
def c32_case():
    """staged_cases' c32 ((32,28)+CRC-8) at L = 4."""
    case = sg.mixed_case("c32", 4)
    return case["rows"], case["info"], case["crc"], compose_dl(case["rows"], case["info"], 4, case["crc"], 8, N=32,
                                                               base=case["exp"])


# Eb/N0 of the N = 1024 batch: the polarization-weight (1024,512) set at list size 4 -- low enough
# that the list decoder still fails some of the frames SC fails (the oracle on the CPU: 48 entries and
# 2 recoveries at 1.0 dB, 19 and 3 at 1.25, 7 and 2 at 1.5, 1 and 1 at 2.0; the tests assert the counts)
N1024_EBNO = 1.25


@functools.lru_cache(maxsize=None)
def n1024_case():
    info = sg.pw_info_set(1024, 512)
    rows = ac.make_llr(5024, 131, info, ac.POLY24, N1024_EBNO, N=1024)
    rows.setflags(write=False)
    return rows, info, compose_dl(rows, info, 4, ac.POLY24, 8, N=1024)
