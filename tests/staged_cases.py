"""Inputs and expected values of the staged-decoding tests (test_sc_lane_cpu.py,
test_gpu_sc_lane.py): pscl_sc_device and pscl_escalate_device at N = 32 .. 1024.  Expected values
come from the oracle alone, through adaptive_cases.compose(..., N=N).  Each case is computed once
per session and shared read-only."""
import functools

import numpy as np

import adaptive_cases as ac
import oracle

POLY8 = "0x107"
LENGTHS = (32, 64, 256, 512, 1024)


def crc_for(N):
    """CRC-8 at N = 32 (the block sets hold 16 bits), CRC-24 elsewhere."""
    return POLY8 if N == 32 else ac.POLY24


def pw_weights(N):
    """Polarization weight of every position: the sum of 2^(j / 4) over the set bits j of i."""
    i = np.arange(N)
    return sum(((i >> j) & 1) * 2.0 ** (j / 4) for j in range(N.bit_length() - 1))


@functools.lru_cache(maxsize=None)
def pw_info_set(N, K):
    """The K positions of largest polarization weight, ascending (ties by the larger index)."""
    order = np.argsort(pw_weights(N), kind="stable")
    return np.sort(order[N - K:]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def block_family(N):
    """The 2 log2 N sets {i : ((i >> j) & 1) == v} (K = N / 2 each), as (name, info): together they
    enter every SC node of the length-N tree in each of its three states."""
    i = np.arange(N)
    return tuple((f"bit{j}={v}", i[((i >> j) & 1) == v].astype(np.int32))
                 for j in range(N.bit_length() - 1) for v in (0, 1))


# (name, N, information set, CRC, Eb/N0, B) of the mixed batches
def mixed_specs():
    return {
        "pw256": (256, pw_info_set(256, 128), ac.POLY24, 2.5, 259),
        "pw512": (512, pw_info_set(512, 256), ac.POLY24, 2.5, 259),
        "pw1024": (1024, pw_info_set(1024, 512), ac.POLY24, 2.0, 131),
        "c64": (64, ac.info_set(64, 40), ac.POLY24, 5.0, 259),
        "c32": (32, ac.info_set(32, 28), POLY8, 5.0, 259),
    }


@functools.lru_cache(maxsize=None)
def mixed_rows(name):
    N, info, crc, ebno, B = mixed_specs()[name]
    rows = ac.make_llr(1000 + N, B, info, crc, ebno, N=N)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def mixed_case(name, L=8):
    N, info, crc, _, _ = mixed_specs()[name]
    return {"N": N, "info": info, "crc": crc, "rows": mixed_rows(name),
            "exp": ac.compose(mixed_rows(name), info, L, crc, N=N)}


@functools.lru_cache(maxsize=None)
def family_case(N, name, L=4):
    """One block set: Gaussian rows at 5 dB, the composition on them, and the rows shifted so that
    stage 1 decides every frame, with their targets.  B = 259 (N <= 64) or 67 (N >= 256): more than
    one workgroup and a ragged group at every N."""
    info = dict(block_family(N))[name]
    crc = crc_for(N)
    B = 259 if N <= 64 else 67
    raw = ac.make_llr(500 + N + len(name), B, info, crc, 5.0, N=N)
    shifted, t = ac.shift_to_valid(raw, info, crc, seed=900 + N, N=N)
    for a in (raw, shifted, t):
        a.setflags(write=False)
    return {"info": info, "crc": crc, "raw": raw, "exp": ac.compose(raw, info, L, crc, N=N), "shifted": shifted, "t": t}


def sc_expected(rows, info, crc):
    """The oracle's SC result of every row: (bits [B, K] int8, CRC pass [B] bool)."""
    sc = np.stack([oracle.sc_decode(r, info) for r in rows])
    return sc, np.array([oracle.check_crc(b, crc) if crc else True for b in sc], bool)


def words(bits):
    B, K = bits.shape
    w = np.zeros((B, (K + 63) // 64), np.uint64)
    for j in range(K):
        w[:, j >> 6] |= bits[:, j].astype(np.uint64) << np.uint64(j & 63)
    return w


def host_counts(bits, ok, ref, kp, ncount, escalated=0):
    """FER/BER counters of outputs (bits, ok) against ref, in the PSCL_CNT_* layout."""
    d = bits != ref
    want = np.zeros(ncount, np.int64)
    want[0] = len(bits)
    want[1] = np.count_nonzero(~ok)
    want[2] = d.sum()
    want[3] = np.count_nonzero(d[:, :kp].any(axis=1))
    want[4] = d[:, :kp].sum()
    want[6] = escalated
    return want
