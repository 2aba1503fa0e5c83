"""Inputs and expected values of the staged de-rate-matching tests (test_rm_staged_cpu.py,
test_gpu_rm_staged.py): pscl_derate_match_device and the staged mode of pscl_set_rate_match_staged.
Expected values come from the oracle alone -- adaptive_cases.compose(rows, info, L, crc, N=N, E=E),
adaptive_cases.internal_rows, staged_cases.sc_expected -- on rows from
adaptive_cases.make_llr(1000 + N + E, B, info, crc, dB, N=N, E=E).  Each case is computed once per
session and shared read-only."""
import functools
from collections import namedtuple

import numpy as np

import adaptive_cases as ac
import staged_cases as sg

POLY8 = sg.POLY8
Case = namedtuple("Case", "name N K pw E L crc dB B escalated list_fail")

# The smallest batches that still leave a ragged last wavefront and more than one workgroup; every one
# has 0 < escalated < B, so both stages run in each.  escalated: frames whose SC result fails the CRC;
# list_fail: frames whose list result fails it (both pinned against the oracle by the CPU test).
# pw: the polarization-weight set (with construct_info_set at N >= 512 every frame fails).
CASES = (
    Case("n32_E45", 32, 28, False, 45, 4, POLY8, 5.0, 259, 106, 30),
    Case("n32_E29", 32, 28, False, 29, 4, POLY8, 8.0, 259, 189, 1),
    Case("n64_E57", 64, 40, False, 57, 4, ac.POLY24, 8.0, 259, 114, 15),
    Case("n64_E200", 64, 40, False, 200, 8, ac.POLY24, 5.0, 259, 215, 112),
    Case("n128_E100", 128, 64, False, 100, 4, ac.POLY24, 5.0, 300, 231, 126),
    Case("n128_E389", 128, 64, False, 389, 8, ac.POLY24, 6.0, 515, 294, 63),
    Case("n128k40_E201", 128, 40, False, 201, 4, ac.POLY16, 5.0, 515, 396, 232),
    Case("n256_E300", 256, 128, True, 300, 8, ac.POLY24, 2.5, 259, 109, 14),
    Case("n256_E249", 256, 128, True, 249, 16, ac.POLY24, 2.5, 131, 41, 4),
    Case("n512_E600", 512, 256, True, 600, 8, ac.POLY24, 2.5, 131, 35, 2),
    Case("n512_E1541", 512, 256, True, 1541, 4, ac.POLY24, 2.5, 131, 12, 1),
    Case("n512_E512", 512, 256, True, 512, 8, ac.POLY24, 2.5, 131, 14, 1),
    Case("n1024_E1100", 1024, 512, True, 1100, 8, ac.POLY24, 2.0, 67, 13, 1),
    Case("n1024_E1017", 1024, 512, True, 1017, 32, ac.POLY24, 2.0, 35, 9, 0),
    Case("n1024_E2048", 1024, 512, True, 2048, 16, ac.POLY24, 2.0, 35, 4, 0),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(BY_NAME)

# the (N, E) pairs of the index-map model and of the pass-alone test: the table's, then
# E in {N - 1, N, N + 1, 2 N, 3 N + 5} at N = 32 and 1024, then two puncture-only pairs below N = 32
EDGE_PAIRS = tuple((N, E) for N in (32, 1024) for E in (N - 1, N, N + 1, 2 * N, 3 * N + 5)) + ((8, 6), (16, 12))
PAIRS = tuple(dict.fromkeys(tuple((c.N, c.E) for c in CASES) + EDGE_PAIRS))


def info_of(c):
    return sg.pw_info_set(c.N, c.K) if c.pw else ac.info_set(c.N, c.K)


@functools.lru_cache(maxsize=None)
def rows_of(name):
    c = BY_NAME[name]
    rows = ac.make_llr(1000 + c.N + c.E, c.B, info_of(c), c.crc, c.dB, N=c.N, E=c.E)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def expected(name):
    """The composition (SC where it passes, else the list result) on the case's rows."""
    c = BY_NAME[name]
    return ac.compose(rows_of(name), info_of(c), c.L, c.crc, N=c.N, E=c.E)


def list_expected(name):
    """The plain list decode's outputs on every frame, in assert_equals' keys."""
    e = expected(name)
    return {"best_bits": e["list_bits"], "crc_pass": e["list_ok"], "best_idx": e["list_idx"]}


# ---- a NumPy model of the pass's index map (derate.hip)

def model_copies(N, E):
    """De-rate-matched position k -> (the received indices summed, in order; the remainder's index or
    -1; the count).  E <= N: one copy where k < E, else none (the pad)."""
    k = np.arange(N)
    if E <= N:
        return [([int(i)] if i < E else [], -1, 1) for i in k]
    reps, rem = divmod(E, N)
    return [([int(i + r * N) for r in range(reps)], int(reps * N + i) if i < rem else -1, reps + (1 if i < rem else 0))
            for i in k]


def model_src(N):
    """Output position i -> the de-rate-matched position it holds: the transpose of an (N / 32) x 32
    matrix, i = c (N / 32) + r <- k = 32 r + c; the identity below N = 32."""
    i = np.arange(N)
    if N < 32:
        return i
    nb = N // 32
    return (i % nb) * 32 + i // nb


def model_pass(rows, N):
    """The pass on host rows [B, E], with its arithmetic: repeats summed in index order, 0.0 + s, the
    remainder copy, one division by the count; E <= N pads with -1.0."""
    rows = np.asarray(rows, np.float64)
    E = rows.shape[1]
    d = np.empty((rows.shape[0], N))
    for k, (idx, rem, cnt) in enumerate(model_copies(N, E)):
        if not idx:
            d[:, k] = -1.0
            continue
        s = rows[:, idx[0]].copy()
        for j in idx[1:]:
            s = s + rows[:, j]
        if E > N:
            s = 0.0 + s
            if rem >= 0:
                s = s + rows[:, rem]
            s = s / float(cnt)
        d[:, k] = s
    return d[:, model_src(N)]


def special_rows(N, E, seed):
    """Five rows each of: integers, all -0.0, values whose pair sums cancel to +-0, +-1e-310
    subnormals, +-1e300 (with signs that do not overflow a sum: each position's copies share one)."""
    rng = np.random.default_rng(seed)
    ints = np.round(rng.normal(1.5, 3.0, size=(5, E)))
    negz = np.full((5, E), -0.0)
    k = np.arange(E) % N
    sign_r = np.where((np.arange(E) // N) % 2 == 0, 1.0, -1.0)  # copy r of a position: + - + - ...
    cancel = np.round(rng.normal(0.0, 4.0, size=(5, N)))[:, k] * sign_r
    sgn = np.where(rng.integers(0, 2, size=(5, N)) == 1, -1.0, 1.0)[:, k]
    sub = sgn * 1e-310
    big = sgn * 1e300 / 8.0 * rng.integers(1, 8, size=(5, E))  # (sums of up to 5 copies stay finite)
    return np.concatenate([ints, negz, cancel, sub, big])


@functools.lru_cache(maxsize=None)
def pass_rows(N, E):
    """The pass-alone batch of one (N, E): Gaussian rows plus special_rows, B = 131 (67 at N = 1024)."""
    B = 67 if N == 1024 else 131
    rng = np.random.default_rng(7000 + N + E)
    rows = np.concatenate([rng.normal(0.5, 4.0, size=(B - 25, E)), special_rows(N, E, 7100 + N + E)])
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def tie_rows(E, seed):
    """40 integer rows, np.round(normal(1.5, 3.0)): exact final-metric ties, which a screening decode
    must defer to the exact re-decode."""
    rows = np.round(np.random.default_rng(seed).normal(1.5, 3.0, size=(40, E)))
    rows.setflags(write=False)
    return rows
