"""Inputs and expected values of the float32-row tests (test_gpu_f32.py).  Every case builds its rows
as float32, widens them on the host with astype(np.float64) -- which is exact -- and takes its
expected values from the oracle alone on the widened rows (adaptive_cases.compose: sc_decode +
check_crc, decode_batch, their composition).  Each case is computed once per session and shared
read-only."""
import functools

import numpy as np

import adaptive_cases as ac
import oracle

INFO64 = lambda: ac.info_set(128, 64)  # noqa: E731
INFO88 = lambda: ac.info_set(128, 88)  # noqa: E731


def f32(rows):
    out = np.ascontiguousarray(rows, dtype=np.float32)
    out.setflags(write=False)
    return out


def widen(rows32):
    assert rows32.dtype == np.float32
    return rows32.astype(np.float64)


@functools.lru_cache(maxsize=None)
def mixed_rows():
    """The 4,099-frame mixed batch of adaptive_cases ((128,64)+CRC-24, 5 dB), rounded to float32."""
    return f32(ac.mixed_rows())


@functools.lru_cache(maxsize=None)
def mixed_expected(L):
    return ac.compose(widen(mixed_rows()), INFO64(), L, ac.POLY24)


@functools.lru_cache(maxsize=None)
def allpass_case():
    rows = f32(ac.allpass_case()[0])
    return rows, ac.compose(widen(rows), INFO64(), 8, ac.POLY24)


@functools.lru_cache(maxsize=None)
def allfail_case():
    rows = f32(ac.allfail_case()[0])
    return rows, ac.compose(widen(rows), INFO64(), 8, ac.POLY24)


@functools.lru_cache(maxsize=None)
def nr_rows(E, B=263):
    """(128,88)+CRC-24 through E received values, 5 dB, float32.  B = 256 + 7: more than one SC
    workgroup (32 frames rate matched), ragged wavefronts in the SC (16 frames) and list (8, 16) kernels."""
    return f32(ac.make_llr(40 + E, B, INFO88(), ac.POLY24, 5.0, E=E))


@functools.lru_cache(maxsize=None)
def nr_expected(E, L):
    return ac.compose(widen(nr_rows(E)), INFO88(), L, ac.POLY24, E=E)


@functools.lru_cache(maxsize=None)
def family_rows(name):
    """One block information set: its Gaussian rows and its codeword-shifted rows (adaptive_cases.
    family_case), rounded to float32, with the oracle's SC result on each."""
    case = ac.family_case(name)
    out = {"info": case["info"]}
    for k in ("raw", "shifted"):
        rows = f32(case[k])
        sc = np.stack([oracle.sc_decode(r, case["info"]) for r in widen(rows)])
        ok = np.array([oracle.check_crc(b, ac.POLY24) for b in sc], bool)
        out[k] = (rows, sc, ok)
    return out


@functools.lru_cache(maxsize=None)
def tie_case():
    """Rows the screening pass must defer (ties: +-1 and small integers, exactly representable in
    float32), each followed by two rows that pass the SC stage: a deferred frame's position in any
    list differs from its row number.  (rows, {L: composition})."""
    rng = np.random.default_rng(4242)
    a = rng.choice([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], size=(96, 128))
    b = rng.choice([-1.0, 1.0], size=(64, 128))
    ties = np.concatenate([a, b])
    good = allpass_case()[0]
    rows = np.empty((3 * len(ties), 128), np.float32)
    rows[0::3] = ties
    rows[1::3] = good[:len(ties)]
    rows[2::3] = good[len(ties):2 * len(ties)]
    rows.setflags(write=False)
    return rows, {L: ac.compose(widen(rows), INFO64(), L, ac.POLY24) for L in (8, 4)}


TINY = np.float32(1e-40)  # a float32 subnormal (the smallest normal is 1.18e-38)


@functools.lru_cache(maxsize=None)
def corner_rows():
    """Exact-arithmetic corners as float32 rows of the (128,64) code: all zero, all -0.0, noiseless
    +-c codewords, small integers, subnormals of both signs (alone, and mixed with normal values),
    and values near 3e38 (float32's largest is 3.4e38)."""
    info = INFO64()
    rng = np.random.default_rng(4301)
    N, K = 128, len(info)

    def codeword_signs():
        u = np.zeros(N, np.int8)
        u[info] = rng.integers(0, 2, size=K)
        return 1.0 - 2.0 * oracle.polar_transform(u)

    cw = np.stack([codeword_signs() * (1.0, 2.5, 1e30)[b % 3] for b in range(48)])
    small = rng.choice([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], size=(64, N))
    # subnormal magnitudes 1 .. 9 units of 1e-40 with a codeword's signs: flushed to zero, every
    # `llr < 0` decision of the row becomes "not negative"
    sub = np.stack([codeword_signs() * (rng.integers(1, 10, size=N) * 1e-40) for _ in range(32)])
    # subnormal and normal magnitudes mixed, position by position
    mag = np.where(rng.random((32, N)) < 0.5, rng.integers(1, 10, size=(32, N)) * 1e-40, rng.uniform(0.5, 4.0, size=(32, N)))
    mix = np.stack([codeword_signs() for _ in range(32)]) * mag
    # noisy rows next to signed subnormals: positions whose value is +-1e-40 in an AWGN row
    noisy = np.array(mixed_rows()[:32], dtype=np.float64)
    noisy[rng.random(noisy.shape) < 0.25] = 1e-40
    noisy[rng.random(noisy.shape) < 0.25] = -1e-40
    big = np.stack([codeword_signs() * rng.uniform(2.0e38, 3.3e38, size=N) for _ in range(16)])
    rows = np.concatenate([np.zeros((3, N)), -np.zeros((2, N)), cw, small, sub, mix, noisy, big]).astype(np.float32)
    s0 = 5 + 48 + 64
    part = rows[s0:s0 + 32]
    assert np.all(part != 0) and np.all(np.abs(part) < np.float32(1.1e-38))  # (subnormal, not rounded to zero)
    assert np.isfinite(rows).all() and np.abs(rows).max() > 3e38
    rows.setflags(write=False)
    return rows, s0
