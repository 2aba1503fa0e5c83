"""Inputs of the decision-LLR replay tests (test_replay_long_cpu.py, test_gpu_replay_long.py): the
code shapes, the three kinds of generated rows, and a plain NumPy restatement of the reference's f/g
recursion (polar.py:122-127, 146-164) with the path's bits given.  Each case is computed once per
session and shared read-only."""
import functools

import numpy as np

import adaptive_cases as ac

# (N, K, L, crc): W = 16 words of bits at K = 1000, one word at K = 9
SHAPES = [(256, 128, 8, ac.POLY24), (512, 200, 4, ac.POLY24), (1024, 512, 4, ac.POLY24), (1024, 1000, 2, None),
          (256, 9, 4, None), (2, 1, 1, None), (64, 32, 4, ac.POLY24)]
LONG_SHAPES = [s for s in SHAPES if s[0] >= 256]
KINDS = ["awgn", "quantised", "noiseless"]
# the reference's goldens that record info_llrs (test_cpu_decoder.py's decode sets)
GOLDEN_SETS = ["g4_decode.npz", "g6_forced.npz", "g10_n16.npz", "g10_n32.npz", "g10_n64_nocrc.npz",
               "g10_k88.npz", "g10_m16.npz", "g10_n8.npz", "g10_n4.npz", "g10_n2.npz",
               "g14_n256.npz", "g14_n256_forced.npz", "g14_n512.npz", "g14_n1024.npz"]
LONG_GOLDEN_SETS = ["g14_n256.npz", "g14_n256_forced.npz", "g14_n512.npz", "g14_n1024.npz"]


def shape_id(s):
    return f"N{s[0]}_K{s[1]}_L{s[2]}" + ("" if s[3] else "_nocrc")


@functools.lru_cache(maxsize=None)
def rows(N, K, crc, kind, B, E=0):
    """[B, N] (or [B, E]) rows of one kind: AWGN at 1 dB; integers in [-3, 3] with zeros of both
    signs; a noiseless codeword at +-20."""
    info = ac.info_set(N, K)
    seed = 1000 * N + K + 7 * KINDS.index(kind) + E
    if kind == "awgn":
        out = ac.make_llr(seed, B, info, crc, 1.0, N=N, E=E)
    elif kind == "quantised":
        rng = np.random.default_rng(seed)
        out = rng.integers(-3, 4, size=(B, E or N)).astype(np.float64)
        neg = rng.integers(0, 2, size=out.shape).astype(bool)
        out[(out == 0.0) & neg] = -0.0
    else:
        big = ac.make_llr(seed, B, info, crc, 60.0, N=N, E=E)  # (the noise is far below the symbol)
        out = np.where(big < 0, -20.0, 20.0)
    out.setflags(write=False)
    return out


def flat_golden(g):
    """(key, M, llr [B, N], force or None, npaths [B], cands [B, M, K], info_llrs [B, M, K]) per key."""
    for key in g["keys"]:
        key = str(key)
        M = int(key.split("_")[0][1:])
        force = g[key + "_force"] if key + "_force" in g.files else None
        yield key, M, g[key + "_llr"], force, g[key + "_npaths"], g[key + "_cands"], g[key + "_info_llrs"]


def golden_paths(g):
    """Every recorded candidate of a golden: (llr rows [P, N], bits [P, K], info_llrs [P, K])."""
    r, b, l = [], [], []
    for key, M, llr, force, npaths, cands, il in flat_golden(g):
        for f in range(llr.shape[0]):
            for p in range(int(npaths[f])):
                r.append(llr[f])
                b.append(cands[f][p])
                l.append(np.asarray(il[f][p], np.float64))
    return np.stack(r), np.stack(b).astype(np.int8), np.stack(l)


def bits_eq(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                                  np.ascontiguousarray(b, dtype=np.float64).view(np.uint64), err_msg=msg)


def numpy_replay(llr, info, bits):
    """The leaf LLRs at the information phases of the path with information bits `bits`, by the
    reference's recursion: f = sign(a) sign(b) min(|a|, |b|), g = b + (1 - 2 c) a."""
    N = llr.size
    u = np.zeros(N, np.int8)
    u[np.asarray(info)] = bits
    leaf = np.zeros(N)

    def rec(seg, start):
        w = seg.size
        if w == 1:
            leaf[start] = seg[0]
            return u[start:start + 1].copy()
        a, b = seg[: w // 2], seg[w // 2:]
        left = rec(np.sign(a) * np.sign(b) * np.minimum(np.abs(a), np.abs(b)), start)
        right = rec(b + (1 - 2 * left.astype(np.float64)) * a, start + w // 2)
        return np.concatenate([left ^ right, right])

    rec(np.asarray(llr, np.float64), 0)
    return leaf[np.asarray(info)]
