"""Inputs and expected values of the flip-label tests (test_label_cpu.py, test_gpu_label.py).

Rows come from adaptive_cases.make_llr(..., with_msg=True): every frame has its own sent message.
Expected values come from the oracle alone, composing the contract of pscl_label_device
(include/polar_scl.h; make_dataset.py:52-91 of the reference per frame): oracle.decode_scl for the
baseline, its best path's info_llrs narrowed to float32, np.argsort(kind="stable") of the absolute
values -- stable is "equal values resolve to the lower index", and without equal values any argsort
agrees -- then oracle.decode_scl with the forced bits of flip.py:30-34 on the BASELINE bits, rank by
rank, until a result passes the CRC and equals the frame's sent message.  Each case is computed once
per session and shared read-only.
"""
import functools
from collections import namedtuple

import numpy as np

import oracle

import adaptive_cases as ac

POLY24 = ac.POLY24
Case = namedtuple("Case", "N K crc L ebno B seed E asu")

# name -> code, list size, Eb/N0, frames, seed, rate-matched length, (A entries, S labelled, U unrepaired)
CASES = {
    "n16k6": Case(16, 6, "0x3", 2, -2.0, 512, 1, 0, (39, 22, 17)),
    "n32k14": Case(32, 14, "0x61", 4, 1.0, 256, 2, 0, (25, 15, 10)),
    "n128k40": Case(128, 40, ac.POLY16, 8, 1.5, 192, 3, 0, (121, 34, 87)),
    "n128L4": Case(128, 64, POLY24, 4, 2.5, 128, 6, 0, (80, 33, 47)),
    "nr88": Case(128, 88, POLY24, 8, 2.5, 128, 5, 256, (105, 12, 93)),
    "n256": Case(256, 128, POLY24, 8, 2.5, 128, 4, 0, (102, 13, 89)),
    "n1024": Case(1024, 512, POLY24, 4, 1.75, 24, 7, 0, (24, 0, 24)),
}
NAMES = tuple(CASES)
MAX_FLIPS = 8


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def force_prefix_flip(bits, idx):
    """flip.py:30-34: bits[:idx] forced, bit idx flipped, the rest free (-1)."""
    f = np.full(bits.size, -1, np.int8)
    f[:idx] = bits[:idx]
    f[idx] = 1 - bits[idx]
    return f


def compose(x, info, L, crc, sent, max_flips=MAX_FLIPS):
    """The contract on decoder-internal rows x [B, N]; sent [K] or [B, K].  Entries in frame order:
    frame, abs_l0, flip, rank, counts (entries, labelled, unrepaired, decodes), plus what the cases
    assert about themselves: wrong_pass (decodes that pass the CRC with another message),
    wrong_entries (entries with such a decode), tie8 (entries with equal values among the first
    max_flips ranks) and tie9 (among the max_flips + 1 smallest)."""
    info = np.asarray(info, np.int32)
    K = info.size
    T = min(max_flips, K)
    sent = np.asarray(sent, np.int8)
    frames, rows, flips, ranks = [], [], [], []
    decodes = wrong_pass = wrong_entries = tie8 = tie9 = 0
    for b in range(x.shape[0]):
        n, c, m, il, best = oracle.decode_scl(x[b], info, L, crc)
        base = c[best].astype(np.int8)
        if oracle.check_crc(base, crc):
            continue
        a = np.abs(il[best].astype(np.float32))
        order = np.argsort(a, kind="stable")
        s = np.sort(a)
        tie8 += bool(np.any(s[1:T] == s[:T - 1]))
        tie9 += bool(np.any(s[1:T + 1] == s[:min(T, K - 1)]))
        want = sent if sent.ndim == 1 else sent[b]
        lab = rk = -1
        wrong = 0
        for t in range(T):
            idx = int(order[t])
            n2, c2, m2, il2, b2 = oracle.decode_scl(x[b], info, L, crc, force_prefix_flip(base, idx))
            decodes += 1
            if oracle.check_crc(c2[b2], crc):
                if np.array_equal(c2[b2], want):
                    lab, rk = idx, t
                    break
                wrong += 1
        wrong_pass += wrong
        wrong_entries += bool(wrong)
        frames.append(b)
        rows.append(a)
        flips.append(lab)
        ranks.append(rk)
    A = len(frames)
    flip = np.array(flips, np.int32).reshape(A)
    out = {
        "frame": np.array(frames, np.int64).reshape(A),
        "abs_l0": np.array(rows, np.float32).reshape(A, K),
        "flip": flip,
        "rank": np.array(ranks, np.int32).reshape(A),
        "counts": np.array([A, np.count_nonzero(flip >= 0), np.count_nonzero(flip < 0), decodes], np.int64),
        "wrong_pass": wrong_pass, "wrong_entries": wrong_entries, "tie8": tie8, "tie9": tie9,
    }
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def info_of(name):
    c = CASES[name]
    return ac.info_set(c.N, c.K)


@functools.lru_cache(maxsize=None)
def rows_of(name):
    """(rows [B, E or N], msg [B, K]) as the decoder's caller hands them over."""
    c = CASES[name]
    rows, msg = ac.make_llr(c.seed, c.B, info_of(name), c.crc, c.ebno, N=c.N, E=c.E, with_msg=True)
    return _frozen(rows), _frozen(msg)


def internal(name):
    """The decoder-internal rows (rate matching undone): the oracle's and the host decoder's input."""
    c = CASES[name]
    return ac.internal_rows(rows_of(name)[0], c.N, c.E)


@functools.lru_cache(maxsize=None)
def expected(name):
    c = CASES[name]
    return compose(internal(name), info_of(name), c.L, c.crc, rows_of(name)[1])


@functools.lru_cache(maxsize=None)
def tie_case():
    """Rows with equal |L0| values: the first 64 failing frames of n128L4 with their LLRs rounded to
    integers (near_tie_cases.base_rows' rounding, np.round(rows / 4)); every frame keeps its message.
    (rows, msg, expected)."""
    rows, msg = rows_of("n128L4")
    fr = expected("n128L4")["frame"][:64]
    r, m = _frozen(np.round(rows[fr] / 4.0)), _frozen(msg[fr])
    c = CASES["n128L4"]
    return r, m, compose(r, info_of("n128L4"), c.L, c.crc, m)


@functools.lru_cache(maxsize=None)
def g12_case(name):
    """The rows of a g12 golden dataset run (tests/golden/g12_dataset.npz; make_dataset's replay
    mode: one all-zero-payload message for every frame, the reference's NumPy noise stream):
    (rows, sent [K], M, expected)."""
    from conftest import GOLDEN
    from polar_code_amd import config
    from polar_code_amd.polar.crc import attach_crc
    from polar_code_amd.polar.polar import encode
    from polar_code_amd.train import make_dataset as md

    g = np.load(GOLDEN / "g12_dataset.npz")
    args = md.build_argparser().parse_args(str(g[name + "_argv"]).split() + ["--out", "unused"])
    cfg = config.get_config()
    sent = attach_crc(np.zeros(cfg.K - cfg.crc_bits, dtype=np.int8), cfg.crc_poly)
    nv = 1.0 / (2.0 * (cfg.K / cfg.N) * 10 ** (args.snr_db / 10.0))
    noise = np.random.default_rng(args.seed).normal(0.0, np.sqrt(nv), size=(args.frames, cfg.N))
    rows = _frozen(2.0 * ((1.0 - 2.0 * encode(sent))[None, :] + noise) / nv)
    sent = _frozen(np.asarray(sent, np.int8))
    return rows, sent, args.M, compose(rows, ac.info_set(cfg.N, cfg.K), args.M, cfg.crc_poly, sent)


@functools.lru_cache(maxsize=None)
def allpass_case():
    """(128,64) + CRC-24 at 5 dB, 64 frames, L = 8, seed 13: every baseline passes (asserted on the oracle)."""
    info = ac.info_set(128, 64)
    rows, msg = ac.make_llr(13, 64, info, POLY24, 5.0, with_msg=True)
    return _frozen(rows), _frozen(msg), compose(rows, info, 8, POLY24, msg)


def subset(exp, n, max_flips=MAX_FLIPS):
    """The expected values of the first n frames of a case (frames are independent): its entries
    below frame n, and their counts -- an entry ran rank + 1 decodes, or every round without a label."""
    keep = exp["frame"] < n
    K = exp["abs_l0"].shape[1]
    rank = exp["rank"][keep]
    decodes = int(np.where(rank >= 0, rank + 1, min(max_flips, K)).sum())
    flip = exp["flip"][keep]
    return {"frame": exp["frame"][keep], "abs_l0": exp["abs_l0"][keep], "flip": flip, "rank": rank,
            "counts": np.array([flip.size, np.count_nonzero(flip >= 0), np.count_nonzero(flip < 0), decodes], np.int64)}


def assert_equals(out, exp, tag):
    """Every output of a label call (entries sorted by frame) against the expected values: frames,
    abs_l0 bit for bit, flips, ranks and all four counts."""
    np.testing.assert_array_equal(np.asarray(out["frame"]), exp["frame"], err_msg=f"{tag}: frame")
    got = np.ascontiguousarray(np.asarray(out["abs_l0"], dtype=np.float32))
    assert got.shape == exp["abs_l0"].shape, f"{tag}: abs_l0 shape {got.shape}"
    np.testing.assert_array_equal(got.view(np.uint32), exp["abs_l0"].view(np.uint32), err_msg=f"{tag}: abs_l0 bits")
    np.testing.assert_array_equal(np.asarray(out["flip"]), exp["flip"], err_msg=f"{tag}: flip")
    np.testing.assert_array_equal(np.asarray(out["rank"]), exp["rank"], err_msg=f"{tag}: rank")
    np.testing.assert_array_equal(np.asarray(out["counts"]), exp["counts"], err_msg=f"{tag}: counts")
