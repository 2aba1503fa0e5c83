"""Inputs and expected values of the adaptive-decoding tests (test_adaptive_cpu.py,
test_gpu_adaptive.py).  Expected values come from the oracle alone: oracle.sc_decode +
oracle.check_crc per frame, oracle.decode_batch for the list decoder, np.where on the SC pass
mask.  Each case is computed once per session and shared read-only."""
import functools

import numpy as np

import oracle

POLY24 = "0x1864CFB"
POLY16 = "0x11021"


def make_llr(seed, B, info, crc, ebno_db, N=128, E=0, signal=True, with_msg=False):
    """Host TX chain: payload, attach_crc, u[info] = msg, polar transform, BPSK, AWGN, LLR.
    One default_rng(seed) stream, frame by frame: the payload (integers' default dtype), then the
    frame's noise.  rate = K / N (kp / E rate matched, through subblock_interleave +
    rate_match_polar).  Returns
    the rows handed to the decoder ([B, N] or [B, E]).  signal=False: noise-only rows.
    crc=None: the payload is the message.  with_msg: (rows, msg [B, K] int8)."""
    rng = np.random.default_rng(seed)
    K = len(info)
    deg = max(oracle.poly_int(crc).bit_length() - 1, 0)
    kp = K - deg
    n_out = E or N
    rate = kp / E if E else K / N
    nv = 1.0 / (2.0 * rate * 10 ** (ebno_db / 10))
    rows = np.empty((B, n_out))
    msgs = np.empty((B, K), np.int8)
    for b in range(B):
        pay = rng.integers(0, 2, size=kp).astype(np.int8)
        msg = oracle.attach_crc(pay, crc) if deg else pay
        msgs[b] = msg
        u = np.zeros(N, np.int8)
        u[info] = msg
        x = oracle.polar_transform(u)
        if E:
            from polar_code_amd.nr.polar import rate_match_polar, subblock_interleave

            x = rate_match_polar(subblock_interleave(x), E)
        sym = (1.0 - 2.0 * x) if signal else 0.0
        rows[b] = 2.0 * (sym + rng.normal(0.0, np.sqrt(nv), size=n_out)) / nv
    return (rows, msgs) if with_msg else rows


def internal_rows(rows, N, E):
    """The decoder-internal LLRs of rate-matched rows (the oracle's side of NR)."""
    if not E:
        return rows
    from polar_code_amd.nr.polar import derate_match_polar, subblock_deinterleave

    return np.stack([subblock_deinterleave(derate_match_polar(r, N), N) for r in rows])


def compose(rows, info, L, crc, N=128, E=0):
    """The contract: SC where it passes the CRC, else the list decoder's result."""
    x = internal_rows(rows, N, E)
    sc = np.stack([oracle.sc_decode(r, info) for r in x])
    ok = np.array([oracle.check_crc(b, crc) for b in sc], bool)
    lb, lok, lidx = oracle.decode_batch(x, info, L, crc=crc, want_idx=True)
    return {
        "best_bits": np.where(ok[:, None], sc, lb).astype(np.int8),
        "crc_pass": np.where(ok, True, lok),
        "best_idx": np.where(ok, 0, lidx).astype(np.int32),
        "stage": np.where(ok, 1, 2).astype(np.uint8),
        "n_escalated": int(np.count_nonzero(~ok)),
        "sc_bits": sc, "sc_ok": ok, "list_bits": lb, "list_ok": lok, "list_idx": lidx,
    }


def assert_equals(out, exp, tag, sl=slice(None)):
    for k in ("best_bits", "crc_pass", "best_idx", "stage"):
        np.testing.assert_array_equal(np.asarray(out[k]), exp[k][sl], err_msg=f"{tag}: {k}")


@functools.lru_cache(maxsize=None)
def info_set(N, K):
    return oracle.construct_info_set(N, K)


def sc_branch_states(info, N=128):
    """The (M, S, left_has_info, right_has_info) of every SC tree node (M leaves from phase S,
    M = 2 .. N) that holds an information bit: the plain-Python mirror of the SC kernel's mask
    tests.  A node is entered only if it holds information, so each of the N - 1 nodes has three
    possible states: both halves, right only (left skipped), left only (right skipped)."""
    mask = np.zeros(N, bool)
    mask[np.asarray(info)] = True
    states = set()
    M = N
    while M >= 2:
        for S in range(0, N, M):
            left, right = bool(mask[S:S + M // 2].any()), bool(mask[S + M // 2:S + M].any())
            if left or right:
                states.add((M, S, left, right))
        M //= 2
    return states


def all_branch_states(N=128):
    """Every (node, state) pair: 3 (N - 1) of them."""
    return {(M, S, l, r) for M in (2 ** k for k in range(1, N.bit_length())) for S in range(0, N, M)
            for l, r in ((True, True), (False, True), (True, False))}


@functools.lru_cache(maxsize=None)
def block_family():
    """The 14 sets {i : ((i >> j) & 1) == v}, j = 0 .. 6, v = 0, 1 (K = 64 each), as (name, info).
    None is reliability ordered; together they enter every SC node in each of its three states."""
    i = np.arange(128)
    return tuple((f"bit{j}={v}", i[((i >> j) & 1) == v].astype(np.int32)) for j in range(7) for v in (0, 1))


@functools.lru_cache(maxsize=None)
def edge_family():
    """Constructed sets at the epilogue's word edges (K = 27: 3 payload bits under CRC-24, 7
    syndrome nibbles, the last partial; 63 and 65: either side of the one-word boundary; 90: two
    words and a partial nibble) and the (128,64) set mirrored (127 - i)."""
    sets = [(f"K{K}", info_set(128, K)) for K in (27, 63, 65, 90)]
    sets.append(("mirror64", np.sort(127 - info_set(128, 64)).astype(np.int32)))
    return tuple(sets)


def family():
    """The 19 information sets of the branch-state tests, as (name, info)."""
    return block_family() + edge_family()


def family_set(name):
    return dict(family())[name]


def shift_to_valid(rows, info, crc, seed, N=128, E=0):
    """Rows on which SC alone decides: each row's signs are flipped by the codeword of
    u[info] = s ^ t, with s the oracle's SC result on the row and t = attach_crc(random payload).
    SC commutes with the sign pattern of a codeword (f and g are odd in the flipped operands), so
    the oracle's SC result on the new row is t: random, non-zero, CRC-valid, and every magnitude is
    kept.  (Not the all-zero target: a kernel that wrongly skips a sub-tree decides zeros.)
    Rate-matched rows (E): s is the SC result on the internal row, and the codeword goes through the
    TX chain (sub-block interleave, rate match) to the received positions -- every repeat of a
    position flips with it, so the de-rate-matched mean flips exactly.  Returns (rows', t); asserts
    on every row, by the oracle alone, that sc_decode of the (internal) new row is t and that t
    passes the CRC."""
    rng = np.random.default_rng(seed)
    K = len(info)
    kp = K - (oracle.poly_int(crc).bit_length() - 1)
    out = np.empty_like(rows)
    tgt = np.empty((len(rows), K), np.int8)
    for b, r in enumerate(rows):
        t = oracle.attach_crc(rng.integers(0, 2, size=kp).astype(np.int8), crc)
        u = np.zeros(N, np.int8)
        u[info] = oracle.sc_decode(internal_rows(r[None], N, E)[0], info) ^ t
        x = oracle.polar_transform(u)
        if E:
            from polar_code_amd.nr.polar import rate_match_polar, subblock_interleave

            x = rate_match_polar(subblock_interleave(x), E)
        out[b] = np.where(np.asarray(x) == 1, -r, r)
        tgt[b] = t
        got = oracle.sc_decode(internal_rows(out[b][None], N, E)[0], info)
        assert np.array_equal(got, t), f"row {b}: the oracle's SC result is not the target"
        assert oracle.check_crc(t, crc), f"row {b}: the target fails the CRC"
    return out, tgt


@functools.lru_cache(maxsize=None)
def family_case(name, B=259, L=4):
    """One set of the family: Gaussian rows at 5 dB (seed 500 + K), the composition on them, and
    the rows shifted so that stage 1 decides every frame, with their targets.  B = 256 + 3: four
    full SC wavefronts and a ragged one; the CPU tests take the first 256 rows of the same case."""
    info = family_set(name)
    raw = make_llr(500 + len(info), B, info, POLY24, 5.0)
    shifted, t = shift_to_valid(raw, info, POLY24, seed=900 + len(info))
    for a in (raw, shifted, t):
        a.setflags(write=False)
    return {"info": info, "raw": raw, "exp": compose(raw, info, L, POLY24), "shifted": shifted, "t": t}


@functools.lru_cache(maxsize=None)
def mixed_rows():
    """(128,64)+CRC-24, 5 dB, B = 4099 (64 * 64 + 3), seed 1234."""
    rows = make_llr(1234, 4099, info_set(128, 64), POLY24, 5.0)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def mixed_expected(L):
    return compose(mixed_rows(), info_set(128, 64), L, POLY24)


@functools.lru_cache(maxsize=None)
def allpass_case():
    """12 dB, B = 1000: every SC result passes."""
    rows = make_llr(1235, 1000, info_set(128, 64), POLY24, 12.0)
    return rows, compose(rows, info_set(128, 64), 8, POLY24)


@functools.lru_cache(maxsize=None)
def nr_case():
    """(128,88)+CRC-24 through E = 256, 5 dB, B = 2051, seed 77, L = 8: (rows, expected)."""
    rows = make_llr(77, 2051, info_set(128, 88), POLY24, 5.0, E=256)
    rows.setflags(write=False)
    return rows, compose(rows, info_set(128, 88), 8, POLY24, E=256)


def tiled(exp, reps):
    """The expected values of np.tile(rows, (reps, 1))."""
    out = {k: np.tile(exp[k], (reps, 1) if exp[k].ndim == 2 else reps)
           for k in ("best_bits", "crc_pass", "best_idx", "stage")}
    out["n_escalated"] = reps * exp["n_escalated"]
    return out


@functools.lru_cache(maxsize=None)
def allfail_case():
    """Noise-only rows (no signal term, the 0 dB sigma), B = 1000: every frame escalates."""
    rows = make_llr(1236, 1000, info_set(128, 64), POLY24, 0.0, signal=False)
    return rows, compose(rows, info_set(128, 64), 8, POLY24)
