"""Inputs and expected values of the off-code tests (test_offcode_cpu.py, test_gpu_offcode.py):
the compiled-in (128,64) and (128,88) information sets under other CRC polynomials and under none,
and the list decoders on information sets that construct_info_set never gives (position 0,
without N - 1, K = N, a list that fills at the last phase or never).  Expected values come from
the oracle alone (decode_scl, decode_batch, dl_batch, decode_with_retries; adaptive_cases.compose),
which test_oracle_golden.py pins to the reference on a slice of these cases (tests/golden/
g17_offcode.npz).  Each case is computed once per session and shared read-only."""
import functools

import numpy as np

import adaptive_cases as ac
import oracle

POLY24 = ac.POLY24
# none, then degrees 1, 6, 11, 16, 24 (not POLY24) and 32 (PSCL_MAX_CRC)
CRCS = (None, "0x3", "0x61", "0xE21", "0x11021", "0x1B2B117", "0x104C11DB7")
NONEMPTY = CRCS[1:]
# the compiled-in codes: tag -> (K, rate-matched length E)
CODES = {"k64": (64, 0), "k88": (88, 256)}
EBNO = (1.0, 3.0, 5.0)
PER_POINT, ROUNDED = 65, 64  # B = 3 * 65 + 64 = 259: four wavefronts of frames and a ragged one
# DL-SCL batches: Eb/N0 per polynomial, picked with the oracle so that a tenth to a third of the 595
# frames fail the baseline at L = 4 and 8 (one parity bit passes some list entry of most frames, so
# its batch lies far below the others'); test_offcode_cpu.py asserts the shares
DL_EBNO = {"0x3": -6.0, "0x61": 3.5, "0xE21": 3.5, "0x11021": 3.5, "0x1B2B117": 3.5, "0x104C11DB7": 3.5}
DL_B, DL_RETRIES = 595, 8
# family batch per code length: h Gaussian rows, h rounded, 3 fixed (B = 67, 35, 19: all ragged)
FAMILY_HALF = {32: 32, 128: 32, 256: 16, 512: 8, 1024: 8}
FULL_SHAPES = ([(N, L) for N in (32, 128) for L in (1, 2, 3, 4, 8, 16, 32)] + [(256, L) for L in (3, 4, 8, 32)])
LONG_SETS = ("head", "all", "random", "blocks")  # N = 512, 1024 at L = 8


def crc_id(crc):
    return "none" if crc is None else crc


def degree(crc):
    return max(oracle.poly_int(crc).bit_length() - 1, 0)


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def words(bits):
    bits = np.asarray(bits)
    B, K = bits.shape
    w = np.zeros((B, (K + 63) // 64 if K > 64 else 1), np.uint64)
    for j in range(K):
        w[:, j >> 6] |= bits[:, j].astype(np.uint64) << np.uint64(j & 63)
    return w


# ------------------------------------------------------------------ part 1: the CRC axis

@functools.lru_cache(maxsize=None)
def crc_rows(code, crc):
    """(rows [259, E or 128], msg [259, K], internal rows [259, 128]) of a compiled-in code under
    `crc`: 65 frames at each of EBNO (adaptive_cases.make_llr) and the first 64 rounded to integers
    (exact metric ties; their message is the unrounded frame's)."""
    K, E = CODES[code]
    info = ac.info_set(128, K)
    parts = [ac.make_llr(7000 + 100 * i + K + degree(crc), PER_POINT, info, crc, e, E=E, with_msg=True)
             for i, e in enumerate(EBNO)]
    rows = np.concatenate([p[0] for p in parts] + [np.round(parts[0][0][:ROUNDED])])
    msg = np.concatenate([p[1] for p in parts] + [parts[0][1][:ROUNDED]])
    x = np.ascontiguousarray(ac.internal_rows(rows, 128, E))
    frozen(rows, msg, x)
    return rows, msg, x


AWGN = slice(0, 3 * PER_POINT)
TIES = slice(3 * PER_POINT, 3 * PER_POINT + ROUNDED)
FULL = np.r_[0:32, 3 * PER_POINT:3 * PER_POINT + 32]  # the 64 frames of the full-output comparison


@functools.lru_cache(maxsize=None)
def crc_plain(code, crc, L):
    """oracle.decode_batch on the internal rows: dict(best_bits, crc_pass, best_idx)."""
    K, _ = CODES[code]
    bits, ok, idx = oracle.decode_batch(crc_rows(code, crc)[2], ac.info_set(128, K), L, crc=crc, want_idx=True)
    frozen(bits, ok, idx)
    return {"best_bits": bits, "crc_pass": ok, "best_idx": idx}


def scl_all(x, info, L, crc):
    """oracle.decode_scl on every row: dict(n_paths [B], cands [B, L, K], metrics [B, L],
    info_llrs [B, L, K], best_idx [B])."""
    B, K = len(x), len(info)
    out = {"n_paths": np.zeros(B, np.int32), "cands": np.zeros((B, L, K), np.int8), "metrics": np.full((B, L), np.nan),
           "info_llrs": np.full((B, L, K), np.nan), "best_idx": np.zeros(B, np.int32)}
    for f in range(B):
        n, c, m, il, b = oracle.decode_scl(x[f], info, L, crc=crc)
        out["n_paths"][f], out["cands"][f], out["metrics"][f], out["info_llrs"][f], out["best_idx"][f] = n, c, m, il, b
    frozen(*out.values())
    return out


@functools.lru_cache(maxsize=None)
def crc_full(code, crc, L=8):
    K, _ = CODES[code]
    return scl_all(crc_rows(code, crc)[2][FULL], ac.info_set(128, K), L, crc)


def assert_full(out, exp, tag, llr_bits=True):
    """Decoder.decode's full outputs == scl_all's, the first n_paths list entries of every frame;
    metrics and decision LLRs as integer views (bit for bit, signed zeros included).  llr_bits=False
    (the GPU kernels): decision LLRs by value -- f_minsum (csrc/scl_device.h) gives a zero the XOR of
    its operands' signs where the reference's sign(0) = 0 gives it the nonzero operand's, and the sign
    of a zero reaches no decision and no metric; metrics stay bit for bit."""
    np.testing.assert_array_equal(out["n_paths"], exp["n_paths"], err_msg=f"{tag}: n_paths")
    np.testing.assert_array_equal(out["best_idx"], exp["best_idx"], err_msg=f"{tag}: best_idx")
    L = exp["metrics"].shape[1]
    live = np.arange(L)[None, :] < exp["n_paths"][:, None]
    np.testing.assert_array_equal(out["cands"][live], exp["cands"][live], err_msg=f"{tag}: candidates")
    for k in ("metrics", "info_llrs"):
        got, want = np.ascontiguousarray(out[k][live]), np.ascontiguousarray(exp[k][live])
        if k == "metrics" or llr_bits:
            got, want = got.view(np.int64), want.view(np.int64)
        else:
            assert not np.isnan(got).any(), f"{tag}: {k}"
        np.testing.assert_array_equal(got, want, err_msg=f"{tag}: {k}")
    f = np.arange(len(exp["best_idx"]))
    np.testing.assert_array_equal(out["best_bits"], exp["cands"][f, exp["best_idx"]], err_msg=f"{tag}: best_bits")


@functools.lru_cache(maxsize=None)
def crc_f32(code, crc, L):
    """(float32 rows, oracle.decode_batch on the widened rows' internal rows)."""
    K, E = CODES[code]
    rows32 = np.ascontiguousarray(crc_rows(code, crc)[0], np.float32)
    x = np.ascontiguousarray(ac.internal_rows(rows32.astype(np.float64), 128, E))
    bits, ok, idx = oracle.decode_batch(x, ac.info_set(128, K), L, crc=crc, want_idx=True)
    frozen(rows32, bits, ok, idx)
    return rows32, {"best_bits": bits, "crc_pass": ok, "best_idx": idx}


@functools.lru_cache(maxsize=None)
def crc_adaptive(code, crc, L):
    K, E = CODES[code]
    exp = ac.compose(crc_rows(code, crc)[0], ac.info_set(128, K), L, crc, E=E)
    frozen(*exp.values())
    return exp


@functools.lru_cache(maxsize=None)
def dl_rows(crc):
    """(rows [595, 128], msg) of the (128,64) code under `crc` at DL_EBNO[crc]."""
    rows, msg = ac.make_llr(7700 + degree(crc), DL_B, ac.info_set(128, 64), crc, DL_EBNO[crc], with_msg=True)
    frozen(rows, msg)
    return rows, msg


@functools.lru_cache(maxsize=None)
def beta_m8():
    from conftest import GOLDEN

    b = np.load(GOLDEN / "beta_M8.npy")
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def dl_case(crc, L, with_beta):
    """oracle.dl_batch on every frame, oracle.decode_with_retries on every 20th (`tried`), and the
    baseline's decode_batch."""
    rows, _ = dl_rows(crc)
    info, beta = ac.info_set(128, 64), beta_m8() if with_beta else None
    bits, succ, att = oracle.dl_batch(rows, info, L, DL_RETRIES, crc=crc, beta=beta)
    base_bits, base_pass = oracle.decode_batch(rows, info, L, crc=crc)
    every = np.arange(0, len(rows), 20)
    tried = np.full((len(every), DL_RETRIES), -1, np.int32)
    for i, f in enumerate(every):
        r = oracle.decode_with_retries(rows[f], info, L, DL_RETRIES, crc=crc, beta=beta)
        assert r["attempts"] == att[f] and r["success"] == bool(succ[f]) and np.array_equal(r["bits"], bits[f])
        tried[i, : len(r["tried"])] = r["tried"]
    exp = {"best_bits": bits, "success": succ, "attempts": att, "base_bits": base_bits, "base_pass": base_pass,
           "every": every, "tried": tried}
    frozen(*exp.values())
    return exp


# ------------------------------------------------------------------ part 2: the information-set axis

def _log2(L):
    return L.bit_length() - 1 if L >= 1 and L & (L - 1) == 0 else None


@functools.lru_cache(maxsize=None)
def info_family(N, L):
    """Named information sets of length N, all sorted, as a dict name -> int32 array.  fills_last
    (log2 L positions, 0 and N - 1 among them: the list is full only after the last phase) and short
    (log2 L - 1 positions: 2^K < L paths) exist where L is a power of two >= 4."""
    i = np.arange(N)
    fam = {"head": i[: N // 2], "tail": i[N // 2:], "all": i, "bit0=0": i[(i & 1) == 0], "bit0=1": i[(i & 1) == 1],
           "blocks": i[((i >> 4) & 1) == 0]}
    rng = np.random.default_rng(1700 + N)
    fam["random"] = np.sort(np.concatenate([[0], rng.choice(np.arange(1, N - 1), N // 2 - 1, replace=False)]))
    k = _log2(L)
    if k is not None and k >= 2:
        fam["fills_last"] = np.unique(np.round(np.linspace(0, N - 1, k)).astype(np.int64))
        fam["short"] = np.unique(np.round(np.linspace(N // 4, 3 * N // 4, k - 1)).astype(np.int64))
        assert fam["fills_last"].size == k and fam["short"].size == k - 1
    fam["first_only"] = i[:1]
    fam["last_only"] = i[-1:]
    out = {name: np.ascontiguousarray(s, np.int32) for name, s in fam.items()}
    for s in out.values():
        assert np.all(np.diff(s) > 0)
    frozen(*out.values())
    assert out["random"][0] == 0 and out["random"][-1] < N - 1 and out["random"].size == N // 2
    return out


def family_names(N, L, every=False):
    """The sets of the full-output comparisons: all at N <= 256, LONG_SETS above (every: all)."""
    return tuple(info_family(N, L)) if N <= 256 or every else LONG_SETS


def family_crc(info):
    """CRC-24 where K > 24, otherwise none."""
    return POLY24 if len(info) > 24 else None


@functools.lru_cache(maxsize=None)
def family_rows(N, name, L):
    """h rows normal(1.0, 2.5) with random signs, those rows rounded to integers (exact ties: the
    stable sort's order decides), then all +0.0, all -0.0 and a noiseless codeword (+-2)."""
    info = info_family(N, L)[name]
    crc = family_crc(info)
    h = FAMILY_HALF[N]
    rng = np.random.default_rng([1701, N, L, sum(name.encode())])
    g = rng.normal(1.0, 2.5, size=(h, N)) * rng.choice([-1.0, 1.0], size=(h, N))
    pay = rng.integers(0, 2, size=len(info) - degree(crc)).astype(np.int8)
    u = np.zeros(N, np.int8)
    u[info] = oracle.attach_crc(pay, crc) if crc else pay
    rows = np.concatenate([g, np.round(g), np.full((1, N), 0.0), np.full((1, N), -0.0),
                           2.0 * (1.0 - 2.0 * oracle.polar_transform(u))[None, :]])
    rows.setflags(write=False)
    return rows


def family_ties(N):
    h = FAMILY_HALF[N]
    return slice(h, 2 * h)


@functools.lru_cache(maxsize=None)
def family_case(N, name, L):
    """dict(info, crc, rows, exp = scl_all on the rows, crc_pass [B])."""
    info = info_family(N, L)[name]
    crc = family_crc(info)
    rows = family_rows(N, name, L)
    exp = scl_all(rows, info, L, crc)
    f = np.arange(len(rows))
    best = exp["cands"][f, exp["best_idx"]]
    ok = np.array([oracle.check_crc(b, crc) if crc else True for b in best], bool)
    frozen(best, ok)
    return {"info": info, "crc": crc, "rows": rows, "exp": exp, "best_bits": best, "crc_pass": ok}


def expected_paths(K, L):
    return min(L, 2 ** K) if K < 31 else L


# ------------------------------------------------------------------ the slice the reference was run on (g17)

def rows_sha(rows):
    import hashlib

    return hashlib.sha256(np.ascontiguousarray(rows, np.float64).tobytes()).hexdigest()


def g17_cases():
    """(tag, N, info, CRC, L, rows) of golden g17 (tests/golden/make_golden.py g17 runs the reference
    on them): the (128,64) code at L = 8 under each of CRCS (an AWGN and a rounded frame), every
    info_family set at N = 32, 128 and L = 4, 8 (a Gaussian and a rounded frame), and head, all and
    short at N = 256, L = 4 (the rounded frame)."""
    out = []
    for crc in CRCS:
        out.append((f"crc_{crc_id(crc)}", 128, ac.info_set(128, 64), crc, 8, crc_rows("k64", crc)[2][[0, TIES.start]]))
    for N in (32, 128):
        for L in (4, 8):
            for name, info in info_family(N, L).items():
                out.append((f"n{N}_L{L}_{name}", N, info, family_crc(info), L,
                            family_rows(N, name, L)[[0, FAMILY_HALF[N]]]))
    for name in ("head", "all", "short"):
        info = info_family(256, 4)[name]
        out.append((f"n256_L4_{name}", 256, info, family_crc(info), 4, family_rows(256, name, 4)[[FAMILY_HALF[256]]]))
    return out


@functools.lru_cache(maxsize=None)
def g17():
    """g17_offcode.npz unpacked: tag -> dict(N, info, crc, L, llr [F, N], npaths [F], best [F], and per
    frame the first npaths candidates, metrics and decision LLRs).  The file holds one flat array per
    field over the cases, a table of their shapes and the SHA-256 of each case's rows; the rows
    themselves are g17_cases()'s seeded draw, repeated here and checked by the hash."""
    from conftest import GOLDEN

    z = np.load(GOLDEN / "g17_offcode.npz", allow_pickle=False)
    off = {k: 0 for k in ("info", "npaths", "best", "cands", "metrics", "info_llrs")}
    drawn = {tag: rows for tag, *_, rows in g17_cases()}

    def take(k, n):
        a = z[k][off[k]:off[k] + n]
        off[k] += n
        return a

    out = {}
    for tag, row, sha in zip(z["cases"], z["table"], z["llr_sha256"]):
        N, K, poly, L, F = (int(v) for v in row)
        llr = drawn[str(tag)]
        assert llr.shape == (F, N) and rows_sha(llr) == sha.decode(), f"{tag}: the rows' draw changed"
        c = {"N": N, "crc": hex(poly) if poly else None, "L": L, "info": take("info", K).astype(np.int32),
             "llr": llr, "npaths": take("npaths", F), "best": take("best", F),
             "cands": [], "metrics": [], "info_llrs": []}
        for n in c["npaths"]:
            c["cands"].append(take("cands", n * K).reshape(n, K))
            c["metrics"].append(take("metrics", n))
            c["info_llrs"].append(take("info_llrs", n * K).reshape(n, K))
        out[str(tag)] = c
    assert all(off[k] == z[k].size for k in off)
    return out
