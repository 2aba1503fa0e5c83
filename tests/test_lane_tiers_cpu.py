"""CPU: a host model of the ranked tier's survivor-count certificate and of its winner-to-freed-lane
matching (scl128_lane.hip, the plain full-list information phase; helpers in scl_lane.h).

The kernel ranks a frame's 2L children (rank counts rg, rbb of strict compares), keeps a better child
when rg < L, lets a worse child win when it is among the d smallest worse children (d = the number
of dropped better children), and certifies "exactly L survivors".  It forms that test from the two
lane masks it needs for the pull anyway -- f8 (lanes whose better child is dropped) and w8 (lanes
whose worse child wins): popcount(w8) == popcount(f8), since survivors = (L - d) + winners and
d = popcount(f8).  The earlier form summed keep_g + win_b over the frame's lanes and compared with L.
Each freed lane then pulls the j-th winner, j = its rank among the freed lanes (nth_set_bit8); with
self-sourced pulls a lane that keeps its child reads its own lane instead."""
import itertools

import numpy as np

POP = np.array([bin(i).count("1") for i in range(256)])


def nth_set_bit8(m, j):
    """scl_lane.h nth_set_bit8, branch for branch."""
    c4 = POP[m & 15]
    h4 = j >= c4
    j = j - c4 if h4 else j
    m = (m >> 4) if h4 else (m & 15)
    c2 = POP[m & 3]
    h2 = j >= c2
    j = j - c2 if h2 else j
    m = (m >> 2) if h2 else m
    h1 = j >= (m & 1)
    return (4 if h4 else 0) + (2 if h2 else 0) + (1 if h1 else 0)


def sources(f8, w8, G):
    """The lane each lane of a frame reads in the pull: a freed lane its winner, a keeper itself."""
    out = []
    for p in range(G):
        pull = (f8 >> p) & 1
        j = POP[f8 & ((1 << p) - 1)]
        out.append(nth_set_bit8(w8, j) if pull else p)
    return out


def test_matching_is_a_bijection_onto_the_winners():
    n = 0
    for G in (4, 8):
        for f8 in range(1 << G):
            for w8 in range(1 << G):
                if POP[f8] != POP[w8]:
                    continue
                src = sources(f8, w8, G)
                pulled = sorted(src[p] for p in range(G) if (f8 >> p) & 1)
                assert pulled == [q for q in range(G) if (w8 >> q) & 1], (G, f8, w8, src)
                assert all(src[p] == p for p in range(G) if not (f8 >> p) & 1)
                assert all(0 <= s < G for s in src)
                n += 1
    assert n == 70 + 12870  # C(8,4) and C(16,8): the pairs of equal population


def test_popcount_certificate_equals_survivor_sum_on_every_mask_pair():
    for G in (4, 8):
        full = (1 << G) - 1
        keep, win = np.meshgrid(np.arange(1 << G), np.arange(1 << G), indexing="ij")
        old = POP[keep] + POP[win] == G
        new = POP[win] == POP[~keep & full]
        np.testing.assert_array_equal(new, old)


def _select(kg, kb, L):
    """scl_lane.h select_survivors (PSCL_LANE_RANK3) on key arrays [n, L]: strict rank counts."""
    allk = np.concatenate([kg, kb], axis=1)
    rg = (allk[:, None, :] < kg[:, :, None]).sum(axis=2)
    rbb = (kb[:, None, :] < kb[:, :, None]).sum(axis=2)
    keep = rg < L
    d = (~keep).sum(axis=1, keepdims=True)
    return keep, rbb < d, d[:, 0]


def _check_keys(kg, kb, L):
    assert np.all(kb >= kg)
    keep, win, d = _select(kg, kb, L)
    bits = 1 << np.arange(L)
    f8, w8 = (~keep * bits).sum(axis=1), (win * bits).sum(axis=1)
    old = (keep.sum(axis=1) + win.sum(axis=1)) == L
    new = POP[w8] == POP[f8]
    np.testing.assert_array_equal(new, old)
    np.testing.assert_array_equal(POP[f8], d)
    # distinct keys: the selection is exact (the L smallest of the 2L children) and always certified
    allk = np.concatenate([kg, kb], axis=1)
    distinct = np.array([len(set(r)) == 2 * L for r in allk])
    if distinct.any():
        assert old[distinct].all()
        thr = np.sort(allk[distinct], axis=1)[:, L - 1:L]
        np.testing.assert_array_equal(keep[distinct], kg[distinct] <= thr)
        np.testing.assert_array_equal(win[distinct], kb[distinct] <= thr)
    return int(np.count_nonzero(~old)), int(np.count_nonzero(distinct))


def test_certificate_on_ranked_keys_with_ties():
    # L = 4: every key pattern over a 5-letter alphabet with kb >= kg (ties of every shape)
    pairs = [(a, b) for a in range(5) for b in range(a, 5)]
    combos = np.array(list(itertools.product(range(len(pairs)), repeat=4)))
    pk = np.array(pairs)
    rejected, _ = _check_keys(pk[combos, 0], pk[combos, 1], 4)
    assert rejected > 0  # equal keys do give wrong counts: the certificate is what rejects them
    # L = 8: random keys, a small alphabet (many ties) and a large one (mostly distinct)
    rng = np.random.default_rng(808)
    for hi in (6, 12, 1 << 20):
        kg = rng.integers(0, hi, size=(40000, 8))
        kb = kg + rng.integers(0, hi, size=(40000, 8))
        rejected, ndistinct = _check_keys(kg, kb, 8)
        assert (rejected > 0) if hi <= 12 else (ndistinct > 39000)


def test_crafted_rows_have_their_survivor_counts():
    """The crafted batch of every configuration (lane_tier_cases.py), by the oracle alone: each frame has
    the d its place in the pattern asks for, every d = 0 .. L / 2 occurs, and the wavefronts are laid out
    as described -- d = 0 and 1 only, d = 0, 1 and >= 2 together, d = L / 2 throughout."""
    import adaptive_cases as ac
    import lane_tier_cases as tc

    for name, (K, L, E) in tc.CONFIGS.items():
        rows, internal, want = tc.case(name)
        F = 64 // L
        assert rows["crafted d"].dtype == np.float32 and len(want) == 8 * F + 5
        got = np.array([tc.worse_survivors(x, ac.info_set(128, K), L) for x in internal["crafted d"]])
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert set(want) == set(range(L // 2 + 1)), name
        waves = [set(want[w * F:(w + 1) * F]) for w in range(3)]
        assert waves[0] == {0, 1} and waves[2] == {L // 2}, (name, waves)
        assert {0, 1} < waves[1] and max(waves[1]) >= 2, (name, waves)
        # no row sits in two places, and the float32 rows are what the oracle saw
        assert len({r.tobytes() for r in rows["crafted d"]}) == len(want)
        np.testing.assert_array_equal(ac.internal_rows(rows["crafted d"].astype(np.float64), 128, E), internal["crafted d"])
