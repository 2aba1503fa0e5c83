"""CPU: a host model of the plain tiers' packed winner-to-freed-lane matching and of their lane-by-lane
certificates (scl128_lane.hip, the plain full-list information phase; helpers in scl_lane.h).

(a) The ranked tier matches the j-th freed lane of a frame with the j-th winner, both counted in lane
order.  The kernel builds one packed word per frame, nibble k = the lane of the k-th winner: each
winner of path index p ORs in p << 4 r, r = popcount(w8 & below(p)), over the frame's lanes; a freed
lane reads (W >> 4 j) & (G - 1).  Whatever the two masks hold, the lane read lies inside the frame; on
every disjoint pair of equal population it is nth_set_bit8's map (test_lane_tiers_cpu.py), lane by lane.

(b) A frame is deferred when ANY of its lanes sets its bit of the ambiguity mask, so a condition "for
all lanes X" needs no frame reduction: each lane tests its own value.  The ranked tier tests
nm > smax per lane where it compared frame_min(nm) with smax; the one-swap tier tests
ismax || kgu < gmax and !bad || wu < gmax per lane where it compared two frame maxima with gmax.
Deferred or not must be identical, ties included."""
import itertools

import numpy as np

from test_lane_tiers_cpu import POP, _select, nth_set_bit8

NONE = 0xFFFFFFFF


def packed_word(w8, G):
    """The frame's packed word as the kernel forms it: the OR of the winners' contributions."""
    W = 0
    for p in range(G):
        if (w8 >> p) & 1:
            W |= p << (4 * POP[w8 & ((1 << p) - 1)])
    return W


def packed_source(f8, w8, p, G):
    j = POP[f8 & ((1 << p) - 1)]
    return (packed_word(w8, G) >> (4 * j)) & (G - 1)


def test_packed_word_fits_32_bits_and_lists_the_winners_in_lane_order():
    for G in (4, 8):
        for w8 in range(1 << G):
            W = packed_word(w8, G)
            assert W < 1 << 32
            winners = [q for q in range(G) if (w8 >> q) & 1]
            assert [(W >> (4 * k)) & 15 for k in range(len(winners))] == winners
            assert W >> (4 * len(winners)) == 0


def test_every_source_lies_in_the_frame_and_matches_nth_set_bit8():
    pairs = 0
    for G in (4, 8):
        for f8 in range(1 << G):
            for w8 in range(1 << G):
                src = [packed_source(f8, w8, p, G) for p in range(G)]
                assert all(0 <= s < G for s in src), (G, f8, w8, src)  # every pair, every lane
                if f8 & w8 or POP[f8] != POP[w8]:
                    continue
                freed = [p for p in range(G) if (f8 >> p) & 1]
                assert sorted(src[p] for p in freed) == [q for q in range(G) if (w8 >> q) & 1]
                for p in freed:
                    assert src[p] == nth_set_bit8(w8, POP[f8 & ((1 << p) - 1)]), (G, f8, w8, p)
                pairs += 1
    # disjoint pairs of equal population: sum over k of C(G, k) C(G - k, k)
    assert pairs == 19 + 1107


def _up(k):
    """A stand-in of the margin-raised key hiw_up: monotone, above the key."""
    return 2 * k + 1


def _ranked(kg, kb, L):
    """The ranked tier's certificate on key arrays [n, L]: (reduction form, lane-by-lane form)."""
    keep, win, d = _select(kg, kb, L)
    kgu, kbu = _up(kg), _up(kb)
    su = np.where(win, kbu, np.where(keep, kgu, 0))
    nm = np.where(keep, np.where(win, NONE, 2 * kb), 2 * kg)  # (keys on hiw_up's scale)
    smax = su.max(axis=1, keepdims=True)
    count = (win.sum(axis=1) == d)[:, None]
    old = ~(count[:, 0] & (nm.min(axis=1) > smax[:, 0]))
    new = (~(count & (nm > smax))).any(axis=1)
    return old, new


def _one_swap(kg, kb, L):
    """The one-swap tier's certificate, for the frames the tier takes (at most one worse child that is
    not clear of every better child): (reduction form, lane-by-lane form, the frames)."""
    kg2, kb2, kgu, kbu = 2 * kg, 2 * kb, _up(kg), _up(kb)
    mx = kgu.max(axis=1, keepdims=True)
    bad = kb2 <= mx
    takes = bad.sum(axis=1) <= 1
    swap = bad.any(axis=1)
    gmax = kg2.max(axis=1, keepdims=True)
    ismax = kg2 == gmax
    nmax = ismax.sum(axis=1)
    g2u = np.where(ismax, 0, kgu).max(axis=1)
    wu = np.where(bad, kbu, 0).max(axis=1)
    old = swap & ~((nmax == 1) & (g2u < gmax[:, 0]) & (wu < gmax[:, 0]))
    lane = swap[:, None] & ~((nmax == 1)[:, None] & (ismax | (kgu < gmax)) & (~bad | (kbu < gmax)))
    return old[takes], lane.any(axis=1)[takes], takes


def _check(kg, kb, L):
    assert np.all(kb >= kg)
    old, new = _ranked(kg, kb, L)
    np.testing.assert_array_equal(new, old)
    sold, snew, takes = _one_swap(kg, kb, L)
    np.testing.assert_array_equal(snew, sold)
    return old, sold, takes


def test_certificates_l4_exhaustive_over_a_4_letter_alphabet():
    keys = np.array(list(itertools.product(range(4), repeat=8)))  # 4^8 key vectors: every tie pattern
    kg, kb = np.minimum(keys[:, :4], keys[:, 4:]), np.maximum(keys[:, :4], keys[:, 4:])
    old, sold, takes = _check(kg, kb, 4)
    assert len(keys) == 4 ** 8
    assert old.any() and not old.all() and takes.any() and sold.any() and not sold.all()


def test_certificates_l8_random_keys_with_ties_and_distinct():
    rng = np.random.default_rng(909)
    keys = rng.integers(0, 6, size=(100000, 16))  # a 6-letter alphabet: ties everywhere
    kg, kb = np.minimum(keys[:, :8], keys[:, 8:]), np.maximum(keys[:, :8], keys[:, 8:])
    old, sold, takes = _check(kg, kb, 8)
    assert old.any()
    # one-swap frames are rare among uniform keys: a batch shaped like the tier's (better children
    # low, worse children high, one of them pulled down among the better ones), ties included
    kg = rng.integers(0, 6, size=(100000, 8))
    kb = kg + 6 + rng.integers(0, 6, size=(100000, 8))
    lane = rng.integers(0, 8, size=100000)
    rows = np.arange(100000)
    kb[rows, lane] = kg[rows, lane] + rng.integers(0, 3, size=100000)
    old, sold, takes = _check(kg, kb, 8)
    assert takes.sum() > 10000 and sold.any() and not sold.all()
    # distinct keys: a random permutation of 16 spread keys per frame
    keys = np.argsort(rng.random((100000, 16)), axis=1) * 3
    kg, kb = np.minimum(keys[:, :8], keys[:, 8:]), np.maximum(keys[:, :8], keys[:, 8:])
    old, sold, takes = _check(kg, kb, 8)
    assert not old.all()
