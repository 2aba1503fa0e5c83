"""GPU: the deferred-frame count of consecutive screening decodes (capi.cpp launch_decode and
pscl_screening_count: one count word per count slot -- the call parities of a pipelined handle, one slot
on a stream-ordered one -- zeroed in front of every screening launch, read by the exact re-decode and by
the host).  What can go wrong with any scheme that zeroes that word elsewhere (two words per slot used
alternately, the idle one zeroed after the exact re-decode on the stream that ran it: built, measured
against this form and not kept, profiles/r09_ab.txt) is a stale count (a word not zeroed before its next
use) or one zeroed early (before the host read it, or before the re-decode read it -- then deferred frames
stay undecoded); this test holds either form to the same figures.

Five consecutive decode_device calls of B = 8 F + 5 frames (F = 64 / L frames per wavefront), and of one
frame, at L = 8 and 4 on a stream-ordered handle and on a pipelined one (depth 2, alternating output
buffers), join() and screening_count() after every call and once more after the last.  Rows: the 5 dB AWGN
rows of lane_tier_cases.py; in call i, k_i = 5, 0, 3, 0, 7 of them are overwritten by rows of constant
magnitude 4096 and random signs, which the screening decode defers outright (a lane's channel magnitudes
sum to 16 * 4096 * log2 e or more, past PSCL_TAIL2_CHAN_SUM; test_screening_bits_domain_bound_deferred).
Every call's best words, CRC flag and best index equal oracle.decode_batch, and every call's count c_i
satisfies k_i <= c_i <= k_i + ceil(0.02 B): the tier tests' cap on what the certificates may defer on
their own."""
import functools
import math

import numpy as np
import pytest

import adaptive_cases as ac
import lane_tier_cases as tc
import oracle
from polar_code_amd import _native
from test_gpu_lane_tiers import _words
from test_gpu_screening import _header_const

pytestmark = pytest.mark.gpu
KS = (5, 0, 3, 0, 7)
# seed of the overwritten positions and signs: the first of 0, 1, 2, .. with which no call exceeds the cap
# on the parent build (as lane_tier_cases.SEEDS; the cap is asserted below)
SEED = 0


@functools.lru_cache(maxsize=None)
def calls(L, B, seed=SEED):
    """[(rows float64 [B, 128], k, best words, CRC pass, best index)] of the five calls."""
    name = f"p64-L{L}"
    K = tc.CONFIGS[name][0]
    info = ac.info_set(128, K)
    base = tc.case(name)[0]["awgn 5 dB"][:B].astype(np.float64)
    rng = np.random.default_rng(7300 + 16 * seed + L)
    bound = _header_const("PSCL_TAIL2_CHAN_SUM") / _header_const("PSCL_LOG2E_F64")
    out = []
    for k in KS:
        k = min(k, B)
        x = base.copy()
        pos = rng.choice(B, size=k, replace=False)
        x[pos] = 4096.0 * rng.choice([-1.0, 1.0], size=(k, 128))
        lanes = np.abs(x).reshape(B, 128 // L, L).sum(axis=1)  # (a lane holds the row positions i = p mod L)
        assert np.count_nonzero(lanes.max(axis=1) >= bound) == k and np.all(lanes[pos].min(axis=1) >= bound)
        bits, ok, idx = oracle.decode_batch(x, info, L, crc=tc.POLY, want_idx=True)
        x.setflags(write=False)
        out.append((x, k, _words(bits), ok, idx))
    return out


def run(L, B, pipe, seed=SEED):
    """The five calls on a fresh handle: [(k, count after the call, best words, flags)], and the count read
    once more after the last call."""
    seq = calls(L, B, seed)
    dec = _native.Decoder(128, ac.info_set(128, tc.CONFIGS[f"p64-L{L}"][0]), L, tc.POLY)
    try:
        if pipe:
            dec.set_pipelined(True, depth=2)
        W = dec.W
        with _native.DeviceArena(dec) as mem:
            d_llr = [mem.alloc(B * 128 * 8) for _ in seq]
            d_out = [(mem.alloc(B * W * 8), mem.alloc(max(B, 8))) for _ in range(2)]
            for d, c in zip(d_llr, seq):
                mem.upload(d, np.ascontiguousarray(c[0]))
            got = []
            for i, c in enumerate(seq):
                d_best, d_flags = d_out[i % 2]
                mem.memset(d_flags, 0x55, max(B, 8))
                dec.decode_device(d_llr[i], B, d_best=d_best, d_flags=d_flags)
                dec.join()
                n = dec.screening_count()
                got.append((c[1], n, mem.download(d_best, B * W * 8, np.uint64).reshape(B, W),
                            mem.download(d_flags, max(B, 8), np.uint8)[:B]))
            dec.join()
            return got, dec.screening_count()
    finally:
        dec.close()


@pytest.mark.parametrize("pipe", [False, True], ids=["plain", "pipelined"])
@pytest.mark.parametrize("one", [False, True], ids=["8F+5", "B=1"])
@pytest.mark.parametrize("L", [8, 4])
def test_count_of_five_consecutive_calls(L, one, pipe):
    B = 1 if one else tc.batch_sizes(L)[-1]
    got, last = run(L, B, pipe)
    cap = math.ceil(0.02 * B)
    print(f"L = {L}, B = {B}, {'pipelined' if pipe else 'plain'}: (k, count) per call {[(k, n) for k, n, _, _ in got]}, "
          f"read again {last}, cap k + {cap}")
    for i, ((k, n, best, flags), (_, _, words, ok, idx)) in enumerate(zip(got, calls(L, B))):
        tag = f"L = {L}, B = {B}, {'pipelined' if pipe else 'plain'}, call {i}"
        np.testing.assert_array_equal(best, words, err_msg=f"{tag}: best bits")
        np.testing.assert_array_equal((flags & 0x80) != 0, ok, err_msg=f"{tag}: CRC flag")
        np.testing.assert_array_equal(flags & 0x3F, idx, err_msg=f"{tag}: best index")
        assert k <= n <= k + cap, f"{tag}: count {n}, {k} rows past the channel-sum bound, cap k + {cap}"
    assert last == got[-1][1]
