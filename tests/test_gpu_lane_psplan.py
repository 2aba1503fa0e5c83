"""GPU: the plain lane-per-path screening decodes (scl_lane_kernel<8, 1>, <4, 1>, <8, 2>) with the
compile-time partial-sum plan (scl128_lane.hip PSCL_LANE_PSPLAN, scl_lane.h psplan_*) and the tiers'
ballots combined in SALU, against the oracle on EVERY frame: best bits, CRC flag, best index and the
five device counters of the counting decode bench.py times.

The plan replaces, at the 56 even non-recompute phases, the transform of the runtime window of decided
bits by sign masks over the information bits that can be non-zero.  Rows:

* AWGN at 1, 3 and 5 dB with random messages (the rows and oracle results of test_gpu_lane_diet.py,
  computed once for both files): every partial-sum set takes both parities on live paths;
* "one-hot" rows: for each information bit i the codeword of the message with only bit i set, plus
  the all-ones and the all-zero message, at amplitude 4 (1 + eps_j), |eps_j| <= 0.02 fixed per
  position -- each set's members one at a time.  The distinct magnitudes keep these rows off exact
  ties, so the SCREENING kernel decodes them (a deferred frame is decoded by the exact kernel and
  tests nothing here): at most 5 % of the frames of a kind may be deferred.

Neither change alters an LLR or a metric, so the frames the screening kernel defers are the frames the
parent commit's kernel defers: the count of each kind is pinned to the parent build's (PARENT_DEFERRED)."""
import functools

import numpy as np
import pytest

import adaptive_cases as ac
import oracle
import test_gpu_lane_diet as diet
from polar_code_amd import _native

pytestmark = pytest.mark.gpu
CONFIGS = diet.CONFIGS  # p64-L8, p64-L4, nr88-L8-E256
B_AWGN = diet.B_AWGN    # 1027: whole wavefronts plus a partial one
AWGN = ["awgn 1 dB", "awgn 3 dB", "awgn 5 dB"]
ONE_HOT = "one-hot"

# screening_count() of the parent commit's library (commit f295ef5, build hash 28088db85910f0ce) on the
# same rows, measured once on an MI355X
PARENT_DEFERRED = {
    "p64-L8": {"awgn 1 dB": 6, "awgn 3 dB": 0, "awgn 5 dB": 1, ONE_HOT: 0},
    "p64-L4": {"awgn 1 dB": 0, "awgn 3 dB": 0, "awgn 5 dB": 0, ONE_HOT: 0},
    "nr88-L8-E256": {"awgn 1 dB": 7, "awgn 3 dB": 3, "awgn 5 dB": 2, ONE_HOT: 0},
}


@functools.lru_cache(maxsize=None)
def _one_hot(name):
    """(rows, msg, bits, ok, idx) of the K + 2 one-hot rows of a configuration, computed once."""
    K, L, E = CONFIGS[name]
    info = ac.info_set(128, K)
    msg = np.concatenate([np.eye(K, dtype=np.int8), np.ones((1, K), np.int8), np.zeros((1, K), np.int8)])
    eps = np.random.default_rng(7310).uniform(-0.02, 0.02, size=128)
    internal = 4.0 * (1.0 + eps)[None, :] * (1.0 - 2.0 * diet._codewords(msg, info))
    assert len(np.unique(np.abs(internal[0]))) == 128
    rows = diet._to_received(internal, E)
    bits, ok, idx = oracle.decode_batch(ac.internal_rows(rows, 128, E), info, L, crc=diet.POLY, want_idx=True)
    # (few of these messages carry a valid CRC: the oracle returns its best path, the message itself,
    # unless a CRC-passing word -- all zero, next to the lightest rows -- is still in the list)
    assert np.count_nonzero((bits != msg).any(axis=1)) <= 2, name
    for a in (rows, msg, bits, ok, idx):
        a.setflags(write=False)
    return rows, msg, bits, ok, idx


def _case(name, kind):
    return _one_hot(name) if kind == ONE_HOT else diet._case(name)[kind]


@pytest.fixture(scope="module", params=list(CONFIGS))
def cfg(request):
    K, L, E = CONFIGS[request.param]
    dec = _native.Decoder(128, ac.info_set(128, K), L, diet.POLY)
    if E:
        dec.set_rate_match(E)
    yield request.param, dec, K
    dec.close()


def _check(cfg, kind):
    name, dec, K = cfg
    rows, msg, bits, ok, idx = _case(name, kind)
    best, flags, cnt, deferred = diet._decode_counting(dec, rows, msg, K)
    tag = f"{name}, {kind}"
    print(f"{tag}: {len(rows)} frames, {np.count_nonzero(~ok)} CRC failures, {deferred} deferred "
          f"(parent {PARENT_DEFERRED[name][kind]})")
    np.testing.assert_array_equal(best, diet._words(bits), err_msg=f"{tag}: best bits")
    np.testing.assert_array_equal((flags & 0x80) != 0, ok, err_msg=f"{tag}: CRC flag")
    np.testing.assert_array_equal(flags & 0x3F, idx, err_msg=f"{tag}: best index")
    np.testing.assert_array_equal(cnt[:5], diet._expected_counters(msg, bits, ok, K - 24), err_msg=f"{tag}: counters")
    assert deferred < 0.05 * len(rows), f"{tag}: {deferred} of {len(rows)} frames deferred"
    assert deferred == PARENT_DEFERRED[name][kind], f"{tag}: {deferred} deferred, the parent build {PARENT_DEFERRED[name][kind]}"


@pytest.mark.parametrize("kind", AWGN)
def test_awgn_every_frame(cfg, kind):
    _check(cfg, kind)


def test_one_hot_every_frame(cfg):
    _check(cfg, ONE_HOT)
