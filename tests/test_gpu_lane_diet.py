"""GPU: the plain lane-per-path screening decodes (scl_lane_kernel<8, 1>, <4, 1>, <8, 2>) after the
instruction-count trims of their recompute (scl128_lane.hip: PSCL_LANE_GSPLIT, PSCL_LANE_U0T)
against the oracle, on EVERY frame: best bits, CRC flag, best index and the device counters of the
counting decode bench.py times.

The trims touch the depth-1 g nodes of the recomputes at phases 64..112 (the sign flip of a channel
value) and the word u0 those recomputes read (kept transformed from phase 64 on, transformed back
for the epilogue's gather and CRC syndrome).  Besides AWGN rows at three SNRs -- CRC failures and passes at a list index > 0
occur in every configuration, deferred frames at L = 8 (at L = 4 none of these 3,081 frames is within
the margin; the tie rows below are deferred at every list size) -- the rows below stress signs and zeros: noiseless codewords, all-negative
rows, small integers with exact zeros, and rows where one lane's 16 (L = 8) or 32 (L = 4) channel
positions are all -0.0 or all +0.0.  Such rows may all be deferred to the exact kernel; equality
with the oracle is what is asserted."""
import functools

import numpy as np
import pytest

import adaptive_cases as ac
import oracle
from polar_code_amd import _native
from polar_code_amd.nr.polar import rate_match_polar, subblock_interleave
from polar_code_amd.polar import crc as pcrc
from polar_code_amd.polar.polar import _polar_transform

pytestmark = pytest.mark.gpu
POLY = ac.POLY24
B_AWGN, B_KIND = 1027, 256  # 128 (L = 8) / 64 (L = 4) whole wavefronts plus a partial one; 256 rows per kind
CONFIGS = {"p64-L8": (64, 8, 0), "p64-L4": (64, 4, 0), "nr88-L8-E256": (88, 8, 256)}


def _words(bits):
    B, K = bits.shape
    w = np.zeros((B, (K + 63) // 64), np.uint64)
    for j in range(K):
        w[:, j >> 6] |= bits[:, j].astype(np.uint64) << np.uint64(j & 63)
    return w


def _to_received(internal, E):
    """Decoder-internal rows [B, 128] to the rows handed to the decoder (E: through the sub-block
    interleaver and the cyclic repetition; the de-rate-matched mean of equal repeats is exact)."""
    if not E:
        return internal
    return np.stack([rate_match_polar(subblock_interleave(r), E) for r in internal])


def _messages(rng, B, K):
    return pcrc.attach_crc(rng.integers(0, 2, size=(B, K - 24), dtype=np.int8), POLY)


def _codewords(msg, info):
    u = np.zeros((len(msg), 128), np.int8)
    u[:, info] = msg
    return _polar_transform(u)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Rows, reference messages and the oracle's results of one configuration, computed once:
    {kind: (rows, msg, bits, ok, idx)}."""
    K, L, E = CONFIGS[name]
    info = ac.info_set(128, K)
    # (the seed: of 5200..5211 the one whose AWGN rows give, by the oracle alone, a CRC pass at a list
    # index > 0 in both (128,64) configurations -- they are rare there, 0..4 per 1,027 frames)
    rng = np.random.default_rng(5209)
    G = L
    kinds = {}
    for ebno in (1.0, 3.0, 5.0):
        msg = _messages(rng, B_AWGN, K)
        x = _to_received(_codewords(msg, info), E)
        nv = 1.0 / (2.0 * ((K - 24) / E if E else K / 128) * 10 ** (ebno / 10))
        kinds[f"awgn {ebno:g} dB"] = (2.0 * ((1.0 - 2.0 * x) + rng.normal(0.0, np.sqrt(nv), size=x.shape)) / nv, msg)
    msg = _messages(rng, B_KIND, K)
    kinds["noiseless +-4"] = (_to_received(4.0 * (1.0 - 2.0 * _codewords(msg, info)), E), msg)
    kinds["all negative"] = (_to_received(-rng.uniform(0.05, 9.0, size=(B_KIND, 128)), E), _messages(rng, B_KIND, K))
    ints = rng.integers(-3, 4, size=(B_KIND, 128)).astype(np.float64)
    ints[rng.random(ints.shape) < 0.1] = 0.0
    assert (ints == 0.0).sum() > 1000 and ints.min() == -3.0 and ints.max() == 3.0
    kinds["integers with zeros"] = (_to_received(ints, E), _messages(rng, B_KIND, K))
    msg = _messages(rng, B_KIND, K)
    z = 3.0 * ((1.0 - 2.0 * _codewords(msg, info)) + rng.normal(0.0, 0.6, size=(B_KIND, 128)))
    for i in range(B_KIND):  # lane p of a frame holds the positions = p (mod G)
        z[i, (i % G)::G] = -0.0 if (i // G) % 2 else 0.0
    kinds["one lane all zeros"] = (_to_received(z, E), msg)
    out = {}
    for kind, (rows, msg) in kinds.items():
        bits, ok, idx = oracle.decode_batch(ac.internal_rows(rows, 128, E), info, L, crc=POLY, want_idx=True)
        for a in (rows, msg, bits, ok, idx):
            a.setflags(write=False)
        out[kind] = (rows, msg, bits, ok, idx)
    return out


def _expected_counters(msg, bits, ok, kp):
    d = bits != msg
    return np.array([len(msg), np.count_nonzero(~ok), d.sum(), np.count_nonzero(d[:, :kp].any(axis=1)), d[:, :kp].sum()],
                    np.int64)


def _decode_counting(dec, rows, msg, K):
    """The bench's call: device rows, best words, flags and the error counters against msg."""
    B, W = len(rows), (K + 63) // 64
    with _native.DeviceArena(dec) as mem:
        d_llr, d_ref = mem.alloc(rows.nbytes), mem.alloc(B * W * 8)
        d_best, d_flags, d_cnt = mem.alloc(B * W * 8), mem.alloc(B), mem.alloc(64)
        mem.upload(d_llr, rows)
        mem.upload(d_ref, _words(msg))
        mem.memset(d_cnt, 0, 64)
        mem.memset(d_flags, 0x55, B)
        dec.decode_device(d_llr, B, d_best=d_best, d_flags=d_flags, d_ref=d_ref, k_payload=K - 24, d_counters=d_cnt)
        deferred = dec.screening_count()
        return (mem.download(d_best, B * W * 8, np.uint64).reshape(B, W), mem.download(d_flags, B, np.uint8),
                mem.download(d_cnt, 64, np.int64), deferred)


@pytest.fixture(scope="module", params=list(CONFIGS))
def cfg(request):
    K, L, E = CONFIGS[request.param]
    dec = _native.Decoder(128, ac.info_set(128, K), L, POLY)
    if E:
        dec.set_rate_match(E)
    yield request.param, dec, K
    dec.close()


def _check(cfg, kind):
    name, dec, K = cfg
    rows, msg, bits, ok, idx = _case(name)[kind]
    best, flags, cnt, deferred = _decode_counting(dec, rows, msg, K)
    tag = f"{name}, {kind}"
    np.testing.assert_array_equal(best, _words(bits), err_msg=f"{tag}: best bits")
    np.testing.assert_array_equal((flags & 0x80) != 0, ok, err_msg=f"{tag}: CRC flag")
    np.testing.assert_array_equal(flags & 0x3F, idx, err_msg=f"{tag}: best index")
    np.testing.assert_array_equal(cnt[:5], _expected_counters(msg, bits, ok, K - 24), err_msg=f"{tag}: counters")
    print(f"{tag}: {len(rows)} frames, {np.count_nonzero(~ok)} CRC failures, {np.count_nonzero(ok & (idx > 0))} passes "
          f"at index > 0, {deferred} deferred")
    return deferred


def test_awgn_every_frame(cfg):
    name = cfg[0]
    fails = later = 0
    for ebno in (1.0, 3.0, 5.0):
        kind = f"awgn {ebno:g} dB"
        _, _, _, ok, idx = _case(name)[kind]
        d = _check(cfg, kind)
        assert d < 0.05 * B_AWGN, f"{name}, {kind}: {d} of {B_AWGN} frames deferred"
        fails += np.count_nonzero(~ok)
        later += np.count_nonzero(ok & (idx > 0))
    assert fails > 0 and later > 0, (name, fails, later)


@pytest.mark.parametrize("kind", ["noiseless +-4", "all negative", "integers with zeros", "one lane all zeros"])
def test_sign_and_zero_rows_every_frame(cfg, kind):
    deferred = _check(cfg, kind)
    if kind == "integers with zeros":  # exact ties at every phase: the deferral path runs
        assert deferred > B_KIND // 2, (cfg[0], deferred)


def test_pipelined_two_buffers_equal_stream_ordered():
    """Five counting decodes on two alternating output buffers (bench.py's steps), pipelined (each
    call's exact re-decode overlaps the next call) and stream ordered: the buffers' final contents
    (calls 4 and 5) and the counters accumulated over all five are equal; the last batch is tie
    heavy (rounded rows), so many of its frames are deferred."""
    info = ac.info_set(128, 64)
    B, nb = B_AWGN, 5
    res = {}
    for pipe in (True, False):
        dec = _native.Decoder(128, info, 8, POLY)
        dec.set_pipelined(pipe)
        with _native.DeviceArena(dec) as mem:
            d_llr = [mem.alloc(B * 128 * 8) for _ in range(nb)]
            d_msg = [mem.alloc(B * 8) for _ in range(nb)]
            d_out = [(mem.alloc(B * 8), mem.alloc(B)) for _ in range(2)]
            d_cnt = mem.alloc(64)
            mem.memset(d_cnt, 0, 64)
            for i in range(nb):
                dec.channel_device(11, 30 + i, 1.5 + 0.5 * i, 0.5, 40, i * B, B, d_llr[i], d_msg[i])
            llr = mem.download(d_llr[nb - 1], B * 128 * 8, np.float64).reshape(B, 128)
            mem.upload(d_llr[nb - 1], np.round(llr / 4.0))
            for i in range(nb):
                dec.decode_device(d_llr[i], B, d_best=d_out[i % 2][0], d_flags=d_out[i % 2][1], d_ref=d_msg[i],
                                  k_payload=40, d_counters=d_cnt)
            res[pipe] = ([(mem.download(b, B * 8, np.uint64), mem.download(f, B, np.uint8)) for b, f in d_out],
                         mem.download(d_cnt, 64, np.int64))
            assert dec.screening_count() > 0
        dec.close()
    for i in range(2):
        np.testing.assert_array_equal(res[True][0][i][0], res[False][0][i][0], err_msg=f"best, buffer {i}")
        np.testing.assert_array_equal(res[True][0][i][1], res[False][0][i][1], err_msg=f"flags, buffer {i}")
    np.testing.assert_array_equal(res[True][1], res[False][1], err_msg="counters")
    assert res[True][1][0] == nb * B
