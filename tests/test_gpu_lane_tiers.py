"""GPU: the one-swap and ranked tiers of the lane-per-path screening decode (scl128_lane.hip: self-sourced
pulls, the survivor-count certificate from the lane masks, the fused rank counts) against the oracle on
every frame -- best bits, CRC flag, best index.

Instances: L = 4 and 8, the (128,64) code and the NR (128,88) code at E = 256, float64 and float32 rows,
the plain call (decode_device / decode_device_f32) and the row-list call (stage 2 of
adaptive_async_device / _f32, which decodes the frames whose SC result fails the CRC).  Batches of 1,
8 F - 3 and 8 F + 5 frames (F = 64 / L frames per wavefront): the last wavefront has empty frame slots.
Rows (lane_tier_cases.py): AWGN at 1 and 3 dB, where nearly every full-list phase is ranked, and at 5 dB;
and crafted rows whose first full-list phase has a chosen number d = 0 .. L / 2 of surviving worse
children (read from the oracle before anything is sent to the GPU), laid out so that one wavefront holds
d = 0, 1 and >= 2 together, another d = 0 and 1 only, another d = L / 2 throughout.

At most 2 % of a case's frames may be deferred to the exact kernel (the handle's deferred count), so no
case passes on the exact kernel alone."""
import numpy as np
import pytest

import adaptive_cases as ac
import lane_tier_cases as tc
import oracle
from polar_code_amd import _native

pytestmark = pytest.mark.gpu
KINDS = tuple(f"awgn {e:g} dB" for e in tc.EBNOS) + ("crafted d",)


def _words(bits):
    B, K = bits.shape
    w = np.zeros((B, (K + 63) // 64), np.uint64)
    for j in range(K):
        w[:, j >> 6] |= bits[:, j].astype(np.uint64) << np.uint64(j & 63)
    return w


@pytest.fixture(scope="module", params=list(tc.CONFIGS))
def cfg(request):
    K, L, E = tc.CONFIGS[request.param]
    dec = _native.Decoder(128, ac.info_set(128, K), L, tc.POLY)
    if E:
        dec.set_rate_match(E)
    assert dec.f32_available()
    yield request.param, dec
    dec.close()


def _decode(dec, rows, B, f32, rowlist):
    """One call on the first B rows: (best words, flags, deferred count, escalated count or None)."""
    W = dec.W
    x = np.ascontiguousarray(rows[:B] if f32 else rows[:B].astype(np.float64))
    with _native.DeviceArena(dec) as mem:
        d_llr, d_best, d_flags, d_n = mem.alloc(x.nbytes), mem.alloc(B * W * 8), mem.alloc(max(B, 8)), mem.alloc(8)
        mem.upload(d_llr, x)
        mem.memset(d_flags, 0x55, max(B, 8))
        mem.memset(d_n, 0, 8)
        if rowlist:
            call = dec.adaptive_async_device_f32 if f32 else dec.adaptive_async_device
            call(d_llr, B, d_best=d_best, d_flags=d_flags, d_n_escalated=d_n)
        else:
            (dec.decode_device_f32 if f32 else dec.decode_device)(d_llr, B, d_best=d_best, d_flags=d_flags)
        dec.sync()
        deferred = dec.screening_count()
        return (mem.download(d_best, B * W * 8, np.uint64).reshape(B, W), mem.download(d_flags, max(B, 8), np.uint8)[:B],
                deferred, int(mem.download(d_n, 8, np.int32)[0]) if rowlist else None)


@pytest.mark.parametrize("rowlist", [False, True], ids=["plain", "rowlist"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_tiers_every_frame(cfg, f32, rowlist):
    name, dec = cfg
    K, L, E = tc.CONFIGS[name]
    rows, _, want = tc.case(name)
    exp = tc.expected(name)
    assert set(np.unique(want)) == set(range(L // 2 + 1))
    for kind in KINDS:
        e = exp[kind]
        bits, ok, idx = (e["best_bits"], e["crc_pass"], e["best_idx"]) if rowlist else (e["list_bits"], e["list_ok"], e["list_idx"])
        for B in tc.batch_sizes(L):
            best, flags, deferred, n_esc = _decode(dec, rows[kind], B, f32, rowlist)
            tag = f"{name}, {'f32' if f32 else 'f64'}, {'row list' if rowlist else 'plain'}, {kind}, B = {B}"
            decoded = int(np.count_nonzero(e["stage"][:B] == 2)) if rowlist else B  # frames the list kernel decodes
            print(f"{tag}: {decoded} list decodes, {deferred} deferred, {np.count_nonzero(~ok[:B])} CRC failures, "
                  f"{np.count_nonzero(ok[:B] & (idx[:B] > 0))} passes at index > 0")
            np.testing.assert_array_equal(best, _words(bits[:B]), err_msg=f"{tag}: best bits")
            np.testing.assert_array_equal((flags & 0x80) != 0, ok[:B], err_msg=f"{tag}: CRC flag")
            np.testing.assert_array_equal(flags & 0x3F, idx[:B], err_msg=f"{tag}: best index")
            if rowlist:
                assert n_esc == decoded, tag
                if B > 1 and kind != "awgn 5 dB":
                    assert decoded > B // 2, f"{tag}: the row-list kernel decoded {decoded} frames only"
            assert deferred <= 0.02 * B, f"{tag}: {deferred} of {B} frames deferred"


def test_pipelined_five_calls_two_buffers_equal_stream_ordered():
    """The crafted and the 1 dB rows of the headline instance, and a tie batch (small integers: the
    deferral path), as five consecutive counting decodes on two alternating output buffers -- the
    deferred count is non-zero in some calls and zero in others -- on a pipelined handle and on a
    stream-ordered one: final buffers, counters and every call's deferred count are equal, and the
    outputs equal the oracle's."""
    name = "p64-L8"
    K, L, E = tc.CONFIGS[name]
    rows, _, _ = tc.case(name)
    exp = tc.expected(name)
    B = tc.batch_sizes(L)[-1]
    rng = np.random.default_rng(99)
    ties = rng.integers(-2, 3, size=(B, 128)).astype(np.float64)
    tb, tok, tidx = oracle.decode_batch(ties, ac.info_set(128, K), L, crc=tc.POLY, want_idx=True)
    seq = [("crafted d", rows["crafted d"].astype(np.float64)), ("ties", ties), ("awgn 5 dB", rows["awgn 5 dB"].astype(np.float64)),
           ("ties", ties), ("awgn 1 dB", rows["awgn 1 dB"].astype(np.float64))]
    ref = np.zeros((B, 1), np.uint64)
    res = {}
    for pipe in (True, False):
        dec = _native.Decoder(128, ac.info_set(128, K), L, tc.POLY)
        dec.set_pipelined(pipe)
        with _native.DeviceArena(dec) as mem:
            d_llr = [mem.alloc(B * 128 * 8) for _ in seq]
            d_ref = mem.alloc(B * 8)
            d_out = [(mem.alloc(B * 8), mem.alloc(B)) for _ in range(2)]
            d_cnt = mem.alloc(64)
            mem.memset(d_cnt, 0, 64)
            mem.upload(d_ref, ref)
            for d, (_, x) in zip(d_llr, seq):
                mem.upload(d, np.ascontiguousarray(x))
            deferred = []
            for i in range(len(seq)):
                dec.decode_device(d_llr[i], B, d_best=d_out[i % 2][0], d_flags=d_out[i % 2][1], d_ref=d_ref, k_payload=K - 24,
                                  d_counters=d_cnt)
                deferred.append(dec.screening_count())
            dec.sync()
            res[pipe] = ([(mem.download(b, B * 8, np.uint64).reshape(B, 1), mem.download(f, B, np.uint8)) for b, f in d_out],
                         mem.download(d_cnt, 64, np.int64), deferred)
        dec.close()
    print("deferred per call (pipelined, stream ordered):", res[True][2], res[False][2])
    assert res[True][2] == res[False][2]
    d = res[False][2]
    assert d[1] > B // 2 and d[3] > B // 2, d  # the tie batches: deferral is the point
    assert d[0] <= 0.02 * B and d[2] <= 0.02 * B and d[4] <= 0.02 * B, d
    assert min(d) == 0, d
    for i in range(2):
        np.testing.assert_array_equal(res[True][0][i][0], res[False][0][i][0], err_msg=f"best, buffer {i}")
        np.testing.assert_array_equal(res[True][0][i][1], res[False][0][i][1], err_msg=f"flags, buffer {i}")
    np.testing.assert_array_equal(res[True][1], res[False][1], err_msg="counters")
    assert res[True][1][0] == len(seq) * B
    # final buffers: call 5 (1 dB rows) in buffer 0, call 4 (ties) in buffer 1
    e = exp["awgn 1 dB"]
    for (best, flags), (bits, ok, idx) in zip(res[True][0], ((e["list_bits"], e["list_ok"], e["list_idx"]), (tb, tok, tidx))):
        np.testing.assert_array_equal(best, _words(bits))
        np.testing.assert_array_equal((flags & 0x80) != 0, ok)
        np.testing.assert_array_equal(flags & 0x3F, idx)
