"""The long replay kernel (csrc/replay_long.hip; N = 256, 512, 1024) through pscl_path_llrs_device,
SCLDecoder.path_llrs_tensor, make_dataset and the DL-SCL chains under the dl_long_replay knob.  Held
to the reference's recorded info_llrs (the g14 goldens), to the decoder's own history for every
candidate, to the host replay for bits on no list, and -- the knob -- to the history chain's outputs
and counters.  Every comparison is on bit patterns."""
import functools

import numpy as np
import pytest

import oracle
from polar_code_amd import _native
from polar_code_amd.polar.scl import SCLDecoder, _pack_words
from polar_code_amd.train import make_dataset as md

import adaptive_cases as ac
import replay_long_cases as rc

pytestmark = pytest.mark.gpu

WG_FRAMES = 4  # rows one workgroup of the replay kernel takes (one wavefront each)


@pytest.mark.parametrize("name", rc.LONG_GOLDEN_SETS)
def test_reference_goldens_every_candidate(golden, name):
    g = golden(name)
    llr, bits, want = rc.golden_paths(g)
    dec = _native.Decoder(llr.shape[1], g["info"], 1, None)
    rc.bits_eq(dec.path_llrs(llr, bits), want, name)
    assert dec.replay_stats() == {"launches": 1, "rows": llr.shape[0]}


def _all_candidates(dec, rows, out, tag):
    L = out["cands"].shape[1]
    assert out["n_paths"].max() == L  # (the lists fill: every candidate slot is compared)
    for p in range(L):
        has = out["n_paths"] > p
        rc.bits_eq(dec.path_llrs(rows[has], out["cands"][has, p]), out["info_llrs"][has, p], f"{tag} cand {p}")


@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("shape", rc.LONG_SHAPES, ids=rc.shape_id)
def test_equals_the_decoders_history(shape, kind):
    N, K, L, crc = shape
    rows = rc.rows(N, K, crc, kind, 24)
    dec = _native.Decoder(N, ac.info_set(N, K), L, crc)
    _all_candidates(dec, rows, dec.decode(rows), f"{shape} {kind}")


@pytest.mark.parametrize("N,K,E", [(256, 128, 300), (256, 128, 200), (512, 200, 1000), (1024, 512, 1536)])
def test_rate_matched_rows(N, K, E):
    rows = rc.rows(N, K, ac.POLY24, "awgn", 24, E)
    dec = _native.Decoder(N, ac.info_set(N, K), 4, ac.POLY24)
    dec.set_rate_match(E)
    _all_candidates(dec, rows, dec.decode(rows), f"N={N} E={E}")
    q = rc.rows(N, K, ac.POLY24, "quantised", 24, E)  # (exact sums and ties through the front end)
    _all_candidates(dec, q, dec.decode(q), f"N={N} E={E} quantised")


@pytest.mark.parametrize("N,K", [(256, 128), (1024, 512)])
def test_random_bits_equal_the_host_replay(N, K):
    info = ac.info_set(N, K)
    rows = rc.rows(N, K, ac.POLY24, "awgn", 24)
    bits = np.random.default_rng(N).integers(0, 2, size=(24, K)).astype(np.int8)
    rc.bits_eq(_native.Decoder(N, info, 1, None).path_llrs(rows, bits),
               _native.CpuDecoder(N, info, 1, None).path_llrs(rows, bits))


def test_launch_edges():
    N, K = 256, 128
    info = ac.info_set(N, K)
    rows = rc.rows(N, K, ac.POLY24, "awgn", 24)
    bits = np.random.default_rng(3).integers(0, 2, size=(24, K)).astype(np.int8)
    want = _native.CpuDecoder(N, info, 1, None).path_llrs(rows, bits)
    dec = _native.Decoder(N, info, 4, ac.POLY24)
    dec.path_llrs_device(0, 0, 0, 0)  # B = 0: returns at once
    assert dec.replay_stats()["launches"] == 0
    for B in (1, WG_FRAMES - 1, WG_FRAMES, WG_FRAMES + 1):
        rc.bits_eq(dec.path_llrs(rows[:B], bits[:B]), want[:B], f"B = {B}")
    # two calls of different B on one handle: the second sees nothing of the first's scratch
    rc.bits_eq(dec.path_llrs(rows[:9], bits[:9]), want[:9])
    rc.bits_eq(dec.path_llrs(rows[20:22], bits[20:22]), want[20:22])
    assert dec.replay_stats(reset=True) == {"launches": 6, "rows": 1 + 3 + 4 + 5 + 9 + 2}
    assert dec.replay_stats() == {"launches": 0, "rows": 0}


def test_short_codes_keep_their_kernel():
    for N, K, L, crc in ((128, 64, 4, ac.POLY24), (64, 32, 4, ac.POLY24)):
        rows = rc.rows(N, K, crc, "awgn", 24)
        dec = _native.Decoder(N, ac.info_set(N, K), L, crc)
        _all_candidates(dec, rows, dec.decode(rows), f"N = {N}")
        assert dec.replay_stats() == {"launches": 0, "rows": 0}


def test_path_llrs_tensor():
    import torch

    N, K = 256, 128
    info = ac.info_set(N, K)
    rows = rc.rows(N, K, ac.POLY24, "awgn", 24)
    bits = np.random.default_rng(4).integers(0, 2, size=(24, K)).astype(np.int8)
    dec = SCLDecoder(N, info, 4, ac.POLY24)
    want = dec.native.path_llrs(rows, bits)
    words = torch.from_numpy(_pack_words(bits, dec.native.W).view(np.int64)).cuda()
    t64 = torch.from_numpy(np.array(rows)).cuda()
    rc.bits_eq(dec.path_llrs_tensor(t64, words).cpu().numpy(), want, "float64")
    side = torch.cuda.Stream()  # the caller's stream: an external one
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = dec.path_llrs_tensor(t64, words)
    side.synchronize()
    rc.bits_eq(got.cpu().numpy(), want, "external stream")
    t32 = t64.float()
    rc.bits_eq(dec.path_llrs_tensor(t32, words).cpu().numpy(),
               dec.path_llrs_tensor(t32.double(), words).cpu().numpy(), "float32 widened")
    for bad in (t64[:, :-1], t64.half(), t64.t()):
        with pytest.raises(ValueError):
            dec.path_llrs_tensor(bad, words)
    with pytest.raises(ValueError):
        dec.path_llrs_tensor(t64, words[:-1])
    with pytest.raises(ValueError):
        dec.path_llrs_tensor(t64, words.int())
    # N = 128: float32 rows on the native float32 form
    d128 = SCLDecoder(128, ac.info_set(128, 64), 4, ac.POLY24)
    r32 = torch.from_numpy(np.array(rc.rows(128, 64, ac.POLY24, "awgn", 24))).cuda().float()
    b128 = np.random.default_rng(6).integers(0, 2, size=(24, 64)).astype(np.int8)
    w128 = torch.from_numpy(_pack_words(b128, 1).view(np.int64)).cuda()
    out = torch.empty((24, 64), dtype=torch.float64, device="cuda")
    d128.native.path_llrs_device_f32(r32.data_ptr(), 24, w128.data_ptr(), out.data_ptr())
    d128.native.sync()
    rc.bits_eq(d128.path_llrs_tensor(r32, w128).cpu().numpy(), out.cpu().numpy(), "N = 128 float32")


def test_make_dataset_best_path_llrs_equals_the_oracle():
    N, K, M, crc = 256, 128, 4, ac.POLY24
    info = ac.info_set(N, K)
    rows = rc.rows(N, K, crc, "awgn", 24)
    base, l0 = [], []
    for b in range(rows.shape[0]):
        n, c, m, il, best = oracle.decode_scl(rows[b], np.asarray(info, np.int32), M, crc)
        base.append(c[best])
        l0.append(il[best])
    rc.bits_eq(md.best_path_llrs(rows, info, M, crc, np.stack(base).astype(np.int8)), np.stack(l0))


# ---- the knob: the chains on the replay equal the chains on the decoder's history
# (256,128)+CRC-24, B = 2048, 4.0 dB, retries 8, rows of ac.make_llr(9000 + L + E, ..).  Beforehand on
# the CPU (oracle.dl_batch = decode_with_retries per frame; pscl_decode_cpu's failing baselines equal
# the chain entries), beta = None / the fixed random beta:
#   L = 4            823 frames enter a chain, 738 / 823 reach attempts >= 3
#   L = 8            422 enter, 378 / 422 reach attempts >= 3
#   L = 4, E = 300   1580 enter, 1535 / 1578 reach attempts >= 3
# (this code's chains rarely end early, so a lower Eb/N0 only makes nearly every frame fail: at 1.5 dB
# 2025 of 2048 enter)
KNOB_B, KNOB_EBNO, KNOB_RETRIES = 2048, 4.0, 8
KNOB_HANDLES = [(4, 0), (8, 0), (4, 300)]
NC = _native.PSCL_NCOUNT


@functools.lru_cache(maxsize=None)
def _knob_inputs(L, E):
    N, K = 256, 128
    info = ac.info_set(N, K)
    rows, msgs = ac.make_llr(9000 + L + E, KNOB_B, info, ac.POLY24, KNOB_EBNO, N=N, E=E, with_msg=True)
    ref = _pack_words(msgs, 2)
    beta = np.random.default_rng(11).random((K, K)).astype(np.float32)
    return info, rows, ref, beta


class _Bufs:
    """One set of device outputs of a chain call."""

    def __init__(self, mem, dec, B, rounds):
        self.mem, self.B, self.W, self.rounds = mem, B, dec.W, rounds
        self.best, self.flags, self.stage = mem.alloc(B * dec.W * 8), mem.alloc(B), mem.alloc(B)
        self.attempts, self.tried = mem.alloc(B * 4), mem.alloc(B * rounds * 4)
        self.cnt, self.nesc = mem.alloc(3 * NC * 8), mem.alloc(8)
        for p, n in ((self.best, B * dec.W * 8), (self.flags, B), (self.stage, B), (self.attempts, B * 4),
                     (self.tried, B * rounds * 4)):
            mem.memset(p, 0xEE, n)
        mem.memset(self.cnt, 0, 3 * NC * 8)
        mem.memset(self.nesc, 0, 8)

    def read(self):
        m, B = self.mem, self.B
        return {"best": m.download(self.best, B * self.W * 8, np.uint64), "flags": m.download(self.flags, B, np.uint8),
                "stage": m.download(self.stage, B, np.uint8), "attempts": m.download(self.attempts, B * 4, np.int32),
                "tried": m.download(self.tried, B * self.rounds * 4, np.int32),
                "counters": m.download(self.cnt, 3 * NC * 8, np.int64), "n_escalated": m.download(self.nesc, 8, np.int32)}


def _call(dec, which, d_llr, d_ref, o, beta):
    B, kp = o.B, dec.K - 24
    common = dict(beta=beta, d_best=o.best, d_flags=o.flags, d_attempts=o.attempts, d_tried=o.tried,
                  tried_stride=o.rounds, d_ref=d_ref, k_payload=kp)
    if which == "dlscl":
        dec.dlscl_device(d_llr, B, KNOB_RETRIES, d_counters_scl=o.cnt, d_counters_dl=o.cnt + NC * 8, **common)
    elif which == "retry":  # after a plain decode
        dec.decode_device(d_llr, B, d_best=o.best, d_flags=o.flags, d_ref=d_ref, k_payload=kp, d_counters=o.cnt)
        dec.retry_device(d_llr, B, KNOB_RETRIES, d_stage=o.stage, d_counters_dl=o.cnt + NC * 8, **common)
    else:
        dec.adaptive_dlscl_device(d_llr, B, KNOB_RETRIES, d_stage=o.stage, d_counters=o.cnt, d_n_escalated=o.nesc, **common)


def _run(dec, rows, ref, beta, which, pipelined=False):
    """The outputs of the call (pipelined: of two calls on alternating buffers, then join) and the
    replay launches it made."""
    dec.replay_stats(reset=True)
    with _native.DeviceArena(dec) as mem:
        d_llr, d_ref = mem.alloc(rows.nbytes), mem.alloc(ref.nbytes)
        mem.upload(d_llr, rows)
        mem.upload(d_ref, ref)
        sets = [_Bufs(mem, dec, rows.shape[0], KNOB_RETRIES) for _ in range(2 if pipelined else 1)]
        if pipelined:
            dec.set_pipelined(True)
        try:
            for o in sets:
                _call(dec, which, d_llr, d_ref, o, beta)
            dec.join()
            dec.sync()
        finally:
            if pipelined:
                dec.set_pipelined(False)
        return [o.read() for o in sets], dec.replay_stats()["launches"]


def _assert_same(a, b, tag):
    for x, y in zip(a, b):
        for k in x:
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{tag}: {k}")


def _not_vacuous(out, tag):
    att = out["attempts"]
    entered = (att > 1) & (att != np.int32(-286331154))  # (0xEEEEEEEE: never written)
    assert np.count_nonzero(entered) >= 50, tag
    assert np.count_nonzero(entered & (att >= 3)) >= 10, tag
    return int(att[entered].max()) - 1  # rounds run


@pytest.mark.parametrize("use_beta", [False, True], ids=["l0", "beta"])
@pytest.mark.parametrize("L,E", KNOB_HANDLES, ids=["L4", "L8", "L4_E300"])
def test_knob_outputs_equal_the_history_chain(L, E, use_beta):
    info, rows, ref, beta = _knob_inputs(L, E)
    beta = beta if use_beta else None
    dec = _native.Decoder(256, info, L, ac.POLY24)
    if E:
        dec.set_rate_match(E)
    # (pscl_adaptive_dlscl_device refuses rate matching at N = 256: tests/test_gpu_adaptive_dl.py test_errors)
    for which in ("dlscl", "retry") + (() if E else ("adaptive",)):
        dec.set_tuning(dl_long_replay=0)
        base, n0 = _run(dec, rows, ref, beta, which)
        rounds = _not_vacuous(base[0], which)
        assert n0 == 0, which
        dec.set_tuning(dl_long_replay=1)
        got, n1 = _run(dec, rows, ref, beta, which)
        _assert_same(base, got, f"L={L} E={E} {which}")
        assert n1 >= 1 + rounds, (which, n1, rounds)
    dec.close()


@pytest.mark.parametrize("L,E", KNOB_HANDLES, ids=["L4", "L8", "L4_E300"])
def test_knob_on_a_pipelined_handle(L, E):
    info, rows, ref, beta = _knob_inputs(L, E)
    dec = _native.Decoder(256, info, L, ac.POLY24)
    if E:
        dec.set_rate_match(E)
    dec.set_tuning(dl_long_replay=0)
    base, n0 = _run(dec, rows, ref, beta, "dlscl", pipelined=True)
    rounds = _not_vacuous(base[0], "pipelined")
    _assert_same(base[:1], base[1:], "the two pipelined calls")
    assert n0 == 0
    dec.set_tuning(dl_long_replay=1)
    got, n1 = _run(dec, rows, ref, beta, "dlscl", pipelined=True)
    _assert_same(base, got, f"L={L} E={E} pipelined")
    assert n1 >= 2 * (1 + rounds), (n1, rounds)
    dec.close()
