"""GPU: staged de-rate-matching -- pscl_derate_match_device (derate.hip) and the staged mode of
pscl_set_rate_match_staged on pscl_sc_device, pscl_adaptive_async_device, pscl_decode_device and
pscl_escalate_device.  The pass equals the reference's de-rate-match + de-interleave bit for bit
(adaptive_cases.internal_rows); with the mode on every output and counter equals the oracle's on
those rows and the mode-off call's, and pscl_rm_staged_stats shows that the staged route ran."""
import numpy as np
import pytest

import adaptive_cases as ac
import rm_staged_cases as rc
import staged_cases as sg
from polar_code_amd import _native

pytestmark = pytest.mark.gpu

NC = _native.PSCL_NCOUNT
PASS, IDX = _native.PSCL_FLAG_CRC_PASS, _native.PSCL_FLAG_IDX_MASK
LONG = tuple(n for n in rc.NAMES if rc.BY_NAME[n].N >= 128)  # the rows whose twin has a screening kernel
SENTINEL = 0x5A


def _bits(words, K):
    j = np.arange(K)
    return ((words[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int8)


def decoder(name, staged=True, L=None):
    c = rc.BY_NAME[name]
    dec = _native.Decoder(c.N, rc.info_of(c), L or c.L, c.crc)
    dec.set_rate_match(c.E)
    dec.set_rate_match_staged(staged)
    return dec


class Outputs:
    """Output buffers of one call on B frames (prefilled with the sentinel) and their unpacked form."""

    def __init__(self, dec, mem, B, ref_bits=None):
        self.dec, self.mem, self.B = dec, mem, B
        W = dec.W
        self.kw = dict(d_best=mem.alloc(max(B * W * 8, 8)), d_flags=mem.alloc(max(B, 8)))
        self.d_stage, self.d_n, self.d_cnt = mem.alloc(max(B, 8)), mem.alloc(8), mem.alloc(8 * NC)
        mem.memset(self.kw["d_best"], SENTINEL, max(B * W * 8, 8))
        mem.memset(self.kw["d_flags"], SENTINEL, max(B, 8))
        mem.memset(self.d_stage, SENTINEL, max(B, 8))
        mem.memset(self.d_n, 0xFF, 8)
        mem.memset(self.d_cnt, 0, 8 * NC)
        self.ref = {}
        if ref_bits is not None:
            d_ref = mem.alloc(B * W * 8)
            mem.upload(d_ref, sg.words(ref_bits))
            self.ref = dict(d_ref=d_ref, d_counters=self.d_cnt)

    def read(self):
        B, W, mem = self.B, self.dec.W, self.mem
        self.dec.sync()
        words = mem.download(self.kw["d_best"], max(B * W * 8, 8), np.uint64)[:B * W].reshape(B, W)
        flags = mem.download(self.kw["d_flags"], max(B, 8), np.uint8)[:B]
        return {"best_bits": _bits(words, self.dec.K), "crc_pass": (flags & PASS) != 0,
                "best_idx": (flags & IDX).astype(np.int32), "stage": mem.download(self.d_stage, max(B, 8), np.uint8)[:B].copy(),
                "n_escalated": int(mem.download(self.d_n, 8, np.int32)[0]), "counters": mem.download(self.d_cnt, 8 * NC, np.int64),
                "words": words.copy(), "flags": flags.copy()}


def upload(mem, rows):
    rows = np.ascontiguousarray(rows, np.float64)
    d = mem.alloc(max(rows.nbytes, 8))
    mem.upload(d, rows)
    return d


def noisy_ref(bits, seed):
    """Reference words a few bits off the expected ones, so that every counter is non-zero."""
    return bits ^ (np.random.default_rng(seed).random(bits.shape) < 0.01).astype(np.int8)


# ---- 1. the pass alone

_PASS_DEC = {}


def pass_decoder(N, E):
    """Any handle of length N (the pass depends on N and E alone)."""
    if N not in _PASS_DEC:
        _PASS_DEC[N] = _native.Decoder(N, np.arange(N // 2, N, dtype=np.int32), 1, None)
    _PASS_DEC[N].set_rate_match(E)
    return _PASS_DEC[N]


def run_pass(dec, mem, d_llr, B, N, rows_alloc):
    """derate_match_device into a sentinel-filled buffer of rows_alloc rows: its uint64 view."""
    d_out = mem.alloc(rows_alloc * N * 8)
    mem.memset(d_out, SENTINEL, rows_alloc * N * 8)
    dec.derate_match_device(d_llr, B, d_out)
    dec.sync()
    return mem.download(d_out, rows_alloc * N * 8, np.uint64).reshape(rows_alloc, N)


@pytest.mark.parametrize("N,E", rc.PAIRS)
def test_pass_equals_the_reference(N, E):
    rows = rc.pass_rows(N, E)
    B = len(rows)
    assert B == (67 if N == 1024 else 131)
    want = np.ascontiguousarray(ac.internal_rows(rows, N, E), np.float64).view(np.uint64)
    sentinel = np.uint64(int.from_bytes(bytes([SENTINEL]) * 8, "little"))
    dec = pass_decoder(N, E)
    with _native.DeviceArena(dec) as mem:
        d_llr = upload(mem, rows)
        np.testing.assert_array_equal(run_pass(dec, mem, d_llr, B, N, B), want, err_msg=f"N={N} E={E}")
        # a prefix call leaves the rest of the buffer alone, a one-row call too
        for Bp in (B - 37, 1):
            got = run_pass(dec, mem, d_llr, Bp, N, B)
            np.testing.assert_array_equal(got[:Bp], want[:Bp], err_msg=f"N={N} E={E} B'={Bp}")
            assert np.all(got[Bp:] == sentinel), f"N={N} E={E} B'={Bp}: rows past B' were written"
        if E % 2:  # rows 8 bytes into their allocation: every second row is not 16-byte aligned either way
            d_off = mem.alloc(rows.nbytes + 8) + 8
            mem.upload(d_off, rows)
            np.testing.assert_array_equal(run_pass(dec, mem, d_off, B, N, B), want, err_msg=f"N={N} E={E} +8 bytes")
        dec.derate_match_device(0, 0, 0)  # B = 0 is fine
    assert dec.rm_staged_stats() == {"passes": 0, "rows": 0}  # (the call of its own is not one of the mode's)


def test_pass_needs_real_division_at_3N_plus_5():
    N, E = 32, 3 * 32 + 5
    cnt = [c for _, _, c in rc.model_copies(N, E)]
    assert sorted(set(cnt)) == [3, 4]
    rows = rc.pass_rows(N, E)
    third = ac.internal_rows(rows, N, E)[:, rc.model_src(N) >= 5]
    assert np.count_nonzero(third * 3.0 != np.round(third * 3.0)) > 100  # (quotients that are not exact)


def test_pass_argument_errors():
    dec = _native.Decoder(256, sg.pw_info_set(256, 128), 8, ac.POLY24)
    with pytest.raises(ValueError):  # no rate matching
        dec.derate_match_device(8, 1, 8)
    dec.set_rate_match(300)
    with pytest.raises(ValueError):
        dec.derate_match_device(8, -1, 8)
    with pytest.raises(ValueError):
        dec.derate_match_device(0, 1, 8)
    with pytest.raises(ValueError):
        dec.derate_match_device(8, 1, 0)
    with pytest.raises(NotImplementedError):
        dec.derate_match_device(8, 2 ** 31, 8)


# ---- 2. the SC stage

@pytest.mark.parametrize("name", [n for n in rc.NAMES if rc.BY_NAME[n].N != 128])
def test_sc_stage(name):
    c, exp, rows = rc.BY_NAME[name], rc.expected(name), rc.rows_of(name)
    x = ac.internal_rows(rows, c.N, c.E)
    bits, ok = sg.sc_expected(x, rc.info_of(c), c.crc)
    kp = c.K - 8
    ref = noisy_ref(bits, 31)
    dec = decoder(name)
    with _native.DeviceArena(dec) as mem:
        o = Outputs(dec, mem, c.B, ref)
        dec.sc_device(upload(mem, rows), c.B, d_stage=o.d_stage, k_payload=kp, **o.kw, **o.ref)
        out = o.read()
    np.testing.assert_array_equal(out["best_bits"], bits, err_msg=name)
    np.testing.assert_array_equal(out["crc_pass"], ok, err_msg=name)
    np.testing.assert_array_equal(out["best_idx"], 0, err_msg=name)
    np.testing.assert_array_equal(out["stage"], np.where(ok, 1, 2), err_msg=name)
    np.testing.assert_array_equal(out["counters"], sg.host_counts(bits, ok, ref, kp, NC), err_msg=name)
    assert int(np.count_nonzero(~ok)) == c.escalated == exp["n_escalated"]
    assert dec.rm_staged_stats() == {"passes": 1, "rows": c.B}
    host_bits, host_ok = dec.decode_sc(rows)  # (the host form over the same call)
    np.testing.assert_array_equal(host_bits, bits)
    np.testing.assert_array_equal(host_ok, ok)


# ---- 3. the adaptive call

def run_adaptive(dec, rows, ref_bits=None, kp=0):
    with _native.DeviceArena(dec) as mem:
        o = Outputs(dec, mem, len(rows), ref_bits)
        dec.adaptive_async_device(upload(mem, rows), len(rows), d_stage=o.d_stage, d_n_escalated=o.d_n, k_payload=kp,
                                  **o.kw, **o.ref)
        return o.read()


@pytest.mark.parametrize("name", rc.NAMES)
def test_adaptive(name):
    c, exp, rows = rc.BY_NAME[name], rc.expected(name), rc.rows_of(name)
    kp = c.K - 8
    ref = noisy_ref(exp["list_bits"], 32)
    dec = decoder(name)
    out = run_adaptive(dec, rows, ref, kp)
    ac.assert_equals(out, exp, name)
    assert out["n_escalated"] == exp["n_escalated"] == c.escalated
    np.testing.assert_array_equal(out["counters"], sg.host_counts(exp["best_bits"], exp["crc_pass"], ref, kp, NC,
                                                                  escalated=c.escalated), err_msg=name)
    st = dec.adaptive_stats()
    if c.N >= 128:  # (every such row has L >= 4: the twin's stage 2 is a row-list screening kernel)
        assert c.L >= 4 and st == {"screened": 1, "exact": 0, "host_waits": st["host_waits"]}, (name, st)
    else:
        assert st["screened"] == 0 and st["exact"] == 1, (name, st)
    assert dec.rm_staged_stats() == {"passes": 1, "rows": c.B}
    # a second call of the same size allocates nothing (no host wait), and counts one more pass
    dec.adaptive_stats(reset=True)
    ac.assert_equals(run_adaptive(dec, rows), exp, f"{name} again")
    assert dec.adaptive_stats()["host_waits"] == 0
    assert dec.rm_staged_stats(reset=True) == {"passes": 2, "rows": 2 * c.B}
    assert dec.rm_staged_stats() == {"passes": 0, "rows": 0}


@pytest.mark.parametrize("name", ["n256_E300", "n128_E389"])
@pytest.mark.parametrize("depth", [1, 2])
def test_adaptive_pipelined_equals_stream_ordered(depth, name):
    """Five calls on two alternating output sets: batches 0, 2, 4 are the case's rows, 1 and 3 their
    reversal, so consecutive calls (and the two parities of the staged rows) hold different data."""
    c, exp, rows = rc.BY_NAME[name], rc.expected(name), rc.rows_of(name)
    rev = {k: exp[k][::-1] for k in ("best_bits", "crc_pass", "best_idx", "stage")}
    dec = decoder(name)
    plain = run_adaptive(dec, rows)  # the stream-ordered run (and the oracle)
    ac.assert_equals(plain, exp, name)
    got = []
    with _native.DeviceArena(dec) as mem:
        d_rows = [upload(mem, rows), upload(mem, rows[::-1])]
        sets = [Outputs(dec, mem, c.B), Outputs(dec, mem, c.B)]
        dec.set_pipelined(True, depth=depth)
        try:
            for i in range(5):
                o = sets[i & 1]
                dec.adaptive_async_device(d_rows[i & 1], c.B, d_stage=o.d_stage, d_n_escalated=o.d_n, **o.kw)
            dec.join()
            got = [sets[1].read(), sets[0].read()]  # (an output set is written again two calls later: calls 3 and 4)
        finally:
            dec.set_pipelined(False)
    ac.assert_equals(got[0], rev, f"{name} depth {depth} call 3")
    ac.assert_equals(got[1], exp, f"{name} depth {depth} call 4")
    np.testing.assert_array_equal(got[1]["words"], plain["words"])
    np.testing.assert_array_equal(got[1]["flags"], plain["flags"])
    assert got[0]["n_escalated"] == got[1]["n_escalated"] == c.escalated
    assert dec.rm_staged_stats() == {"passes": 6, "rows": 6 * c.B}


# ---- 4. the plain decode

def run_decode(dec, rows, ref_bits=None, kp=0):
    with _native.DeviceArena(dec) as mem:
        o = Outputs(dec, mem, len(rows), ref_bits)
        dec.decode_device(upload(mem, rows), len(rows), k_payload=kp, **o.kw, **o.ref)
        out = o.read()
    out["deferred"] = dec.screening_count()
    return out


def assert_list(out, want, tag):
    for k in ("best_bits", "crc_pass", "best_idx"):
        np.testing.assert_array_equal(out[k], want[k], err_msg=f"{tag}: {k}")


@pytest.mark.parametrize("name", LONG)
def test_plain_decode_on_and_off(name):
    c, rows, want = rc.BY_NAME[name], rc.rows_of(name), rc.list_expected(name)
    kp = c.K - 8
    ref = noisy_ref(want["best_bits"], 33)
    on, off = decoder(name, True), decoder(name, False)
    a, b = run_decode(on, rows, ref, kp), run_decode(off, rows, ref, kp)
    assert_list(a, want, f"{name} staged")
    assert_list(b, want, f"{name} unstaged")
    np.testing.assert_array_equal(a["words"], b["words"])
    np.testing.assert_array_equal(a["flags"], b["flags"])
    np.testing.assert_array_equal(a["counters"], b["counters"])
    np.testing.assert_array_equal(a["counters"], sg.host_counts(want["best_bits"], want["crc_pass"], ref, kp, NC))
    assert on.rm_staged_stats() == {"passes": 1, "rows": c.B}
    assert off.rm_staged_stats() == {"passes": 0, "rows": 0}
    assert b["deferred"] == 0  # (the mode-off handle has no screening kernel: nothing is deferred)


@pytest.mark.parametrize("name", ["n256_E300", "n128_E100"])
def test_plain_decode_defers_ties_to_the_right_rows(name):
    """40 integer rows: exact final-metric ties, which the screening kernel must hand to the exact
    re-decode -- that reads the caller's rate-matched rows, not the staged ones."""
    import oracle

    c = rc.BY_NAME[name]
    rows = rc.tie_rows(c.E, 4242 + c.N)
    info = rc.info_of(c)
    lb, lok, lidx = oracle.decode_batch(ac.internal_rows(rows, c.N, c.E), info, c.L, crc=c.crc, want_idx=True)
    on = decoder(name, True)
    out = run_decode(on, rows)
    assert_list(out, {"best_bits": lb, "crc_pass": lok, "best_idx": lidx}, f"{name} ties")
    assert out["deferred"] > 0, name
    assert on.rm_staged_stats() == {"passes": 1, "rows": 40}


def test_plain_decode_pipelined():
    """Depth 2, four calls on two alternating output sets and one staged-row buffer."""
    name = "n256_E300"
    c, rows, want = rc.BY_NAME[name], rc.rows_of(name), rc.list_expected(name)
    rev = {k: v[::-1] for k, v in want.items()}
    dec = decoder(name)
    with _native.DeviceArena(dec) as mem:
        d_rows = [upload(mem, rows), upload(mem, rows[::-1])]
        sets = [Outputs(dec, mem, c.B), Outputs(dec, mem, c.B)]
        dec.set_pipelined(True, depth=2)
        try:
            for i in range(4):
                dec.decode_device(d_rows[i & 1], c.B, **sets[i & 1].kw)
            dec.join()
            a, b = sets[0].read(), sets[1].read()
        finally:
            dec.set_pipelined(False)
    assert_list(a, want, "pipelined call 2")
    assert_list(b, rev, "pipelined call 3")
    assert dec.rm_staged_stats() == {"passes": 4, "rows": 4 * c.B}


# ---- 5. the escalation

def test_escalate_after_sc():
    name = "n512_E600"
    c, exp, rows = rc.BY_NAME[name], rc.expected(name), rc.rows_of(name)
    dec = decoder(name)
    with _native.DeviceArena(dec) as mem:
        o = Outputs(dec, mem, c.B)
        d_llr = upload(mem, rows)
        dec.sc_device(d_llr, c.B, d_stage=o.d_stage, **o.kw)
        n = dec.escalate_device(d_llr, c.B, d_stage=o.d_stage, **o.kw)
        out = o.read()
    ac.assert_equals(out, exp, name)
    assert n == c.escalated
    # (the SC stage's pass over B rows, then the dense batch's over the escalated ones)
    assert dec.rm_staged_stats() == {"passes": 2, "rows": c.B + c.escalated}
    host = dec.decode_staged(rows)
    ac.assert_equals(host, exp, f"{name}: decode_staged")


# ---- 6. the edges of the mode

def test_mode_without_rate_matching_changes_nothing():
    case = sg.mixed_case("pw256", 8)
    dec = _native.Decoder(case["N"], case["info"], 8, case["crc"])
    dec.set_rate_match_staged(True)  # (before any pscl_set_rate_match: no effect while rm_E is 0)
    ac.assert_equals(run_adaptive(dec, case["rows"]), case["exp"], "plain rows, mode on")
    out = run_decode(dec, case["rows"])
    assert_list(out, {"best_bits": case["exp"]["list_bits"], "crc_pass": case["exp"]["list_ok"],
                      "best_idx": case["exp"]["list_idx"]}, "plain rows, mode on")
    assert dec.rm_staged_stats() == {"passes": 0, "rows": 0}


def test_switching_the_mode_between_calls():
    name = "n256_E300"
    c, exp, rows, want = rc.BY_NAME[name], rc.expected(name), rc.rows_of(name), rc.list_expected(name)
    dec = _native.Decoder(c.N, rc.info_of(c), c.L, c.crc)
    dec.set_rate_match_staged(True)  # the setter before pscl_set_rate_match
    dec.set_rate_match(c.E)
    outs = []
    for on in (True, False, True):
        dec.set_rate_match_staged(on)
        outs.append(run_decode(dec, rows))
        assert_list(outs[-1], want, f"mode {on}")
    np.testing.assert_array_equal(outs[0]["words"], outs[1]["words"])
    np.testing.assert_array_equal(outs[0]["flags"], outs[2]["flags"])
    assert dec.rm_staged_stats() == {"passes": 2, "rows": 2 * c.B}
    ac.assert_equals(run_adaptive(dec, rows), exp, "adaptive after the switches")
    dec.set_rate_match_staged(False)
    with pytest.raises(NotImplementedError):  # mode off: today's refusal
        run_adaptive(dec, rows)
    dec.set_rate_match(0)
    dec.set_rate_match_staged(True)
    x = ac.internal_rows(rows, c.N, c.E)
    assert_list(run_decode(dec, x), want, "plain rows after rate matching was switched off")


def test_compiled_nr_code_keeps_its_own_kernels():
    """A staged (128,88) E = 256 handle at L = 8 has rate-matched screening kernels of its own."""
    rows, exp = ac.nr_case()
    rows, B = rows[:515], 515
    dec = _native.Decoder(128, ac.info_set(128, 88), 8, ac.POLY24)
    dec.set_rate_match(256)
    dec.set_rate_match_staged(True)
    out = run_decode(dec, rows)
    assert_list(out, {"best_bits": exp["list_bits"][:B], "crc_pass": exp["list_ok"][:B], "best_idx": exp["list_idx"][:B]}, "NR")
    ac.assert_equals(run_adaptive(dec, rows), exp, "NR adaptive", slice(0, B))
    assert dec.adaptive_stats()["screened"] == 1
    assert dec.rm_staged_stats() == {"passes": 0, "rows": 0}


def test_calls_outside_the_mode_behave_as_unstaged():
    """The _f32 and DL-SCL calls on a staged N = 256 handle: the same refusals, the same results."""
    name = "n256_E300"
    c, rows = rc.BY_NAME[name], rc.rows_of(name)[:67]
    res = []
    for staged in (True, False):
        dec = decoder(name, staged)
        with _native.DeviceArena(dec) as mem:
            d32 = mem.alloc(rows.size * 4)
            mem.upload(d32, rows.astype(np.float32))
            o = Outputs(dec, mem, 67)
            assert not dec.f32_available()
            with pytest.raises(NotImplementedError):
                dec.decode_device_f32(d32, 67, **o.kw)
            with pytest.raises(NotImplementedError):
                dec.sc_device_f32(d32, 67, **o.kw)
            with pytest.raises(NotImplementedError):
                dec.adaptive_async_device_f32(d32, 67, **o.kw)
            with pytest.raises(NotImplementedError):
                dec.adaptive_dlscl_device(upload(mem, rows), 67, 4, tried_stride=4, **o.kw)
            d_att = mem.alloc(67 * 4)
            dec.dlscl_device(upload(mem, rows), 67, 4, d_attempts=d_att, **o.kw)
            out = o.read()
            res.append((out["words"], out["flags"], mem.download(d_att, 67 * 4, np.int32)))
        assert dec.rm_staged_stats() == {"passes": 0, "rows": 0}
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    assert np.any(res[0][2] > 1)  # (some frame entered a retry chain)


def test_tensor_methods_on_a_side_stream():
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    name = "n256_E300"
    c, exp, rows = rc.BY_NAME[name], rc.expected(name), rc.rows_of(name)
    dec = SCLDecoder(c.N, rc.info_of(c), c.L, c.crc)
    dec.native.set_rate_match(c.E)
    dec.native.set_rate_match_staged(True)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        llr = torch.from_numpy(rows.copy()).to("cuda")
        x = dec.derate_match_tensor(llr)
        best, flags, stage, n_esc = dec.decode_tensor_adaptive_async(llr)
        sbest, sflags, sstage = dec.decode_tensor_sc(llr)
        tbest, tflags, tstage = dec.decode_tensor_staged(llr)
    stream.synchronize()
    assert x.shape == (c.B, c.N) and x.dtype == torch.float64
    np.testing.assert_array_equal(x.cpu().numpy().view(np.uint64),
                                  np.ascontiguousarray(ac.internal_rows(rows, c.N, c.E)).view(np.uint64))
    for b, f, s in ((best, flags, stage), (tbest, tflags, tstage)):
        f = f.cpu().numpy()
        np.testing.assert_array_equal(b.cpu().numpy().view(np.uint64), sg.words(exp["best_bits"]))
        np.testing.assert_array_equal((f & PASS) != 0, exp["crc_pass"])
        np.testing.assert_array_equal(f & IDX, exp["best_idx"])
        np.testing.assert_array_equal(s.cpu().numpy(), exp["stage"])
    assert int(n_esc.cpu()[0]) == c.escalated
    np.testing.assert_array_equal(sbest.cpu().numpy().view(np.uint64), sg.words(exp["sc_bits"]))
    np.testing.assert_array_equal((sflags.cpu().numpy() & PASS) != 0, exp["sc_ok"])
    np.testing.assert_array_equal(sstage.cpu().numpy(), np.where(exp["sc_ok"], 1, 2))
    with pytest.raises(ValueError):
        dec.derate_match_tensor(llr.float())
    with pytest.raises(ValueError):
        SCLDecoder(c.N, rc.info_of(c), c.L, c.crc).derate_match_tensor(llr)  # no rate matching
