"""One pipelined handle driven through every scratch family at once: plain decodes, adaptive calls
without a host wait, DL-SCL calls with retries and simulate blocks, interleaved, with the batch size
changed in the middle so that scratch regrows while earlier calls' work is pending.  Every call
writes its own output buffers; every output and counter must equal, bit for bit, the same call made
alone on a fresh unpipelined handle (the decoders are deterministic)."""
import functools

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_dl_cases as dc
import staged_cases as sg
from polar_code_amd import _native

pytestmark = pytest.mark.gpu

NC = _native.PSCL_NCOUNT
RETRIES = 8
# 3 plain decodes, 3 adaptive calls, 5 DL-SCL calls (every compaction parity and both chain sets rotate),
# 5 simulate blocks; the batch size changes after the eighth call
ORDER = ("dl", "dec", "sim", "ad", "dl", "sim", "dec", "dl", "ad", "sim", "dl", "sim", "dec", "ad", "dl", "sim")
assert [ORDER.count(k) for k in ("dec", "ad", "dl", "sim")] == [3, 3, 5, 5]
SWITCH = 8


@functools.lru_cache(maxsize=None)
def case(N, B1):
    """(information set, beta, rows, reference words): B1 -> B2 rows (a 1.5x-grown buffer of B1 rows
    cannot hold B2) plus one row of offset per call.  The SNRs leave the list decoder failing on about a
    third of the N = 128 rows and on 32 of the N = 256 rows, so every DL-SCL call runs retry chains."""
    B2 = B1 * 5 // 3
    if N == 128:
        info, beta, ebno = ac.info_set(128, 64), dc.golden_beta(8), 3.0
    else:
        info, beta, ebno = sg.pw_info_set(N, N // 2), None, 1.5
    rows, msg = ac.make_llr(4200 + N, B2 + len(ORDER), info, ac.POLY24, ebno, N=N, with_msg=True)
    return info, beta, rows, sg.words(msg), B2


class Call:
    """The buffers of one call of the sequence: call i reads the rows from row i on."""

    def __init__(self, mem, kind, i, B, N, W, d_rows, d_refs):
        self.kind, self.i, self.B, self.W = kind, i, B, W
        self.mem = mem
        self.llr, self.ref = d_rows + i * N * 8, d_refs + i * W * 8
        self.sizes = {"best": B * W * 8, "flags": B, "stage": B, "att": B * 4, "tried": B * RETRIES * 4, "n": 8,
                      "cnt": 3 * NC * 8}
        self.p = {k: mem.alloc(n) for k, n in self.sizes.items()}
        for k, n in self.sizes.items():
            mem.memset(self.p[k], 0 if k == "cnt" else 0x5A, n)

    def issue(self, dec, beta, kp):
        p, B = self.p, self.B
        if self.kind == "dec":
            dec.decode_device(self.llr, B, d_best=p["best"], d_flags=p["flags"], d_ref=self.ref, k_payload=kp,
                              d_counters=p["cnt"])
        elif self.kind == "ad":
            dec.adaptive_async_device(self.llr, B, d_best=p["best"], d_flags=p["flags"], d_stage=p["stage"], d_ref=self.ref,
                                      k_payload=kp, d_counters=p["cnt"], d_n_escalated=p["n"])
        elif self.kind == "dl":
            dec.dlscl_device(self.llr, B, RETRIES, beta=beta, d_best=p["best"], d_flags=p["flags"], d_attempts=p["att"],
                             d_tried=p["tried"], tried_stride=RETRIES, d_ref=self.ref, k_payload=kp,
                             d_counters_scl=p["cnt"], d_counters_dl=p["cnt"] + NC * 8)
        else:
            dec.simulate_device(77, 5, 3.0, dec.K / dec.N, kp, 100000 * self.i, B, RETRIES, True, p["cnt"])

    def read(self):
        dt = {"best": np.uint64, "att": np.int32, "tried": np.int32, "n": np.int32, "cnt": np.int64}
        return {k: self.mem.download(self.p[k], n, dt.get(k, np.uint8)).copy() for k, n in self.sizes.items()}


def run(dec, mem, calls, beta, d_rows, d_refs):
    """Buffers first (an allocation or a copy through the handle joins its pending work), then the
    calls back to back, then one join."""
    N, W, kp = dec.N, dec.W, dec.K - dec.crc_deg
    cs = [Call(mem, kind, i, B, N, W, d_rows, d_refs) for kind, i, B in calls]
    dec.set_beta(beta)
    for c in cs:
        c.issue(dec, beta, kp)
    dec.join()
    dec.sync()
    return [c.read() for c in cs]


@pytest.mark.parametrize("N,L,B1", [(128, 8, 3000), (256, 4, 300)])
def test_interleaved_calls_equal_each_alone(N, L, B1):
    info, beta, rows, refs, B2 = case(N, B1)
    calls = [(kind, i, B1 if i < SWITCH else B2) for i, kind in enumerate(ORDER)]
    dec = _native.Decoder(N, info, L, ac.POLY24)
    dec.set_pipelined(True)
    with _native.DeviceArena(dec) as mem:
        d_rows, d_refs = mem.alloc(rows.nbytes), mem.alloc(refs.nbytes)
        mem.upload(d_rows, rows)
        mem.upload(d_refs, refs)
        got = run(dec, mem, calls, beta, d_rows, d_refs)
        retried = 0
        for call, g in zip(calls, got):
            alone = _native.Decoder(N, info, L, ac.POLY24)
            with _native.DeviceArena(alone) as m2:
                r_rows, r_refs = m2.alloc(rows.nbytes), m2.alloc(refs.nbytes)
                m2.upload(r_rows, rows)
                m2.upload(r_refs, refs)
                (want,) = run(alone, m2, [call], beta, r_rows, r_refs)
            alone.close()
            for k in want:
                np.testing.assert_array_equal(g[k], want[k], err_msg=f"N={N} call {call}: {k}")
            if call[0] == "dl":
                retried += int(np.count_nonzero(want["att"] > 1))
        assert retried > 0, "no frame entered a retry chain: the case exercises nothing"
    dec.close()
