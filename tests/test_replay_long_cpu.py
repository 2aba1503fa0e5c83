"""The host decision-LLR replay (pscl_path_llrs_cpu, csrc/scl_cpu.cpp) on a GPU-less host: held to the
reference's recorded info_llrs of every candidate of every golden that has them, to pscl_decode_cpu's
info_llrs on generated rows, and -- for bits on no list -- to a NumPy restatement of the reference's
f/g recursion.  Every comparison is on bit patterns.  No test here touches a GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle
from polar_code_amd import _native
from polar_code_amd.train import make_dataset as md

import adaptive_cases as ac
import replay_long_cases as rc


@pytest.mark.parametrize("name", rc.GOLDEN_SETS)
def test_reference_goldens_every_candidate(golden, name):
    g = golden(name)
    llr, bits, want = rc.golden_paths(g)
    dec = _native.CpuDecoder(llr.shape[1], g["info"], 1, None, threads=2)
    rc.bits_eq(dec.path_llrs(llr, bits), want, name)


@pytest.mark.parametrize("kind", rc.KINDS)
@pytest.mark.parametrize("shape", rc.SHAPES, ids=rc.shape_id)
def test_equals_the_cpu_decoders_info_llrs(shape, kind):
    N, K, L, crc = shape
    llr = rc.rows(N, K, crc, kind, 6)
    dec = _native.CpuDecoder(N, ac.info_set(N, K), L, crc, threads=2)
    out = dec.decode(llr)
    assert out["n_paths"].max() == min(L, 2 ** K)  # (the lists fill: every candidate slot is compared)
    for p in range(L):
        has = out["n_paths"] > p
        rc.bits_eq(dec.path_llrs(llr[has], out["cands"][has, p]), out["info_llrs"][has, p], f"{shape} {kind} cand {p}")


def test_bits_on_no_list_equal_the_numpy_recursion():
    N, K = 1024, 512
    info = ac.info_set(N, K)
    llr = rc.rows(N, K, ac.POLY24, "awgn", 6)[:3]
    bits = np.random.default_rng(5).integers(0, 2, size=(3, K)).astype(np.int8)
    got = _native.CpuDecoder(N, info, 1, None).path_llrs(llr, bits)
    for b in range(3):
        rc.bits_eq(got[b], rc.numpy_replay(llr[b], info, bits[b]), f"frame {b}")


def test_argument_errors():
    lib = _native.lib()
    info = np.ascontiguousarray(ac.info_set(256, 128), np.int32)
    ip = info.ctypes.data_as(C.POINTER(C.c_int32))
    llr, bits, out = np.zeros((2, 256)), np.zeros((2, 128), np.int8), np.zeros((2, 128))

    def call(N=256, info_p=ip, K=128, l=llr.ctypes.data, B=2, b=bits.ctypes.data, o=out.ctypes.data):
        return lib.pscl_path_llrs_cpu(N, info_p, K, l, B, b, o, 1)

    assert call() == _native.PSCL_OK
    assert call(l=None) == call(b=None) == call(o=None) == call(info_p=None) == _native.PSCL_EINVAL
    assert call(N=96) == call(N=2048) == call(B=-1) == _native.PSCL_EINVAL
    assert call(B=0) == call(B=0, l=None, b=None, o=None) == _native.PSCL_OK
    bad = bits.copy()
    bad[1, 5] = 2
    assert call(b=bad.ctypes.data) == _native.PSCL_EINVAL


def test_cpu_decoder_and_label_batch_equal_the_oracle():
    """CpuDecoder.path_llrs and make_dataset.label_batch at (256,128) on the CPU decoder, against the
    oracle's own decode: no monkeypatch of best_path_llrs."""
    N, K, M, crc = 256, 128, 4, ac.POLY24
    info = ac.info_set(N, K)
    llr, msgs = ac.make_llr(77, 48, info, crc, 1.0, N=N, with_msg=True)
    # all frames carry frame 0's message by the channel's symmetry, as make_dataset's single `sent`
    u = np.zeros((llr.shape[0], N), np.int8)
    u[:, info] = msgs ^ msgs[:1]
    llr = llr * (1.0 - 2.0 * np.stack([oracle.polar_transform(r) for r in u]))
    sent = msgs[0]
    base, ok, l0 = [], [], []
    for b in range(llr.shape[0]):
        n, c, m, il, best = oracle.decode_scl(llr[b], np.asarray(info, np.int32), M, crc)
        base.append(c[best])
        ok.append(oracle.check_crc(c[best], crc))
        l0.append(il[best])
    base, ok, l0 = np.stack(base).astype(np.int8), np.array(ok, bool), np.stack(l0)
    fail = np.flatnonzero(~ok)
    assert fail.size >= 3  # (1 dB: several of the 48 frames fail the CRC)
    rc.bits_eq(_native.CpuDecoder(N, info, M, crc).path_llrs(llr[fail], base[fail]), l0[fail])
    rc.bits_eq(md.best_path_llrs(llr[fail], info, M, crc, base[fail], device="cpu"), l0[fail])

    def oracle_decode(rows, forced=None):
        bits = np.zeros((rows.shape[0], K), np.int8)
        good = np.zeros(rows.shape[0], bool)
        for b in range(rows.shape[0]):
            n, c, m, il, best = oracle.decode_scl(rows[b], np.asarray(info, np.int32), M, crc,
                                                  None if forced is None else forced[b])
            bits[b] = c[best]
            good[b] = oracle.check_crc(bits[b], crc)
        return bits, good

    # the oracle-labelled result: label_batch's steps with the oracle as decoder and its own L0
    abs_l0 = np.abs(l0[fail].astype(np.float32))
    order = np.stack([np.argsort(r) for r in abs_l0])
    label = np.full(fail.size, -1, np.int32)
    for t in range(8):
        todo = np.flatnonzero(label < 0)
        idx = order[todo, t]
        cand, cpass = oracle_decode(llr[fail[todo]], md._force_prefix_flip(base[fail][todo], idx))
        hit = cpass & np.all(cand == sent[None, :], axis=1)
        label[todo[hit]] = idx[hit]
    keep = label >= 0
    a, lab, nf = md.label_batch(llr, info, M, crc, sent, device="cpu")
    np.testing.assert_array_equal(a.view(np.uint32), abs_l0[keep].view(np.uint32))
    np.testing.assert_array_equal(lab, label[keep])
    assert nf == int(np.count_nonzero(~keep))
