"""CPU tier of the near-tie fixture (near_tie_cases.py): what makes its rows worth decoding on the GPU,
pinned on the reference side alone, and the product's host decoder on the same rows.

The un-margined model (oracle.decode_batch_f32tail: the oracle's source with the screening kernels' fp32
metric tail, no margin, nothing deferred) must be WRONG on a large share of the INSIDE and float32 rows --
so a screening kernel that dropped its margin would be too -- and right on every AWGN row those were made
from, which is why AWGN batches cannot show such a kernel.  Conditions (the issue's; the smallest measured
shares were 20 % INSIDE and 9.7 % float32 on its B = 400 .. 1000 batches):

    INSIDE, every case      the model differs from the oracle on >= 10 % of the frames and on >= 8 frames
    float32 class           on >= 5 % of the frames
    AWGN, N = 128 and 256   on no frame
    DL-SCL cases            >= 25 % of the frames take a retry (oracle.decode_with_retries)

Measured on this case table (frames differing of B; AWGN 0 everywhere, N = 512 and 1024 included):
INSIDE 18 .. 49 of 131 at N = 128, 30 .. 68 of 131 at N = 256 (16 on the E = 300 rows), 54 .. 58 of 67 at
N = 512, 62 .. 66 of 67 at N = 1024; float32 10 .. 20 of 131; 57 .. 69 % of the DL-SCL frames retry."""
import numpy as np
import pytest

import near_tie_cases as nt
from polar_code_amd import _native

ALL = nt.NAMES + (nt.RM256.name,)
F32 = tuple(c.name for c in nt.CASES if c.group == "compiled" and c.L in (4, 8))
DL = ("n128k64_L4", "n128k64_L8")


@pytest.mark.parametrize("name", ALL)
def test_model_is_wrong_inside_the_margin(name):
    d = nt.model_differs(name, "inside")
    print(f"{name}: INSIDE {int(d.sum())} of {d.size} frames differ, STRADDLE "
          f"{int(nt.model_differs(name, 'straddle').sum())}")
    assert d.sum() >= 8 and d.mean() >= 0.10, (name, int(d.sum()), d.size)


@pytest.mark.parametrize("name", F32)
def test_model_is_wrong_on_float32_rows(name):
    rows = nt.rows_of(name, "f32")
    assert rows.dtype == np.float32
    d = nt.model_differs(name, "f32")
    print(f"{name}: float32 {int(d.sum())} of {d.size} frames differ")
    assert d.mean() >= 0.05, (name, int(d.sum()), d.size)


@pytest.mark.parametrize("name", [n for n in ALL if nt.case(n).N <= 256])
def test_model_is_right_on_awgn_rows(name):
    assert int(nt.model_differs(name, "awgn").sum()) == 0, name


@pytest.mark.parametrize("with_beta", [False, True], ids=["none", "beta"])
@pytest.mark.parametrize("name", DL)
def test_dl_cases_take_retries(name, with_beta):
    exp = nt.dl_expected(name, with_beta)
    share = float((exp["attempts"] > 1).mean())
    print(f"{name} beta={with_beta}: {share:.1%} of {len(exp['attempts'])} frames retried")
    assert share >= 0.25, (name, share)


def test_rows_are_what_they_claim():
    """Perturbations of the stated sizes on integer bases; rate-matched bases stay dyadic inside."""
    for name in ("n128k64_L8", "n128k88e256_L8", nt.RM256.name):
        c = nt.case(name)
        base = nt.base_rows(c.N, c.K, c.B, c.ebno, c.seed, c.E)
        assert np.array_equal(base, np.round(base)) and base.shape == (c.B, c.E or c.N)
        for cls, ds in (("inside", nt.INSIDE), ("straddle", nt.STRADDLE)):
            dev = np.abs(nt.rows_of(name, cls) - base).max(axis=1)
            d = nt.class_d(ds, c.B)
            assert np.all(dev < 6.0 * d) and np.all(dev > 0.5 * d), (name, cls)
        x = nt.ac.internal_rows(base, c.N, c.E)
        assert np.array_equal(2.0 * x, np.round(2.0 * x)), name  # (means of one or two integers)
    assert nt.case("n512k256_L4").B == 67 and nt.case("n256k128_L32").B == 131


@pytest.mark.parametrize("cls", ["inside", "straddle"])
@pytest.mark.parametrize("name", [n for n in ALL if nt.case(n).N <= 256])
def test_cpu_decoder_equals_oracle(name, cls):
    """pscl_decode_cpu on every near-tie batch at N <= 256: path counts, candidates in list order, fp64
    metrics, decision LLRs, best index, best bits and CRC flag, bit for bit."""
    c = nt.case(name)
    n, cands, mets, illr, best = nt.full_expected(name, cls)
    exp = nt.expected(name, cls)
    out = _native.CpuDecoder(c.N, nt.info_of(c), c.L, nt.POLY, threads=2).decode(nt.internal(name, cls))
    np.testing.assert_array_equal(out["n_paths"], n)
    assert np.all(n == c.L)  # (every list is full: all L entries are compared)
    np.testing.assert_array_equal(out["cands"], cands)
    np.testing.assert_array_equal(out["metrics"].view(np.int64), mets.view(np.int64))
    np.testing.assert_array_equal(out["info_llrs"].view(np.int64), illr.view(np.int64))
    np.testing.assert_array_equal(out["best_idx"], best)
    for k in ("best_bits", "crc_pass", "best_idx", "n_paths"):
        np.testing.assert_array_equal(out[k], exp[k], err_msg=f"{name} {cls}: {k}")
