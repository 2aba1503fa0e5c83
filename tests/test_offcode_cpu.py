"""CPU: the host decoder and the host encoder off the project's CRC and off constructed information
sets (offcode_cases.py), against the oracle and the host mirrors of the NR front end -- and, on the
oracle alone, the conditions the GPU tier (test_gpu_offcode.py) relies on: that the DL-SCL batches
retry and succeed, that both adaptive stages are populated, that the short sets leave the list
unfilled.  No GPU."""
import numpy as np
import pytest

import adaptive_cases as ac
import offcode_cases as oc
from encode_cases import crc_degree, expected, info_set, pack, payloads, unpack
from polar_code_amd import _native

# (N, K with the CRC, E): k_payload under the degree-32 polynomial is 32 (the remainder wholly in
# word 0, ending at bit 63), 56 (across words 0 / 1, also rate matched) and 108 (across two lanes
# of the long kernel)
ENCODE_CODES = [(128, 64, 0), (128, 88, 0), (128, 88, 201), (256, 140, 0)]


@pytest.mark.parametrize("crc", oc.CRCS, ids=oc.crc_id)
@pytest.mark.parametrize("code", list(oc.CODES))
def test_cpu_decoder_on_the_compiled_in_sets_under_every_crc(code, crc):
    K, _ = oc.CODES[code]
    x = oc.crc_rows(code, crc)[2]
    info = ac.info_set(128, K)
    out = _native.CpuDecoder(128, info, 8, crc).decode(x[oc.FULL])
    oc.assert_full(out, oc.crc_full(code, crc), f"{code} {oc.crc_id(crc)}")
    for L in (1, 2, 4, 8):
        exp = oc.crc_plain(code, crc, L)
        got = _native.CpuDecoder(128, info, L, crc).decode(x, want_metrics=False, want_cands=False, want_info_llrs=False)
        for k in ("best_bits", "crc_pass", "best_idx"):
            np.testing.assert_array_equal(got[k], exp[k], err_msg=f"{code} {oc.crc_id(crc)} L={L}: {k}")
        assert np.all(got["n_paths"] == L)
        if crc is None:
            assert got["crc_pass"].all() and not got["best_idx"].any()


@pytest.mark.parametrize("N,L", oc.FULL_SHAPES)
def test_cpu_decoder_on_the_information_set_family(N, L):
    for name in oc.family_names(N, L):
        c = oc.family_case(N, name, L)
        out = _native.CpuDecoder(N, c["info"], L, c["crc"]).decode(c["rows"])
        oc.assert_full(out, c["exp"], f"N={N} L={L} {name}")
        np.testing.assert_array_equal(out["crc_pass"], c["crc_pass"], err_msg=f"N={N} L={L} {name}: crc_pass")


@pytest.mark.parametrize("crc", oc.NONEMPTY)
@pytest.mark.parametrize("N,K,E", ENCODE_CODES)
def test_encode_cpu_places_every_remainder(N, K, E, crc):
    bits = payloads(N, K, crc, 65, seed=17)
    bits[0], bits[1] = 0, 1
    want_msg, want_tx = expected(N, K, crc, E, bits)
    msg, code = _native.encode_cpu(N, info_set(N, K), crc, pack(bits), E)
    assert bits.shape[1] == K - crc_degree(crc)
    np.testing.assert_array_equal(unpack(msg, K), want_msg)
    np.testing.assert_array_equal(unpack(code, E or N), want_tx)
    if K & 63:
        assert not np.any(msg[:, -1] >> np.uint64(K & 63))


def test_encode_cases_reach_the_remainder_placements():
    kp = [K - 32 for _, K, _ in ENCODE_CODES]
    assert kp == [32, 56, 56, 108]  # ends at bit 63; straddles words 0 / 1; two lanes of the long kernel


# ---- what the GPU tier relies on, from the oracle alone

@pytest.mark.parametrize("with_beta", [False, True], ids=["none", "beta_M8"])
@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("crc", oc.NONEMPTY)
def test_dl_batches_retry_and_succeed(crc, L, with_beta):
    exp = oc.dl_case(crc, L, with_beta)
    retried, first = int((exp["attempts"] > 1).sum()), int((exp["success"] & (exp["attempts"] == 1)).sum())
    print(f"{crc} L={L}: {retried} retried, {first} pass at the first attempt, {int((~exp['success']).sum())} still failing")
    assert retried >= 30 and first >= 30
    np.testing.assert_array_equal(exp["attempts"] > 1, ~exp["base_pass"])


@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("crc", oc.NONEMPTY)
@pytest.mark.parametrize("code", list(oc.CODES))
def test_adaptive_cases_populate_both_stages(code, crc, L):
    exp = oc.crc_adaptive(code, crc, L)
    n1, n2 = int((exp["stage"] == 1).sum()), int((exp["stage"] == 2).sum())
    print(f"{code} {crc} L={L}: stage 1 {n1}, stage 2 {n2}")
    assert n1 >= 20 and n2 >= 20 and exp["n_escalated"] == n2


@pytest.mark.parametrize("N", [32, 128, 256, 512, 1024])
def test_family_sets_are_what_they_are_named(N):
    for L in (4, 8, 16, 32):
        fam = oc.info_family(N, L)
        k = L.bit_length() - 1
        assert fam["fills_last"].size == k and fam["fills_last"][0] == 0 and fam["fills_last"][-1] == N - 1
        assert fam["short"].size == k - 1
        assert fam["all"].size == N and fam["head"][-1] == N // 2 - 1 and fam["tail"][0] == N // 2
        assert 0 in fam["random"] and N - 1 not in fam["random"] and 0 in fam["blocks"] and N - 1 not in fam["blocks"]
        assert set(fam["blocks"] // 16) == set(range(0, N // 16, 2)) and fam["blocks"].size == N // 2
    for L in (1, 2, 3):
        assert "short" not in oc.info_family(N, L) and "fills_last" not in oc.info_family(N, L)


@pytest.mark.parametrize("N,L", [(N, L) for N in (32, 128, 256) for L in (4, 8, 16, 32)] + [(512, 8), (1024, 8)])
def test_short_sets_leave_the_list_unfilled(N, L):
    """short: L / 2 paths on every frame; fills_last: L, reached only at the last phase."""
    for name, want in (("short", L // 2), ("fills_last", L), ("first_only", 2), ("last_only", 2)):
        n = oc.family_case(N, name, L)["exp"]["n_paths"]
        assert np.all(n == want), (N, L, name, n)
