"""Pin the C oracle (oracle/scl_oracle.c) to the reference's own outputs.

The golden .npz files were produced by running the reference (tests/golden/make_golden.py);
every assertion is bit-exact (integers, bits, and fp64 metrics/LLRs compared by value).
"""
import numpy as np
import pytest

import oracle

DECODE_SETS = ["g4_decode.npz", "g6_forced.npz", "g10_n16.npz", "g10_n32.npz", "g10_n64_nocrc.npz",
               "g10_k88.npz", "g10_m16.npz", "g10_n8.npz", "g10_n4.npz", "g10_n2.npz",
               "g14_n256.npz", "g14_n256_forced.npz", "g14_n512.npz", "g14_n1024.npz"]


def test_info_sets(golden):
    g = golden("g1_info_sets.npz")
    for key in g.files:
        _, N, K = key.split("_")
        np.testing.assert_array_equal(oracle.construct_info_set(int(N), int(K)), g[key], err_msg=key)


def test_crc(golden):
    g = golden("g2_crc.npz")
    for p, a in zip(g["payload"], g["attached"]):
        np.testing.assert_array_equal(oracle.attach_crc(p, "0x1864CFB"), a)
    for p, a in zip(g["payload8"], g["attached8_0x17"]):
        np.testing.assert_array_equal(oracle.attach_crc(p, "0x17"), a)
    assert all(oracle.check_crc(a, "0x1864CFB") == bool(c) for a, c in zip(g["attached"], g["check_ok"]))
    assert all(oracle.check_crc(a, "0x1864CFB") == bool(c) for a, c in zip(g["corrupted"], g["check_bad"]))
    assert all(oracle.check_crc(a, "0x1864CFB") == bool(c) for a, c in zip(g["random64"], g["check_random"]))
    with pytest.raises(ValueError):
        oracle.check_crc(np.zeros(24, np.int8), "0x1864CFB")


def test_encode(golden):
    g = golden("g3_encode.npz")
    info = oracle.construct_info_set(128, 64)
    for m, c in zip(g["msg"], g["code"]):
        u = np.zeros(128, np.int8)
        u[info] = m
        np.testing.assert_array_equal(oracle.polar_transform(u), c)
    for u, x in zip(g["u"], g["transform"]):
        np.testing.assert_array_equal(oracle.polar_transform(u), x)


def _check_decode_set(g, M, key, crc):
    info = g["info"]
    for f in range(g[key + "_llr"].shape[0]):
        force = g[key + "_force"][f] if key + "_force" in g.files else None
        if force is not None and np.all(force == -1):
            force = None
        n, c, m, il, b = oracle.decode_scl(g[key + "_llr"][f], info, M, crc=crc, force=force)
        assert n == g[key + "_npaths"][f], (key, f)
        np.testing.assert_array_equal(c[:n], g[key + "_cands"][f][:n], err_msg=f"{key} frame {f}")
        np.testing.assert_array_equal(m[:n], g[key + "_metrics"][f][:n], err_msg=f"{key} frame {f}")
        np.testing.assert_array_equal(il[:n], g[key + "_info_llrs"][f][:n], err_msg=f"{key} frame {f}")
        assert b == g[key + "_best"][f], (key, f)


@pytest.mark.parametrize("name", DECODE_SETS)
def test_decode_scl(golden, name):
    g = golden(name)
    crc = str(g["crc"]) or None
    for key in g["keys"]:
        key = str(key)
        M = int(key.split("_")[0][1:])
        _check_decode_set(g, M, key, crc)


def test_decode_ties(golden):
    g = golden("g5_ties.npz")
    for key in g["keys"]:
        key = str(key)
        M = int(key.split("_M")[1])
        _check_decode_set(g, M, key, "0x1864CFB")


def test_sc_decode(golden):
    g = golden("g9_sc.npz")
    for llr, bits in zip(g["llr"], g["bits"]):
        np.testing.assert_array_equal(oracle.sc_decode(llr, g["info"]), bits)


def test_sc_decode_n256(golden):
    g = golden("g14_sc256.npz")
    for llr, bits in zip(g["llr"], g["bits"]):
        np.testing.assert_array_equal(oracle.sc_decode(llr, g["info"]), bits)


def test_decode_with_retries(golden):
    g = golden("g7_flip.npz")
    for tag, beta in (("beta", g["beta"]), ("none", None)):
        mism = 0
        for f, llr in enumerate(g["llr"]):
            r = oracle.decode_with_retries(llr, g["info"], 4, 8, crc="0x1864CFB", beta=beta)
            exp_tried = [int(t) for t in g[f"{tag}_tried"][f] if t >= 0]
            same = (r["tried"] == exp_tried and r["attempts"] == g[f"{tag}_attempts"][f]
                    and r["success"] == bool(g[f"{tag}_success"][f])
                    and np.array_equal(r["bits"], g[f"{tag}_bits"][f]))
            mism += not same
        # flip ranking ties (argsort kind / BLAS summation order) are not pinned: see DESIGN.md
        assert mism == 0, f"{tag}: {mism} frames differ"


def test_decode_with_retries_short_and_odd_shapes():
    """g16: N < 128, K = N, short CRCs, retries >= K and the N = 128 codes with K != 64, beta random
    fp32 and None.  The generator keeps no frame whose flip choice is within 1e-9 relative of
    another untried candidate, so every frame is held exactly (bits, success, attempts, tried)."""
    from dl_short_cases import g16, g16_beta

    g = g16()  # (g16_dl_short.npz, unpacked per case)
    assert len(g["cases"]) == 9
    for tag in g["cases"]:
        info, crc, M, retries = g[f"{tag}_info"], g[f"{tag}_crc"], g[f"{tag}_M"], g[f"{tag}_retries"]
        for name, beta in (("beta", g16_beta(tag)), ("none", None)):
            assert g[f"{tag}_{name}_tried"].shape[1] == retries
            for f, llr in enumerate(g[f"{tag}_llr"]):
                r = oracle.decode_with_retries(llr, info, M, retries, crc=crc, beta=beta)
                assert r["tried"] == [int(t) for t in g[f"{tag}_{name}_tried"][f] if t >= 0], (tag, name, f)
                assert r["attempts"] == g[f"{tag}_{name}_attempts"][f], (tag, name, f)
                assert r["success"] == bool(g[f"{tag}_{name}_success"][f]), (tag, name, f)
                np.testing.assert_array_equal(r["bits"], g[f"{tag}_{name}_bits"][f], err_msg=f"{tag} {name} {f}")


def test_decode_scl_other_crcs_and_unconstructed_info_sets():
    """g17: the (128,64) set under CRCs of degree 1, 6, 11, 16, 24, 32 and none at M = 8; the
    information-set family of offcode_cases.py (position 0, without N - 1, K = N, 16-position blocks,
    K = log2 M and K < log2 M) at N = 32, 128, M = 4, 8 and three of its sets at N = 256.  Path
    count, every candidate, metric and decision LLR (as integer views) and the best index."""
    import offcode_cases as oc

    g = oc.g17()
    assert [t for t, *_ in oc.g17_cases()] == list(g) and len(g) == 7 + 2 * 2 * 11 + 3
    short = 0
    for tag, c in g.items():
        for f, llr in enumerate(c["llr"]):
            n, cands, m, il, b = oracle.decode_scl(llr, c["info"], c["L"], crc=c["crc"])
            assert n == c["npaths"][f], (tag, f)
            assert n == oc.expected_paths(len(c["info"]), c["L"]), (tag, f)
            short += n < c["L"]
            np.testing.assert_array_equal(cands[:n], c["cands"][f], err_msg=f"{tag} frame {f}")
            np.testing.assert_array_equal(m[:n].view(np.int64), c["metrics"][f].view(np.int64), err_msg=f"{tag} frame {f}")
            np.testing.assert_array_equal(np.ascontiguousarray(il[:n]).view(np.int64), c["info_llrs"][f].view(np.int64),
                                          err_msg=f"{tag} frame {f}")
            assert b == c["best"][f], (tag, f)
    assert short >= 20  # (first_only, last_only, short and fills_last below its list size)


def test_batch_matches_single(golden):
    g = golden("g4_decode.npz")
    llr = g["M8_snr3_llr"]
    bits, ok = oracle.decode_batch(llr, g["info"], 8, "0x1864CFB")
    for f in range(llr.shape[0]):
        b = g["M8_snr3_best"][f]
        np.testing.assert_array_equal(bits[f], g["M8_snr3_cands"][f][b])
        assert ok[f] == oracle.check_crc(bits[f], "0x1864CFB")
