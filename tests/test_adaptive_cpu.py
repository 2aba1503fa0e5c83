"""Adaptive decoding on the host (pscl_decode_adaptive_cpu, CpuDecoder.decode_adaptive): SC first,
the list decoder only where the SC result fails the CRC.  The result is the composition of the
oracle's sc_decode + check_crc and decode_batch, bit for bit (adaptive_cases.compose).  Also the
code-object check of the device stage's SC kernel (no scratch, no spills).  No GPU needed."""
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
from polar_code_amd import _native

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "polar_code_amd" / "libpolar_mi355x.so"
READELF = Path("/opt/rocm/lib/llvm/bin/llvm-readelf")


def _cpu(L, threads=0, N=128, K=64, crc=ac.POLY24):
    return _native.CpuDecoder(N, ac.info_set(N, K), L, crc, threads=threads)


@pytest.mark.parametrize("L", [8, 4])
def test_cpu_mixed_batch_equals_composition(L):
    exp = ac.mixed_expected(L)
    assert 0.15 * 4099 < exp["n_escalated"] < 0.5 * 4099
    out = _cpu(L).decode_adaptive(ac.mixed_rows())
    ac.assert_equals(out, exp, f"cpu mixed L={L}")
    assert out["n_escalated"] == exp["n_escalated"]


def test_cpu_all_pass_and_all_fail():
    rows, exp = ac.allpass_case()
    assert exp["n_escalated"] == 0
    out = _cpu(8).decode_adaptive(rows)
    ac.assert_equals(out, exp, "cpu all-pass")
    assert out["n_escalated"] == 0 and np.all(out["stage"] == 1)
    rows, exp = ac.allfail_case()
    assert exp["n_escalated"] == len(rows)
    out = _cpu(8).decode_adaptive(rows)
    ac.assert_equals(out, exp, "cpu all-fail")
    np.testing.assert_array_equal(out["best_bits"], exp["list_bits"])  # plain L = 8 exactly
    np.testing.assert_array_equal(out["best_idx"], exp["list_idx"])
    assert out["n_escalated"] == len(rows)


def test_cpu_threads_give_identical_output():
    rows = ac.mixed_rows()[:1500]
    a, b = _cpu(8, threads=1).decode_adaptive(rows), _cpu(8, threads=4).decode_adaptive(rows)
    for k in ("best_bits", "crc_pass", "best_idx", "stage"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["n_escalated"] == b["n_escalated"]


def test_cpu_n256():
    info = ac.info_set(256, 128)
    rows = ac.make_llr(79, 300, info, ac.POLY24, 3.0, N=256)
    exp = ac.compose(rows, info, 4, ac.POLY24, N=256)
    assert 0 < exp["n_escalated"] < 300
    out = _cpu(4, N=256, K=128).decode_adaptive(rows)
    ac.assert_equals(out, exp, "cpu N=256")
    assert out["n_escalated"] == exp["n_escalated"]


def test_block_family_enters_every_sc_node_in_every_state(golden):
    """The SC kernel's only branches are its mask tests: 127 nodes, each entered with information
    in both halves, in the right half only or in the left half only.  The block family covers all
    381 pairs; the constructed sets cover no "left only" pair at all (position i + M/2 is never
    less reliable than position i), which is why the family exists."""
    every = ac.all_branch_states()
    assert len(every) == 381
    fam = ac.block_family()
    assert len(fam) == 14 and all(len(s) == 64 and np.all(np.diff(s) > 0) for _, s in fam)
    np.testing.assert_array_equal(dict(fam)["bit6=0"], np.arange(0, 64))
    np.testing.assert_array_equal(dict(fam)["bit6=1"], np.arange(64, 128))
    covered = set().union(*(ac.sc_branch_states(s) for _, s in fam))
    print(f"block family: {len(covered & every)} of {len(every)} (node, state) pairs")
    assert covered == every
    g1 = golden("g1_info_sets.npz")
    built = [s for _, s in ac.edge_family()[:4]] + [ac.info_set(128, K) for K in (40, 64, 88)]
    built += [g1["info_128_64"], g1["info_128_88"]]
    got = set().union(*(ac.sc_branch_states(s) for s in built))
    assert got <= every and not [st for st in got if st[2] and not st[3]]
    assert len(ac.family()) == 19 and len({n for n, _ in ac.family()}) == 19
    assert [len(s) for _, s in ac.edge_family()] == [27, 63, 65, 90, 64]


@pytest.mark.parametrize("name", [n for n, _ in ac.family()])
def test_cpu_every_branch_state(name):
    """The host form on the 19 sets, B = 256, L = 4: the composition on the raw rows, and on the
    shifted rows (the oracle's SC result is a random CRC-valid word on every one) exactly the
    targets from stage 1."""
    case = ac.family_case(name)
    info, B = case["info"], 256
    dec = _native.CpuDecoder(128, info, 4, ac.POLY24)
    out = dec.decode_adaptive(case["raw"][:B])
    ac.assert_equals(out, case["exp"], f"cpu {name} raw", slice(0, B))
    assert out["n_escalated"] == int(np.count_nonzero(~case["exp"]["sc_ok"][:B]))
    out = dec.decode_adaptive(case["shifted"][:B])
    np.testing.assert_array_equal(out["best_bits"], case["t"][:B])
    assert np.all(out["stage"] == 1) and np.all(out["crc_pass"]) and out["n_escalated"] == 0


def _sc_model(llr, mask, S, bad, u):
    """sc_decode in plain Python with the kernel's sub-tree skips; the node in state `bad` =
    (M, S, left, right) is mishandled: its g sees the left partial sums inverted (both halves; right
    only: the skipped half's zeros as ones), or it hands its own sums up inverted (left only)."""
    M = len(llr)
    if M == 1:
        u[S] = int(llr[0] < 0)
        return np.array([u[S]], np.int8)
    h = M // 2
    left, right = bool(mask[S:S + h].any()), bool(mask[S + h:S + M].any())
    hit = bad == (M, S, left, right)
    a, b = llr[:h], llr[h:]
    xl, xr = np.zeros(h, np.int8), np.zeros(h, np.int8)
    if left:
        xl = _sc_model(np.sign(a) * np.sign(b) * np.minimum(np.abs(a), np.abs(b)), mask, S, bad, u)
    if right:
        xs = 1 - xl if hit else xl
        xr = _sc_model(b + (1 - 2 * xs) * a, mask, S + h, bad, u)
    elif hit:
        xl = 1 - xl
    return np.concatenate([xl ^ xr, xr])


def test_shifted_rows_observe_every_branch_state():
    """What the shifted rows can see, on the host: with any one (node, state) pair mishandled, the
    model's bits differ from the targets on some row of a block set that enters the pair.  The
    exceptions are the seven "left only" nodes on the tree's right edge, whose partial sums no g
    ever reads."""
    cases = [ac.family_case(n) for n, _ in ac.block_family()]
    masks = []
    for c in cases:
        m = np.zeros(128, bool)
        m[c["info"]] = True
        masks.append(m)

    def differs(c, mask, bad, r):
        u = np.zeros(128, np.int8)
        _sc_model(c["shifted"][r], mask, 0, bad, u)
        return not np.array_equal(u[c["info"]], c["t"][r])

    assert not any(differs(c, m, None, r) for c, m in zip(cases, masks) for r in range(3))  # the model itself
    blind = [p for p in sorted(ac.all_branch_states())
             if not any(differs(c, m, p, r) for c, m in zip(cases, masks) if p in ac.sc_branch_states(c["info"])
                        for r in range(8))]
    assert blind == [(M, 128 - M, True, False) for M in (2, 4, 8, 16, 32, 64, 128)]


def test_cpu_requires_a_crc():
    dec = _native.CpuDecoder(128, ac.info_set(128, 64), 8, None)
    with pytest.raises(ValueError):
        dec.decode_adaptive(ac.mixed_rows()[:4])


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="needs the built library and llvm-readelf")
def test_sc_kernel_uses_no_scratch_and_does_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hits = {n: v for n, v in mod.kernels(LIB).items() if re.search(r"sc128_lane_kernelILb[01]E", n)}
    assert len(hits) == 2, sorted(hits)  # the plain and the rate-matched instance
    for n, v in hits.items():
        assert v.get("private_segment_fixed_size", 0) == 0, f"{n} uses {v['private_segment_fixed_size']} B of scratch"
        assert v.get("vgpr_spill_count", 0) == 0, f"{n} spills {v['vgpr_spill_count']} VGPRs"
        assert v.get("sgpr_spill_count", 0) == 0, f"{n} spills {v['sgpr_spill_count']} SGPRs"
