"""Staged de-rate-matching without a GPU: the case table is pinned against the oracle, the three
symbols are declared, exported and bound, arguments are validated before any device call, and a
NumPy model of the pass's index map equals the reference's de-rate-match + de-interleave."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_cases as ac
import rm_staged_cases as rc
from polar_code_amd import _native

HEADER = Path(__file__).resolve().parent.parent / "include" / "polar_scl.h"
SYMBOLS = ("pscl_derate_match_device", "pscl_set_rate_match_staged", "pscl_rm_staged_stats")


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_counts_are_the_oracles(name):
    """A drifting input cannot turn a mixed batch into a one-sided one unnoticed."""
    c, e = rc.BY_NAME[name], rc.expected(name)
    esc = ~e["sc_ok"]
    assert rc.rows_of(name).shape == (c.B, c.E)
    assert e["n_escalated"] == int(esc.sum()) == c.escalated
    assert 0 < c.escalated < c.B
    assert int(np.count_nonzero(~e["list_ok"])) == c.list_fail


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = _native.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), s
        assert s in _native.EXPORTS
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and fn.argtypes, s
    for m in ("set_rate_match_staged", "derate_match_device", "rm_staged_stats"):
        assert callable(getattr(_native.Decoder, m))
    from polar_code_amd.polar.scl import SCLDecoder
    assert callable(SCLDecoder.derate_match_tensor)


def test_abi_version_stays_1():
    assert _native.lib().pscl_abi_version() == 1
    assert re.search(r"#define\s+PSCL_ABI_VERSION\s+1\b", HEADER.read_text())


def test_null_handle_is_a_value_error():
    lib = _native.lib()
    a, b = C.c_int64(), C.c_int64()
    for call in (lambda: lib.pscl_derate_match_device(None, None, 1, None),
                 lambda: lib.pscl_set_rate_match_staged(None, 1),
                 lambda: lib.pscl_rm_staged_stats(None, C.byref(a), C.byref(b), 0)):
        with pytest.raises(ValueError):
            _native.check(call())


@pytest.mark.parametrize("N,E", rc.PAIRS)
def test_index_map_model_equals_the_reference(N, E):
    from polar_code_amd.nr.polar import derate_match_polar, subblock_deinterleave

    assert len(rc.EDGE_PAIRS) == 12 and set(rc.PAIRS) == set(rc.EDGE_PAIRS) | {(c.N, c.E) for c in rc.CASES}
    row =np.arange(E, dtype=np.float64)
    want = subblock_deinterleave(derate_match_polar(row, N), N)
    got = rc.model_pass(row[None], N)[0]
    np.testing.assert_array_equal(got.view(np.uint64), np.asarray(want, np.float64).view(np.uint64))
    # the map itself: i -> rm_src[i] is a permutation, and every received index is read exactly once
    src = rc.model_src(N)
    assert sorted(src.tolist()) == list(range(N))
    np.testing.assert_array_equal(src, np.asarray(subblock_deinterleave(np.arange(N), N)))
    copies = rc.model_copies(N, E)
    used = sorted(i for idx, rem, _ in copies for i in idx + ([rem] if rem >= 0 else []))
    assert used == list(range(min(E, N) if E <= N else E))
    assert all(cnt == len(idx) + (rem >= 0) for idx, rem, cnt in copies if idx)


@pytest.mark.parametrize("N,E", [(32, 101), (1024, 3077), (64, 200), (256, 249)])
def test_model_equals_the_reference_on_special_values(N, E):
    """The model's arithmetic (sum order, 0.0 + s, remainder, one division) on the special rows the
    GPU test feeds the kernel: signed zeros, cancelling pairs, subnormals, large values."""
    rows = rc.special_rows(N, E, 5)
    np.testing.assert_array_equal(rc.model_pass(rows, N).view(np.uint64),
                                  np.ascontiguousarray(ac.internal_rows(rows, N, E)).view(np.uint64))
