"""CPU: the compile-time partial-sum plan of the plain lane kernels (scl_lane.h psplan_*, scl128_lane.hip
PSCL_LANE_PSPLAN), restated independently in Python for both compiled-in information sets.

At the 56 even phases phi that are not recompute phases (t = phi mod 16 in {2, .., 14}) the first
rewritten depth is a row of w = t & -t g nodes; node k's sign bit is bit k of the in-word Arikan
transform of the window u[phi - w, phi).  The plan replaces it by the parity of the window over S_k =
{i : window bit i is an information bit, (i & k) == k}.  Here: for every such phase and every window
value the frozen pattern allows, that parity against the transform (the kernels' stage form and the
Python mirror _polar_transform); the node and set counts the kernel's instruction saving rests on;
the phases that keep the transform; and that the masks compiled into the kernels are these sets."""
import re
from pathlib import Path

import numpy as np
import pytest

from polar_code_amd.polar.polar import _polar_transform, construct_info_set

CSRC = Path(__file__).resolve().parent.parent / "polar_code_amd" / "csrc"
K_OF_CODE = {1: 64, 2: 88}
PHASES = [phi for phi in range(128) if phi % 16 and phi % 2 == 0]
# distinct non-empty sets per phase, in phase order: a window's sets are {i in I : i contains k}, so
# one information bit (or a window ending in a single one) gives 1, "...I.III" and denser give 8
DISTINCT = {
    1: [0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 4, 0, 1, 1, 0, 1, 0, 2, 0, 1, 1, 0, 1, 1, 8, 1, 4, 1,
        0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 8, 1, 4, 1, 0, 1, 1, 8, 1, 4, 1, 1, 2, 1, 8, 1, 4, 2],
    2: [0, 1, 0, 2, 0, 1, 1, 0, 1, 1, 8, 1, 4, 2, 0, 1, 1, 8, 1, 4, 1, 1, 2, 1, 8, 1, 4, 2,
        0, 1, 1, 8, 1, 4, 1, 1, 2, 1, 8, 1, 4, 2, 1, 2, 1, 8, 1, 4, 2, 1, 4, 2, 8, 2, 4, 2],
}
PLAIN_ADDS = {1: 36, 2: 12}         # nodes with an empty set: b + a, no sign operation
KEEPS_TRANSFORM = {1: [], 2: [120]}  # phases where the plan is not cheaper (window "IIIIIII.")


def _info_bits(code):
    bits = np.zeros(128, bool)
    bits[construct_info_set(128, K_OF_CODE[code])] = True
    return bits


def _window(code, phi):
    t = phi % 16
    w = t & -t
    return w, phi - w, _info_bits(code)[phi - w:phi]


def _sets(code, phi):
    w, _, inf = _window(code, phi)
    return [frozenset(i for i in range(w) if inf[i] and (i & k) == k) for k in range(w)]


def _transform8(x):
    """The kernels' in-word stage form (scl_device.h polar_transform8)."""
    for s, m in ((1, 0x55), (2, 0x33), (4, 0x0F)):
        x ^= (x >> s) & m
    return x


def test_compiled_in_masks_are_the_constructed_sets():
    text = (CSRC / "scl128_impl.h").read_text()
    rows = re.findall(r"\{(0x[0-9a-f]+)ULL,\s*(0x[0-9a-f]+)ULL\}", text[text.index("kSpecInfo[3][2]"):])
    for code in (1, 2):
        lo, hi = (int(v, 16) for v in rows[code - 1])
        bits = np.array([((lo if i < 64 else hi) >> (i & 63)) & 1 for i in range(128)], bool)
        np.testing.assert_array_equal(bits, _info_bits(code), err_msg=f"code {code}")


@pytest.mark.parametrize("code", [1, 2])
def test_sets_give_the_transform_on_every_allowed_window(code):
    assert len(PHASES) == 56
    for phi in PHASES:
        w, lo, inf = _window(code, phi)
        assert lo // 8 == (phi - 1) // 8, "a window lies inside one byte of u"
        sets = _sets(code, phi)
        imask = sum(1 << i for i in range(w) if inf[i])
        for v in range(1 << w):
            if v & ~imask:
                continue  # a frozen bit set: never decoded
            x = _transform8(v)
            bits = np.array([(v >> i) & 1 for i in range(w)], np.int8)
            mirror = _polar_transform(bits[None, :])[0]
            for k in range(w):
                par = sum((v >> i) & 1 for i in sets[k]) & 1
                assert par == (x >> k) & 1 == mirror[k], (code, phi, v, k)


@pytest.mark.parametrize("code", [1, 2])
def test_node_and_set_counts(code):
    plain = nodes = 0
    distinct = []
    for phi in PHASES:
        sets = _sets(code, phi)
        nodes += len(sets)
        distinct.append(len({s for s in sets if s}))
        if phi not in KEEPS_TRANSFORM[code]:
            plain += sum(1 for s in sets if not s)
    assert nodes == 192
    assert plain == PLAIN_ADDS[code]
    assert distinct == DISTINCT[code]
    # node 0's set is every information bit of the window; the last node's is the bit of phase
    # phi - 1 alone, when that is an information bit
    for phi in PHASES:
        w, _, inf = _window(code, phi)
        sets = _sets(code, phi)
        assert sets[0] == frozenset(np.flatnonzero(inf).tolist())
        assert sets[w - 1] == (frozenset([w - 1]) if inf[w - 1] else frozenset())


def _cost_planned(sets, ninfo):
    """Instructions of the planned form as the kernel emits it (scl_lane.h psplan_cost): a shift per
    information bit of the window, an xor per distinct set of two or more bits met while a set's
    mask is built from the mask of the set without its lowest bit, a sign xor per non-empty node."""
    seen, cost = set(), ninfo
    for s in sets:
        cost += 1 if s else 0
        s = sorted(s)
        while len(s) >= 2:
            if tuple(s) not in seen:
                seen.add(tuple(s))
                cost += 1
            s = s[1:]
    return cost


@pytest.mark.parametrize("code", [1, 2])
def test_phases_that_keep_the_transform(code):
    keeps, today, planned = [], 0, 0
    for phi in PHASES:
        w, _, inf = _window(code, phi)
        transform = 2 + 2 * {2: 1, 4: 2, 8: 3}[w] + 2 * w  # extract, stages, shift + xor per node
        plan = _cost_planned(_sets(code, phi), int(inf.sum()))
        if not plan < transform:
            keeps.append(phi)
        today += transform
        planned += min(plan, transform)
    assert keeps == KEEPS_TRANSFORM[code]
    assert today == 672
    # the header proves its own constexpr count (psplan_cost / psplan_planned summed over the phases)
    # against literals in static_asserts, so the build fails if the C++ count moves; the same literals
    # are read here, so this restatement and the header cannot drift apart either
    text = (CSRC / "scl_lane.h").read_text()
    m = re.search(r"static_assert\(psplan_total\(kSpecInfo\[%d\]\[0\], kSpecInfo\[%d\]\[1\]\) == (\d+) && "
                  r"psplan_kept\(kSpecInfo\[%d\]\[0\], kSpecInfo\[%d\]\[1\]\) == (\d+)" % ((code,) * 4), text)
    assert m, "scl_lane.h: the static_assert on the plan's totals"
    assert (planned, len(keeps)) == (int(m.group(1)), int(m.group(2)))
    if code == 2:
        assert "!psplan_planned(psplan_window(kSpecInfo[2][0], kSpecInfo[2][1], 120), 8)" in text
