"""CPU: the fact the lane kernel's transformed u0 rests on (scl128_lane.hip, PSCL_LANE_U0T).

After phase 63 the plain lane-per-path kernels keep the first decided word as its Arikan transform
(the form the recomputes at phases 64..112 read) and the epilogue applies the transform once more
to get the decided bits back.  That is right because the transform is an involution; and the in-word
stage form the kernels use (x ^= (x >> s) & M_s, scl_device.h polar_transform64) is the Python
mirror _polar_transform on the word's 64 bits."""
import numpy as np

from polar_code_amd.polar.polar import _polar_transform


def _transform64_words(x):
    """The kernels' in-word form on uint64 arrays."""
    x = x.copy()
    for s, m in ((1, 0x5555555555555555), (2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F),
                 (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF), (32, 0x00000000FFFFFFFF)):
        x ^= (x >> np.uint64(s)) & np.uint64(m)
    return x


def test_transform_twice_is_identity():
    rng = np.random.default_rng(4164)
    w = rng.integers(0, 2**64, size=4096, dtype=np.uint64)
    w[:4] = (0, 1, 2**63, 2**64 - 1)
    bits = ((w[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.int8)
    once = _polar_transform(bits)
    assert np.any(once != bits)
    np.testing.assert_array_equal(_polar_transform(once), bits)
    # the word form the kernel applies at phase 64 and again in the epilogue is that mirror
    tw = _transform64_words(w)
    packed = (once.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    np.testing.assert_array_equal(tw, packed)
    np.testing.assert_array_equal(_transform64_words(tw), w)
