"""bench.py --dump-outputs on CPU: the files dump_outputs writes for a step's output buffers
(packed best words + flag bytes, as pscl_decode_device leaves them) -- float arrays, the same
fixed sample of a large batch every time, under the 64 MB bound."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def _step(B, K, seed):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=(B, K), dtype=np.uint64)
    W = (K + 63) // 64
    words = np.zeros((B, W), np.uint64)
    for j in range(K):
        words[:, j >> 6] |= bits[:, j] << np.uint64(j & 63)
    ok, idx = rng.integers(0, 2, size=B).astype(bool), rng.integers(0, 8, size=B)
    flags = (np.where(ok, 0x80, 0) | idx).astype(np.uint8)
    r = {"last": {"best": words, "flags": flags}, "K": K, "retries": 0,
         "c": np.arange(8, dtype=np.int64) * 1000, "cdl": np.zeros(8, np.int64)}
    return r, bits, ok, idx


def _load(d):
    return {p.stem: np.load(p) for p in sorted(Path(d).glob("*.npy"))}


def test_small_batch_dumped_whole(tmp_path):
    r, bits, ok, idx = _step(1000, 64, 1)
    bench.dump_outputs(str(tmp_path / "a"), r)
    out = _load(tmp_path / "a")
    assert set(out) == {"frame_index", "best_bits", "crc_pass", "best_idx", "counters"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert np.array_equal(out["frame_index"], np.arange(1000))
    assert np.array_equal(out["best_bits"], bits)
    assert np.array_equal(out["crc_pass"], ok)
    assert np.array_equal(out["best_idx"], idx)
    assert np.array_equal(out["counters"], r["c"])


def test_large_batch_fixed_sample_within_bound(tmp_path):
    B, K = bench.DUMP_MAX_FRAMES + 12345, 88  # (K = 88: the widest workload, NR config 5)
    r, bits, ok, idx = _step(B, K, 2)
    bench.dump_outputs(str(tmp_path / "a"), r)
    bench.dump_outputs(str(tmp_path / "b"), r)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    sel = a["frame_index"].astype(np.int64)
    assert sel.size == bench.DUMP_MAX_FRAMES and np.all(np.diff(sel) > 0) and sel[-1] < B
    assert np.array_equal(a["best_bits"], bits[sel]) and np.array_equal(a["best_idx"], idx[sel])
    assert np.array_equal(a["crc_pass"], ok[sel])
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= 64 * 10**6
