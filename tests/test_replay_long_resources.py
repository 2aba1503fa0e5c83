"""The long replay kernel's instances, read from the gfx950 code objects' metadata in the built
library (tools/kernel_resources.py; CPU only): the three exist under their names, use no scratch and
spill no register, and every kernel the library held before them
(tests/golden/kernel_names_before_replay_long.txt) is still there.  In the manner of
tests/test_rm_staged_resources.py."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "polar_code_amd" / "libpolar_mi355x.so"
READELF = Path("/opt/rocm/lib/llvm/bin/llvm-readelf")
BEFORE = ROOT / "tests" / "golden" / "kernel_names_before_replay_long.txt"
# replay_long_kernel<R>: R = N / 64 words of bits (N = 256, 512, 1024)
NEW = ("replay_long_kernelILi4EE", "replay_long_kernelILi8EE", "replay_long_kernelILi16EE")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels():
    if not LIB.exists() or not READELF.exists():
        pytest.skip("needs the built library and llvm-readelf")
    return _tool().kernels(LIB)


def _one(kernels, part):
    hits = [(n, v) for n, v in kernels.items() if part in n]
    assert len(hits) == 1, (part, [n for n, _ in hits])
    return hits[0][1]


def test_the_new_unit_holds_these_instances_and_no_other(kernels):
    new = sorted(n for n in kernels if "replay_long" in n)
    assert len(new) == len(NEW), new
    for part in NEW:
        _one(kernels, part)


@pytest.mark.parametrize("part", NEW)
def test_instance_is_clean(part, kernels):
    k = _one(kernels, part)
    assert k.get("private_segment_fixed_size", 0) == 0, (part, "scratch", k)
    assert k.get("vgpr_spill_count", 0) == 0, (part, "spilled VGPRs", k)
    assert k.get("sgpr_spill_count", 0) == 0, (part, "SGPRs parked in VGPR lanes", k)
    assert k.get("group_segment_fixed_size", 0) == 0, (part, "the tree level lives in registers: no LDS", k)
    assert k["vgpr_count"] <= 128, (part, "four wavefronts per SIMD", k)


def test_every_earlier_kernel_is_still_present(kernels):
    before = BEFORE.read_text().split()
    assert len(before) == 181
    missing = [n for n in before if n not in kernels]
    assert not missing, missing
    assert not [n for n in before if "replay_long" in n]
    # the N <= 128 replay keeps its name and its launches
    assert [n for n in before if "replay_kernel" in n and "r32" not in n]
