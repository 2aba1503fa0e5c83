"""The float32 DL-SCL kernel instances, read from the gfx950 code objects' metadata in the built
library (tools/kernel_resources.py; CPU only): every one exists under a name of its own, uses no
scratch, spills no VGPR, parks no more SGPRs in VGPR lanes than its float64 twin, keeps at least its twin's wavefronts per SIMD, and compiles with the IEEE fp32 denormal
mode (the widening conversion follows it: a flushed subnormal LLR would lose its sign).  The float64
twins are still there under their old names.  (The instances are named *_r32, for float32 rows:
test_f32_cpu.py counts the *_f32 kernels of the plain float32 paths, these are counted here.)  In the
manner of tests/test_kernel_resources.py."""
import importlib.util
import struct
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "polar_code_amd" / "libpolar_mi355x.so"
READELF = Path("/opt/rocm/lib/llvm/bin/llvm-readelf")

# (float32 name part, float64 name part) of every instance pair: the post pass (N, K compiled in or
# from the launch; 8 or 4 wavefronts per workgroup; 2 or 4 entries per wavefront), the replay, the
# forced-bit lane-per-path screening decode of the (128,64) code, the exact forced-bit decode of both
# compiled-in codes (CH = rate matched for code 2)
POST = ["ILi0ELi0ELi4ELi2EE", "ILi0ELi0ELi8ELi2EE", "ILi128ELi64ELi4ELi2EE", "ILi128ELi64ELi4ELi4EE", "ILi128ELi64ELi8ELi2EE",
        "ILi128ELi88ELi4ELi2EE", "ILi128ELi88ELi8ELi2EE"]
PAIRS = ([("dl_post_kernel_r32" + a, "dl_post_kernel" + a) for a in POST]
         + [("replay_kernel_r32E", "replay_kernelE")]
         + [(f"scl_lane_fs_kernel_r32ILi{l}ELi1ELb1ELb0ELb0ELb0ELb0EE", f"scl_lane_kernelILi{l}ELi1ELb1ELb0ELb0ELb0ELb0EE") for l in (4, 8)]
         + [(f"scl128_fs_kernel_r32ILi{l}ELb0ELb{c - 1}ELb1ELi{c}ELb0EE", f"scl128_kernelILi{l}ELb0ELb{c - 1}ELb1ELi{c}ELb0EE")
            for l in (4, 8) for c in (1, 2)])


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


def _waves_per_simd(vgprs):
    """Wavefronts per SIMD by VGPR count (512 per lane, allocated in blocks of 8, at most 8 waves)."""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def test_the_new_units_hold_these_instances_and_no_other(kernels):
    new = sorted(n for n in kernels if "_r32" in n)
    assert len(new) == len(PAIRS) == 14, new
    for part, _ in PAIRS:
        _one(kernels, part)


@pytest.mark.parametrize("f32,f64", PAIRS)
def test_instance_is_clean_and_keeps_its_twins_occupancy(f32, f64, kernels):
    a, b = _one(kernels, f32), _one(kernels, f64)
    assert a.get("private_segment_fixed_size", 0) == 0, (f32, "scratch", a)
    assert a.get("vgpr_spill_count", 0) == 0, (f32, "spilled VGPRs", a)
    assert a.get("sgpr_spill_count", 0) <= b.get("sgpr_spill_count", 0), (f32, a, b)
    assert _waves_per_simd(a["vgpr_count"]) >= _waves_per_simd(b["vgpr_count"]), (f32, a["vgpr_count"], b["vgpr_count"])


def _kernel_descriptors(elf):
    """{kernel name: its 64-byte kernel descriptor} of one code object (the <name>.kd symbols)."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in secs:
        if s[1] not in (2, 11):  # SHT_SYMTAB, SHT_DYNSYM
            continue
        strtab = secs[s[6]]
        for k in range(s[5] // 24):
            name_off, _, _, shndx, value, _ = struct.unpack_from("<IBBHQQ", elf, s[4] + 24 * k)
            end = elf.index(b"\0", strtab[4] + name_off)
            name = elf[strtab[4] + name_off:end].decode()
            if name.endswith(".kd") and 0 < shndx < shnum:
                sec = secs[shndx]
                off = sec[4] + value - sec[3]
                out[name[:-3]] = elf[off:off + 64]
    return out


@pytest.mark.skipif(not LIB.exists(), reason="needs the built library")
def test_instances_keep_fp32_denormals():
    """FLOAT_DENORM_MODE_32 (bits 16-17 of compute_pgm_rsrc1, byte 48 of the kernel descriptor) is 3 --
    input and output denormals kept -- in every new instance."""
    kds = {}
    for co in _tool().code_objects(LIB):
        kds.update(_kernel_descriptors(co))
    new = {n: kd for n, kd in kds.items() if "_r32" in n}
    assert len(new) == 14, sorted(new)
    for n, kd in new.items():
        rsrc1, = struct.unpack_from("<I", kd, 48)
        assert (rsrc1 >> 16) & 3 == 3, (n, hex(rsrc1))

