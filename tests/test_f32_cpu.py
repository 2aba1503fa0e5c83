"""CPU: the float32-row entry points -- declared, bound and exported with their signatures; the
float32 kernel instances exist in the gfx950 code objects under names of their own, use no scratch,
spill nothing, keep their float64 twin's wavefronts-per-SIMD class and compile with the IEEE fp32
denormal mode (the widening conversion follows it); the float64 instances are still there under
their old names; the float32 adaptive path makes no host wait; the torch methods validate before
any device call.  No GPU."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import pytest

from polar_code_amd import _native

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "polar_scl.h"
CSRC = ROOT / "polar_code_amd" / "csrc"
LIB = ROOT / "polar_code_amd" / "libpolar_mi355x.so"
READELF = Path("/opt/rocm/lib/llvm/bin/llvm-readelf")

_SC = ["pscl_handle*", "const float*", "int64_t", "uint64_t*", "uint8_t*", "uint8_t*", "const uint64_t*", "int", "int64_t*"]
NEW = {
    "pscl_f32_available": ["pscl_handle*"],
    "pscl_decode_device_f32": ["pscl_handle*", "const float*", "int64_t", "uint64_t*", "uint8_t*", "const uint64_t*", "int",
                               "int64_t*"],
    "pscl_sc_device_f32": _SC,
    "pscl_escalate_device_f32": _SC + ["int64_t*"],
    "pscl_adaptive_async_device_f32": _SC + ["int32_t*"],
}
# float64 form -> float32 form: the same arguments but the row pointer
TWINS = {"pscl_sc_device": "pscl_sc_device_f32", "pscl_escalate_device": "pscl_escalate_device_f32",
         "pscl_adaptive_async_device": "pscl_adaptive_async_device_f32"}


def _declared_args(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in polar_scl.h"
    return [re.sub(r"\s*\b\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NEW))
def test_declared_bound_and_exported(name):
    assert _declared_args(name) == NEW[name]
    assert name in _native.EXPORTS
    fn = getattr(_native.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(NEW[name])
    for method in ("f32_available", "decode_device_f32", "sc_device_f32", "escalate_device_f32", "adaptive_async_device_f32"):
        assert callable(getattr(_native.Decoder, method))


@pytest.mark.parametrize("f64,f32", sorted(TWINS.items()))
def test_f32_forms_take_their_float64_forms_arguments(f64, f32):
    a, b = _declared_args(f64), _declared_args(f32)
    assert a[1] == "const double*" and b[1] == "const float*" and a[:1] + a[2:] == b[:1] + b[2:]


def test_null_handle():
    lib = _native.lib()
    assert re.search(r"#define PSCL_ABI_VERSION 1\b", HEADER.read_text()) and lib.pscl_abi_version() == 1  # (additions only)
    assert lib.pscl_f32_available(None) == 0
    assert lib.pscl_decode_device_f32(None, None, 0, None, None, None, 0, None) == -1
    assert lib.pscl_sc_device_f32(None, None, 0, None, None, None, None, 0, None) == -1
    assert lib.pscl_escalate_device_f32(None, None, 0, None, None, None, None, 0, None, None) == -1
    assert lib.pscl_adaptive_async_device_f32(None, None, 0, None, None, None, None, 0, None, None) == -1


# ---- the code objects

def _waves_per_simd(vgprs):
    """Wavefronts per SIMD by VGPR count (512 per lane, allocated in blocks of 8, at most 8 waves)."""
    return min(8, 512 // (-(-vgprs // 8) * 8))


@pytest.fixture(scope="module")
def kernels():
    if not LIB.exists() or not READELF.exists():
        pytest.skip("needs the built library and llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernels(LIB)


def _one(kernels, part):
    hits = [(n, v) for n, v in kernels.items() if part in n]
    assert len(hits) == 1, (part, [n for n, _ in hits])
    return hits[0][1]


def _clean(v, tag, sgpr_parked=0):
    """No scratch memory, no spilled VGPR, and at most sgpr_parked SGPRs parked in VGPR lanes (which
    costs no memory traffic)."""
    assert v.get("private_segment_fixed_size", 0) == 0, (tag, "scratch", v)
    assert v.get("vgpr_spill_count", 0) == 0, (tag, "spilled VGPRs", v)
    assert v.get("sgpr_spill_count", 0) <= sgpr_parked, (tag, "SGPRs parked in VGPR lanes", v, sgpr_parked)


def _sgpr_parked_limit(name):
    """SGPRs an instance may park in VGPR lanes: none in the SC and the (128,64) lane instances; the
    float64 lane instances of the (128,88) code park 2 (L = 8) and 4 (L = 4, plain form); the exact
    scl128_kernel instances park 162-245 by design (they sit at their VGPR limit)
    -- their float32 forms may reach the float64 figures of this build, not pass them."""
    m = re.search(r"scl_lane_kernel(?:_f32)?ILi(\d)ELi(\d)ELb0ELb0ELb0ELb0ELb(\d)EE", name)
    if m:
        l, code, rl = map(int, m.groups())
        return {(8, 2, 0): 2, (4, 2, 0): 4}.get((l, code, rl), 0)
    m = re.search(r"scl128_kernel(?:_f32)?ILi(\d)ELb0ELb\dELb0ELi(\d)ELb0EE", name)
    if m:
        return {(4, 1): 176, (4, 2): 245, (8, 1): 162, (8, 2): 236}[tuple(map(int, m.groups()))]
    return 0


# (float32 name part, float64 name part) of every instance pair
PAIRS = (
    [(f"sc128_lane_kernel_f32ILb{rm}EE", f"sc128_lane_kernelILb{rm}EE") for rm in (0, 1)]
    + [(f"scl_lane_kernel_f32ILi{l}ELi{c}ELb0ELb0ELb0ELb0ELb{rl}EE", f"scl_lane_kernelILi{l}ELi{c}ELb0ELb0ELb0ELb0ELb{rl}EE")
       for l in (4, 8) for c in (1, 2) for rl in (0, 1)]
    + [(f"scl128_kernel_f32ILi{l}ELb0ELb{c - 1}ELb0ELi{c}ELb0EE", f"scl128_kernelILi{l}ELb0ELb{c - 1}ELb0ELi{c}ELb0EE")
       for l in (4, 8) for c in (1, 2)]
)


@pytest.mark.parametrize("f32,f64", PAIRS)
def test_f32_instance_is_clean_and_keeps_its_twins_occupancy_class(f32, f64, kernels):
    a, b = _one(kernels, f32), _one(kernels, f64)
    _clean(a, f32, _sgpr_parked_limit(f32))
    _clean(b, f64, _sgpr_parked_limit(f64))
    assert a.get("sgpr_spill_count", 0) <= b.get("sgpr_spill_count", 0), (f32, a, b)
    assert _waves_per_simd(a["vgpr_count"]) >= _waves_per_simd(b["vgpr_count"]), (f32, a["vgpr_count"], b["vgpr_count"])


def test_sc_instances_stay_inside_their_register_budget(kernels):
    """Three wavefronts per SIMD on plain rows (168 VGPRs), two on rate-matched rows."""
    assert _one(kernels, "sc128_lane_kernel_f32ILb0EE")["vgpr_count"] <= 168
    assert _one(kernels, "sc128_lane_kernel_f32ILb1EE")["vgpr_count"] <= 256


def test_gather_twin_exists_and_is_clean(kernels):
    _clean(_one(kernels, "sc_gather_rows_f32_kernel"), "gather")
    _one(kernels, "sc_gather_rows_kernel")


def test_f32_units_hold_nothing_but_their_instances(kernels):
    """No float32 instance of a form the entry points never launch (fused TX, forced bits, the exact
    lane instance, the screening forms of scl128_kernel)."""
    lane = [n for n in kernels if "scl_lane_kernel_f32" in n]
    spec = [n for n in kernels if "scl128_kernel_f32" in n]
    sc = [n for n in kernels if "sc128_lane_kernel_f32" in n]
    assert (len(lane), len(spec), len(sc)) == (8, 4, 2), (lane, spec, sc)


def _kernel_descriptors(elf):
    """{kernel name: its 64-byte kernel descriptor} of one code object (the <name>.kd symbols)."""
    import struct

    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in secs:
        if s[1] not in (2, 11):  # SHT_SYMTAB, SHT_DYNSYM
            continue
        strtab = secs[s[6]]
        for k in range(s[5] // 24):
            name_off, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, s[4] + 24 * k)
            end = elf.index(b"\0", strtab[4] + name_off)
            name = elf[strtab[4] + name_off:end].decode()
            if name.endswith(".kd") and 0 < shndx < shnum:
                sec = secs[shndx]
                off = sec[4] + value - sec[3]
                out[name[:-3]] = elf[off:off + 64]
    return out


@pytest.mark.skipif(not LIB.exists(), reason="needs the built library")
def test_f32_instances_keep_fp32_denormals():
    """v_cvt_f64_f32 follows the wave's fp32 denormal mode: the instances must not flush (a flushed
    subnormal LLR would lose its sign at the `llr < 0` decision).  FLOAT_DENORM_MODE_32 (bits 16-17 of
    compute_pgm_rsrc1, byte 48 of the kernel descriptor) is 3 -- input and output denormals kept --
    in every float32 instance."""
    import struct

    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kds = {}
    for co in mod.code_objects(LIB):
        kds.update(_kernel_descriptors(co))
    f32 = {n: kd for n, kd in kds.items() if "_f32" in n}
    assert len(f32) == 15, sorted(f32)  # (2 SC + the gather, 8 lane, 4 exact)
    for n, kd in f32.items():
        rsrc1, = struct.unpack_from("<I", kd, 48)
        assert (rsrc1 >> 16) & 3 == 3, (n, hex(rsrc1))
    from polar_code_amd import build

    assert not (set(build.BASE_FLAGS) & {"-fgpu-flush-denormals-to-zero", "-ffast-math", "-Ofast"})


# ---- the path without a host wait

F32_ASYNC_FUNCS = ("f32_unsupported", "adaptive_async_impl", "pscl_adaptive_async_device_f32", "pscl_adaptive_async_device",
                   "adaptive_begin", "adaptive_escalate_enqueue", "launch_sc_stage", "pscl_f32_available")


def test_f32_async_path_makes_no_host_wait():
    spec = importlib.util.spec_from_file_location("stream_order", ROOT / "tests" / "test_stream_order.py")
    so = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(so)
    src = so.strip_comments((CSRC / "capi.cpp").read_text())
    for name in F32_ASYNC_FUNCS:
        m = re.search(r"\b" + name + r"\s*\([^;{}]*\)\s*\{", src)
        assert m, f"{name} not found in capi.cpp"
        depth, j = 0, m.end() - 1
        while True:
            depth += {"{": 1, "}": -1}.get(src[j], 0)
            if depth == 0:
                break
            j += 1
        body = src[m.end() - 1:j]
        assert not re.search(r"\bhip\w*Synchronize\s*\(", body), f"{name} waits on the host"
        assert not re.search(r"\bhipMemcpy\s*\(|\bhipMemcpyAsync\s*\([^;]*DeviceToHost", body), f"{name} copies to the host"


def test_dtype_flag_is_per_call_not_handle_state():
    """pscl_handle has no float32 member: the flag lives in the launches' parameter blocks."""
    src = (CSRC / "capi.cpp").read_text()
    m = re.search(r"struct pscl_handle \{(.*?)\n\};", src, re.S)
    assert m and "f32" not in m.group(1)
    hdr = (CSRC / "scl_kernels.h").read_text()
    body = re.search(r"struct pscl_decode_params \{(.*?)\n\};", hdr, re.S).group(1)
    # in the padding between rm_E and rm_src, held there by a static_assert: the block keeps its size
    # and every member its offset, so the float64 kernels' argument offsets do not move
    body = re.sub(r"\s*//[^\n]*", "", body)
    assert re.search(r"int rm_E;\s+int f32;\s+const int32_t\* rm_src;", body)
    assert re.search(r"static_assert\(offsetof\(pscl_decode_params, rm_src\) == offsetof\(pscl_decode_params, rm_E\) \+ 8", hdr)
    # the SC block has no padding to spare: the row type of an SC launch is the launch function called
    assert "f32" not in re.search(r"struct pscl_sc_params \{(.*?)\n\};", hdr, re.S).group(1)
    # the flag is set where a _f32 entry point passes it down, nowhere else
    assert re.findall(r"\.f32 = ([^;]*);", src) == ["f32 ? 1 : 0", "f32 ? 1 : 0"]


# ---- the torch methods validate before any device call

class _NoDevice:
    """Stands in for the native decoder: the row length and nothing else."""
    E, W = 0, 1

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before validation")


@pytest.mark.parametrize("method", ["decode_tensor", "decode_tensor_adaptive_async", "decode_tensor_staged", "decode_tensor_sc"])
def test_tensor_methods_refuse_bad_rows_before_any_device_call(method):
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    dec = SCLDecoder.__new__(SCLDecoder)
    dec.N, dec.L, dec._dec = 128, 8, _NoDevice()
    call = getattr(dec, method)
    for bad in (torch.zeros((4, 128), dtype=torch.float16),
                torch.zeros((4, 128), dtype=torch.bfloat16),
                torch.zeros((4, 128), dtype=torch.int32),
                torch.zeros((4, 256), dtype=torch.float32)[:, ::2],  # not contiguous
                torch.zeros((128, 4), dtype=torch.float32).t(),      # not contiguous
                torch.zeros((4, 127), dtype=torch.float32),
                torch.zeros((4, 129), dtype=torch.float32),
                torch.zeros((128,), dtype=torch.float32),
                torch.zeros((4, 256), dtype=torch.float64)[:, ::2],
                torch.zeros((4, 127), dtype=torch.float64)):
        with pytest.raises(ValueError):
            call(bad)
    # (good rows reach the device layer: the stand-in objects to the first call)
    for good in (torch.zeros((4, 128), dtype=torch.float32), torch.zeros((4, 128), dtype=torch.float64)):
        with pytest.raises(AssertionError, match="device call"):
            call(good)
