"""Machine code of every kernel of one built library against another's, function by function (no GPU).

    python tools/compare_kernels.py <old library> <new library>

For "this change leaves the existing kernels as they were": build the parent commit in a checkout of its
own (python -m polar_code_amd.build), then compare its polar_code_amd/libpolar_mi355x.so with this
tree's.  Every function symbol of every gfx950 code object (tools/kernel_resources.py finds them in the
offload bundles) is read as the bytes between its address and its size; a kernel is identical when
those bytes are.  Prints the kernels that differ, the ones that are gone and the new ones; exit status 1
if a kernel of the old library differs or is missing.
"""
import importlib.util
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


def functions(elf: bytes) -> dict:
    """{symbol: code bytes} of the STT_FUNC symbols of one ELF code object."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in secs:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        strtab = secs[s[6]]
        for k in range(s[5] // 24):
            name_off, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, s[4] + 24 * k)
            if (info & 15) != 2 or not 0 < shndx < shnum or size == 0:
                continue
            end = elf.index(b"\0", strtab[4] + name_off)
            sec = secs[shndx]
            off = sec[4] + value - sec[3]
            out[elf[strtab[4] + name_off:end].decode()] = elf[off:off + size]
    return out


def library_functions(lib: Path) -> dict:
    out = {}
    for co in kr.code_objects(lib):
        for name, code in functions(co).items():
            assert name not in out, f"{name} is defined in two code objects"
            out[name] = code
    return out


def main():
    old, new = (library_functions(Path(p)) for p in sys.argv[1:3])
    differ = [n for n in sorted(old) if n in new and old[n] != new[n]]
    gone = [n for n in sorted(old) if n not in new]
    added = sorted(set(new) - set(old))
    for n in differ:
        print(f"DIFFERS  {len(old[n])} -> {len(new[n])} bytes  {n}")
    for n in gone:
        print(f"MISSING  {n}")
    for n in added:
        print(f"new      {len(new[n])} bytes  {n}")
    print(f"old library: {len(old)} kernels; identical code {len(old) - len(differ) - len(gone)}, different {len(differ)}, "
          f"missing {len(gone)}; new {len(added)}")
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main())
