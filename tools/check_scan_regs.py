#!/usr/bin/env python3
"""Build-time check of the register trick the default int8 scan bodies rest on.

The int8 bodies (tools/gen_scan_asm.py: ArchVGPR accumulators) name v64..v191 explicitly and list them as clobbers;
hipcc warns that v128.. are "reserved registers" there.  It works because the kernel descriptor hipcc emits for
these kernels asks for 240 registers per lane (192 ArchVGPRs + 48 AccVGPRs, two waves per SIMD) with nothing spilled.  A
compiler that decided otherwise would still build -- and run wrong, or slowly through scratch.  This script reads the
descriptors back from the object file and fails the build unless every int8 body says exactly that:

    vgpr_count == 240, vgpr_spill_count == 0, private_segment_fixed_size == 0 (no scratch)

Usage: check_scan_regs.py <kernels_filter.o>   (called by `make` after the object is built, and by __graft_entry__.build()).
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
# filter_scan_asm_kernel<SPACE, R, I8, NQT, QB>: the int8 bodies (I8 = true) are the ArchVGPR bodies, one per space and query-tile
# count, and one per space with four Q buffers (kernels_filter.hip, launch_scan_space)
I8_BODY = re.compile(r"_ZN5mlvdb22filter_scan_asm_kernelILi(\d)ELi(\d)ELb1ELi(\d+)E")
WANT = {".vgpr_count": 240, ".vgpr_spill_count": 0, ".private_segment_fixed_size": 0}


def kernel_records(obj: Path):
    """(kernel name, {metadata field: int}) of every gfx950 kernel in the object's offload bundle (decompressed if need be)."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = Path(tmp) / "fat.bin", Path(tmp) / "k.co"
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(obj), str(fat)], check=True)
        if not fat.exists() or fat.stat().st_size == 0:
            raise SystemExit(f"{obj}: no .hip_fatbin section")
        subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        # amdhsa.kernels is a YAML list; one record per "  - .key:" item
        for rec in re.split(r"\n\s+- (?=\.[a-z_]+:)", notes):
            m = re.search(r"\.name:\s+(\S+)", rec)
            if m:
                fields = {k: int(v) for k, v in re.findall(r"(\.[a-z_]+):\s+(\d+)\s*$", rec, flags=re.M)}
                yield m.group(1), fields


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    obj = Path(argv[1])
    checked, bad = 0, []
    for name, f in kernel_records(obj):
        if not I8_BODY.match(name):
            continue
        checked += 1
        for key, want in WANT.items():
            if f.get(key) != want:
                bad.append(f"{name}: {key} = {f.get(key)} (want {want})")
    if checked != 12:
        bad.append(f"{checked} int8 scan bodies found in {obj} (want 12: three spaces x (16 / 8 / 4 query tiles + four Q buffers))")
    if bad:
        print("check_scan_regs: the default scan bodies do not have the register budget they were written for:", file=sys.stderr)
        for b in bad:
            print("  " + b, file=sys.stderr)
        return 1
    print(f"check_scan_regs: {checked} int8 scan bodies: 240 VGPRs, no spills, no scratch")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
