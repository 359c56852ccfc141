#!/usr/bin/env python3
"""Register / scratch / LDS use per kernel, from the code-object metadata hipcc writes with --save-temps.
usage: tools/kernel_regs.py fq_pc.hip [substring ...] [-Dflags ...] [--hash]   (compiles with the product Makefile's flags)
--hash adds a hash of each kernel's instruction stream: two builds whose tables are equal run the same device code."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_hash(text, mangled):
    """The kernel's body, label to .rodata, without comments, symbol names and the function's index in its labels."""
    body = text.split("\n" + mangled + ":", 1)[1].split("\t.section\t.rodata", 1)[0]
    body = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", re.sub(r";.*", "", body)))
    return hashlib.sha256("\n".join(ln.strip() for ln in body.splitlines() if ln.strip()).encode()).hexdigest()[:16]


def main():
    src = sys.argv[1]
    want_hash = "--hash" in sys.argv[2:]
    flags = [a for a in sys.argv[2:] if a.startswith("-") and a != "--hash"]
    subs = [a for a in sys.argv[2:] if not a.startswith("-")]
    base = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "mhaq_amd", "csrc"), "print-flags"],
                          capture_output=True, text=True, check=True).stdout.split()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["/opt/rocm/bin/hipcc", *base, *flags, "--save-temps", "-c",
                        os.path.join(ROOT, "mhaq_amd", "csrc", src), "-o", "x.o"], cwd=tmp, check=True,
                       stderr=subprocess.DEVNULL)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")][0]
        text = open(os.path.join(tmp, asm)).read()
    rows = []
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        f = {k: v for k, v in re.findall(r"\n\s+\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size"
                                         r"|max_flat_workgroup_size):\s+(\S+)", blk)}
        name = subprocess.run(["c++filt", f["name"]], capture_output=True, text=True).stdout.strip()
        name = name.split("(")[0].replace("void ", "")
        if subs and not any(s in name for s in subs):
            continue
        rows.append((name, int(f["vgpr_count"]), int(f["sgpr_count"]), int(f["private_segment_fixed_size"]),
                     int(f["group_segment_fixed_size"]), int(f["max_flat_workgroup_size"]),
                     "  stream " + stream_hash(text, f["name"]) if want_hash else ""))
    for name, vg, sg, scr, lds, wg, sh in sorted(rows):
        waves = min(8, 512 // max(vg, 1))
        print(f"{name:75s} vgpr {vg:3d} (<= {waves} waves/SIMD)  sgpr {sg:3d}  scratch {scr:4d}  lds {lds:6d}  wg {wg}{sh}")


if __name__ == "__main__":
    main()
