#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code of two builds (objects or libraries): opcode histogram and differing disassembly lines
(addresses and encodings stripped).  What a refactor that must not change a kernel is checked with, next to tools/kernel_stats.py.
    python tools/isa_diff.py OLD/libmppi_hip.so NEW/libmppi_hip.so [--show kernel-name-part]"""
import collections
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(path):
    """{symbol: [instruction text, ...]} of every gfx950 code object in `path` (a symbol that repeats in several units: its first copy)"""
    tmp = tempfile.mkdtemp(prefix="isadiff_")
    try:
        shutil.copy(path, os.path.join(tmp, "in.bin"))
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "in.bin"], cwd=tmp, check=True, capture_output=True)
        out = {}
        for co in sorted(glob.glob(os.path.join(tmp, "in.bin.*gfx950*"))):
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = None if m.group(1) in out else out.setdefault(m.group(1), [])
                    continue
                code = line.split("//")[0].strip()
                if cur is not None and code and not code.endswith(":"):
                    cur.append(code)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    show = sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--show" else None
    if set(a) != set(b):
        print("kernel sets differ:", sorted(set(a) ^ set(b)))
    total = differing = other_histogram = 0
    for k in sorted(set(a) & set(b)):
        total += len(b[k])
        if a[k] == b[k]:
            continue
        ha, hb = (collections.Counter(l.split()[0] for l in x[k]) for x in (a, b))
        ops = difflib.SequenceMatcher(None, a[k], b[k], autojunk=False).get_opcodes()
        nd = sum(max(i2 - i1, j2 - j1) for t, i1, i2, j1, j2 in ops if t != "equal")
        differing += nd
        hd = {o: (ha[o], hb[o]) for o in set(ha) | set(hb) if ha[o] != hb[o]}
        other_histogram += bool(hd)
        print(f"{k[:100]:<100} lines {len(a[k])}/{len(b[k])} differing {nd} histogram {hd if hd else 'same'}")
        if show and show in k:
            for l in difflib.unified_diff(a[k], b[k], lineterm="", n=2):
                print("    " + l)
    print(f"{len(set(a) & set(b))} kernels, {total} disassembly lines, {differing} differing, {other_histogram} kernels with another opcode histogram")
    return 1 if other_histogram or set(a) != set(b) else 0


if __name__ == "__main__":
    sys.exit(main())
