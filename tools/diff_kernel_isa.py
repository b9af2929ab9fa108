#!/usr/bin/env python3
"""Compare the gfx950 machine code of every kernel of two csrc directories (CPU only: hipcc cross-compiles).

    python tools/diff_kernel_isa.py <csrc before> <csrc after>

Every .hip of each directory is compiled with the Makefile's flags plus --offload-device-only -S.  A kernel's text is
its assembly from its label to its .end_amdhsa_kernel (the instructions and the .amdhsa_* descriptor block).  Kernels
are matched by mangled name, whichever file they are in.  Two things that only count the functions of the file are
taken out first: the function number in block and jump-table labels (BB<function>_<block>), and the padding in front of
comments, which follows the label's length.  Prints "identical" or a unified diff per kernel; exit status 1 on any
difference or on a kernel that only one side has.  The comparison is of text: no instruction is looked for.
"""
import concurrent.futures
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("ARCH", "gfx950")


def makefile_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    return re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", ARCH).split()


def assembly(src, flags, out_dir):
    out = os.path.join(out_dir, os.path.basename(src) + ".s")
    r = subprocess.run([HIPCC, *flags, "--offload-device-only", "-S", src, "-o", out], cwd=os.path.dirname(src),
                       capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{src} does not compile:\n{r.stderr}")
    return open(out).read().splitlines()


def kernels(csrc, out_dir):
    """{mangled name: its lines} over every .hip of csrc."""
    flags = makefile_flags(csrc)
    srcs = sorted(glob.glob(os.path.join(os.path.abspath(csrc), "*.hip")))
    found = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        for src, lines in zip(srcs, pool.map(lambda s: assembly(s, flags, out_dir), srcs)):
            start = {}
            for i, line in enumerate(lines):
                m = re.match(r"(\w+):", line)
                if m:
                    start[m.group(1)] = i
                m = re.match(r"\s*\.amdhsa_kernel (\w+)", line)
                if m:
                    name = m.group(1)
                    end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
                    if name in found:
                        sys.exit(f"{name} is defined twice in {csrc} (second time in {os.path.basename(src)})")
                    body = [re.sub(r"(BB|JTI)\d+_(\d)", r"\1_\2", s) for s in lines[start[name]:end + 1]]
                    found[name] = [re.sub(r"\s+;", " ;", s) for s in body]    # comments are padded to a column
    return found


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = kernels(sys.argv[1], ta), kernels(sys.argv[2], tb)
    differ = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only in {sys.argv[1] if name in a else sys.argv[2]}")
            differ += 1
        elif a[name] == b[name]:
            print(f"{name}: identical ({len(a[name])} lines)")
        else:
            print(f"{name}: DIFFERENT")
            print("\n".join(difflib.unified_diff(a[name], b[name], "before", "after", lineterm="", n=2)))
            differ += 1
    print(f"{len(a)} kernels before, {len(b)} after, {differ} different or unmatched")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
