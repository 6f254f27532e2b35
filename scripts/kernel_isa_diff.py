#!/usr/bin/env python3
"""Are the kernels of one HIP unit instruction-identical between two checkouts?  (a unit that gains
kernels changes its object hash; this says whether the kernels it already had changed.)

    python3 scripts/kernel_isa_diff.py kernels_sample.hip /path/to/other/checkout

compiles artemis_amd/csrc/<unit> of this checkout and of the other one to gfx950 assembly with the library's flags
(`--cuda-device-only -S`, no GPU needed) and compares, kernel by kernel, the instruction streams with comments dropped and
the basic-block label numbers normalised (they count the functions of the unit, so they move when a kernel is added).
Prints SAME / DIFF for every kernel both units have and NEW / GONE for the rest; exit status 1 if any kernel differs.
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from artemis_amd.build import HIP_FLAGS, HIPCC  # noqa: E402


def kernels(root, unit, tmp, tag):
    out = os.path.join(tmp, tag + ".s")
    subprocess.check_call([HIPCC] + HIP_FLAGS + ["--cuda-device-only", "-S", os.path.join(root, "artemis_amd", "csrc", unit), "-o", out],
                          stderr=subprocess.DEVNULL)
    fns, cur = {}, None
    for line in open(out):
        m = re.match(r"^(\w+):", line)
        if m and not line.startswith(".L"):
            cur = m.group(1)
            fns[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith("\t.section") or ".amdhsa_kernel" in line:
            cur = None
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";.*", "", line)).strip()
        if s and not s.startswith("."):
            fns[cur].append(s)
    return {k: v for k, v in fns.items() if len(v) > 1}


def main():
    unit, other = sys.argv[1], os.path.abspath(sys.argv[2])
    with tempfile.TemporaryDirectory() as tmp:
        mine, theirs = kernels(ROOT, unit, tmp, "this"), kernels(other, unit, tmp, "other")
    bad = 0
    for k in sorted(set(mine) | set(theirs)):
        state = "NEW " if k not in theirs else "GONE" if k not in mine else "SAME" if mine[k] == theirs[k] else "DIFF"
        bad += state == "DIFF"
        print(state, len(mine.get(k, theirs.get(k))), k)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
