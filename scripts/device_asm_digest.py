#!/usr/bin/env python3
"""Digest of the gfx950 device assembly of the library's HIP sources: for each unit, compile with
`--cuda-device-only -S`, drop the lines that depend on where the tree lies (the `__hip_cuid` symbol, `.file`, `.ident`)
and print the unit, the line count and the sha256 of the rest.  Two trees whose digests agree run the same device code.
    python scripts/device_asm_digest.py [-jN] [kernels_ppm.hip ...] > profiles/<name>.txt      (default: all of HIP_SOURCES)"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artemis_amd.build import HIPCC, HIP_FLAGS, HIP_SOURCES, NO_SINCOS  # noqa: E402


def digest(unit, extra):
    src = os.path.join(ROOT, "artemis_amd", "csrc", unit)
    cmd = [HIPCC] + HIP_FLAGS + (NO_SINCOS if unit == "abi.hip" else []) + extra + ["--cuda-device-only", "-S", src, "-o", "-"]
    asm = subprocess.run(cmd, stdout=subprocess.PIPE, check=True).stdout
    h, n = hashlib.sha256(), 0
    for line in asm.splitlines(keepends=True):
        if b"__hip_cuid" in line or line.lstrip().startswith((b".file", b".ident")):
            continue
        h.update(line)
        n += 1
    return "%-24s %9d %s" % (unit, n, h.hexdigest())


def main():
    args = sys.argv[1:]
    jobs = max([int(a[2:]) for a in args if a.startswith("-j")] + [1])
    extra = [a for a in args if a.startswith("-") and not a.startswith("-j")]
    units = [a for a in args if not a.startswith("-")] or HIP_SOURCES
    print("# %s --cuda-device-only -S <unit>" % " ".join([os.path.basename(HIPCC)] + HIP_FLAGS + extra))
    with ThreadPoolExecutor(jobs) as pool:
        for row in pool.map(lambda u: digest(u, extra), units):
            print(row, flush=True)


if __name__ == "__main__":
    main()
