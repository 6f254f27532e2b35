#!/usr/bin/env python3
"""Static audit of LDS read latency in the generated code: compile one HIP source of the library to gfx950 assembly
with build.py's flags and print, per kernel, what its main loop holds and how many LDS round trips it exposes.

    python scripts/lds_wait_audit.py kernels_fused.hip [extra hipcc flags] > profiles/lds_batch_audit_kernels_fused.txt

Definitions (text order of the assembly; control flow inside the region is ignored)
  region     the largest backward-branch span of the kernel (label ... branch back to it): the plane loop of a march;
             the whole body when the kernel has no loop.
  VALU       instructions whose mnemonic starts with `v_`; ds_read / ds_write: `ds_read*` / `ds_write*` (LDS atomics
             and the like are counted with neither).
  read group a maximal run of `ds_read*` with no `s_waitcnt lgkmcnt(..)` between them: LDS operations return in order
             and back to back, so the reads of a group cost the wave one round trip, however many waits (lgkmcnt(3),
             lgkmcnt(2), ...) then pick its values up one by one.
  wait       a read group some `s_waitcnt lgkmcnt(N)` retires a read of (such a wait retires every LDS operation
             issued before it except the N youngest); each group counts once, at the first such wait.
  exposed    a wait with at most EXPOSED_VALU (2) VALU instructions between the group's youngest read and that first
             wait: nothing of the wave's own covers the round trip.
The count is static: one per instruction in the text, whatever share of the waves runs the branch it stands in.
"""
import functools
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from artemis_amd.build import HIPCC, HIP_FLAGS  # noqa: E402

EXPOSED_VALU = 2

_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
_INSN = re.compile(r"^\s+([a-z_][a-z0-9_]*)")
_LGKM = re.compile(r"lgkmcnt\((\d+)\)")


def compile_asm(source, extra=()):
    """The gfx950 assembly of artemis_amd/csrc/<source> (device side only) with the library's flags, as text."""
    src = os.path.join(ROOT, "artemis_amd", "csrc", source)
    cmd = [HIPCC] + HIP_FLAGS + list(extra) + ["--cuda-device-only", "-S", src, "-o", "-"]
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout


def kernels(asm):
    """{mangled name: {"lines": [...], <metadata fields of the .amdhsa_kernel block and the resource comments>}}"""
    lines = asm.splitlines()
    names = [m.group(1) for m in (re.match(r"^\s+\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    out = {}
    known = set(names)
    start = {}
    for i, ln in enumerate(lines):  # `<name>:` at the start of a line, possibly with a comment behind it
        head = ln.split(":", 1)[0]
        if head in known and ln.startswith(head + ":"):
            start.setdefault(head, i)
    for name in names:
        if name not in start:
            continue
        i0 = start[name]
        i1 = i0
        while i1 < len(lines) and not lines[i1].startswith(".Lfunc_end"):
            i1 += 1
        info = {"lines": lines[i0 + 1:i1]}
        for ln in lines[i1:i1 + 400]:  # the resource comments and the descriptor follow the body
            m = re.match(r"^; (ScratchSize|Occupancy|NumVgprs|LDSByteSize): (\d+)", ln)
            if m:
                info[m.group(1)] = int(m.group(2))
            if ln.startswith("\t.end_amdhsa_kernel"):
                break
        out[name] = info
    return out


def main_region(lines):
    """(first, last) line indices of the largest backward-branch span; the whole body if there is none."""
    at = {}
    best = None
    for i, ln in enumerate(lines):
        m = _LABEL.match(ln)
        if m:
            at[m.group(1)] = i
            continue
        m = _BRANCH.match(ln)
        if m and m.group(1) in at and (best is None or i - at[m.group(1)] > best[1] - best[0]):
            best = (at[m.group(1)], i)
    return best or (0, len(lines) - 1)


def audit(lines):
    """Counts over the main region of one kernel body (see the module docstring)."""
    lo, hi = main_region(lines)
    n = {"valu": 0, "ds_read": 0, "ds_write": 0, "waits": 0, "exposed": 0, "loop": (lo, hi) != (0, len(lines) - 1)}
    pending = []  # LDS operations not yet retired, oldest first: the read group they belong to, or None
    youngest = {}  # read group -> VALU count at its youngest read
    group, open_ = 0, False
    for ln in lines[lo:hi + 1]:
        m = _INSN.match(ln)
        if not m:
            continue
        op = m.group(1)
        if op.startswith("v_"):
            n["valu"] += 1
        elif op.startswith("ds_"):
            rd = op.startswith("ds_read")
            n["ds_read"] += rd
            n["ds_write"] += op.startswith("ds_write")
            if rd and not open_:
                group, open_ = group + 1, True
            if rd:
                youngest[group] = n["valu"]
            pending.append(group if rd else None)
        elif op == "s_waitcnt":
            c = _LGKM.search(ln)
            if not c:
                continue
            open_ = False
            keep = int(c.group(1))
            retired = pending[:len(pending) - keep] if keep else pending
            pending = pending[len(pending) - keep:] if keep else []
            for g in sorted({g for g in retired if g is not None and g in youngest}):
                n["waits"] += 1
                n["exposed"] += (n["valu"] - youngest.pop(g)) <= EXPOSED_VALU
    return n


def demangle(names):
    out = subprocess.run(["c++filt"] + list(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    out = [re.sub(r"artemis::\(anonymous namespace\)::", "", x) for x in out]
    return [re.sub(r"\(.*$", "", x) for x in out]


def table(source, extra=()):
    """[(demangled kernel name, audit counts + resource fields)] for every kernel of the source (compiled once per
    process and command line: two test modules ask for the same table)."""
    return list(_table(source, tuple(extra)))


@functools.lru_cache(maxsize=None)
def _table(source, extra):
    ks = kernels(compile_asm(source, extra))
    rows = []
    for name, short in zip(ks, demangle(ks)):
        r = audit(ks[name]["lines"])
        r.update({k: v for k, v in ks[name].items() if k != "lines"})
        rows.append((short, r))
    return rows


def main():
    rows = table(sys.argv[1], sys.argv[2:])
    print("# %s %s --cuda-device-only -S artemis_amd/csrc/%s" % (os.path.basename(HIPCC), " ".join(HIP_FLAGS + sys.argv[2:]), sys.argv[1]))
    print("# region: the kernel's largest loop (L) or its whole body (B); exposed: <= %d VALU between read and wait" % EXPOSED_VALU)
    print("%-100s %2s %6s %7s %8s %5s %7s" % ("kernel", "", "VALU", "ds_read", "ds_write", "waits", "exposed"))
    for short, r in rows:
        print("%-100s %2s %6d %7d %8d %5d %7d" % (short[:100], "L" if r["loop"] else "B", r["valu"], r["ds_read"],
                                                  r["ds_write"], r["waits"], r["exposed"]))


if __name__ == "__main__":
    main()
