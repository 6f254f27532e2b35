#!/usr/bin/env python3
"""What a reduced field output costs next to the full one, and that the time loop is what it was (DESIGN.md "Reduced field
outputs").

One MI355X, one job:

  (a) the flagship 256^3 Sedov deck of bench.py (inputs/blast/blast.in, Cartesian, gas only), one block, the three shipped
      variables (gas.prim.density, .velocity, .pressure: five components): Simulation.gather() in full
      (artemis_hip_pack_fields) and with reduce = {x3}, {x2, x3}, {x1, x2, x3} (artemis_hip_reduce_fields), in double and in
      float: median, minimum and maximum of --calls calls after 2 warm-up calls, on the state after the warm-up cycles.
      These are CALL times -- kernels, the device-to-host copy into pageable memory, synchronisation -- not kernel times;
  (b) the shipped inputs/disk/disk_sph.in (spherical-polar, 128 x 64 x 64 in sixteen blocks of 32^3): the same for reduce = {x3} (the
      azimuthal integral) and {x2, x3} (the radial profile) next to the full gather;
  (c) zone-cycles/s of --cycles cycles of (a)'s deck (one evolve() call, the driver's own device-synchronised wall clock)
      with outputs off; with --parent DIR the same loop also runs on the library and Python package of another checkout (the
      parent commit, built there) in a process of its own, alternating, --repeats times each; the runs must take
      bit-identical steps (asserted).

Prints one JSON object.  A machine without a GPU fails in capi.load() / Simulation().

    python3 scripts/fields_reduce_cost.py [--n 256] [--cycles 200] [--repeats 3] [--parent DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from history_cost import loop, overrides  # noqa: E402

SHIPPED = ["gas.prim.density", "gas.prim.velocity", "gas.prim.pressure"]


def timed(f, warm, calls):
    for _ in range(warm):
        f()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        out.append(time.perf_counter() - t0)
    return dict(median=1e3 * statistics.median(out), min=1e3 * min(out), max=1e3 * max(out), calls=len(out))


def gathers(s, reductions, calls):
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    res = dict(zones=s.total_zones, block=list(nx), bytes_read=5 * 8 * s.total_zones)
    for red in (None,) + tuple(reductions):
        tag = "full" if red is None else "reduce_" + "".join(red)
        out = s.gather(SHIPPED, reduce=red)
        res[tag] = dict(shape=list(out.shape), bytes_out_f8=out.nbytes,
                        gather_f8_ms=timed(lambda: s.gather(SHIPPED, reduce=red), 2, calls),
                        gather_f4_ms=timed(lambda: s.gather(SHIPPED, single=True, reduce=red), 2, calls))
        if red is not None:
            res[tag]["over_full_f8"] = res[tag]["gather_f8_ms"]["median"] / res["full"]["gather_f8_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--parent", default=None, help="another checkout (built) whose outputs-off loop is timed too")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, ROOT)
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    deck = os.path.join(ROOT, "inputs", "blast", "blast.in")
    res = dict(n=args.n, cycles=args.cycles, source_sha=capi.source_sha(), variables=SHIPPED,
               note="call times (kernels + device-to-host copy + synchronisation), not kernel times")
    s = Simulation(deck, overrides(args.n))
    s.evolve(args.warm)
    res["a"] = gathers(s, (("x3",), ("x2", "x3"), ("x1", "x2", "x3")), args.calls)
    s.close()
    s = Simulation(os.path.join(ROOT, "inputs", "disk", "disk_sph.in"), ["parthenon/time/nlim=-1"])
    s.evolve(args.warm)
    res["b"] = gathers(s, (("x3",), ("x2", "x3")), args.calls)
    s.close()
    off, parent = [], []
    loop(Simulation, deck, args.n, args.warm, args.cycles)  # (warms every shape of the loop)
    for _ in range(args.repeats):
        off.append(loop(Simulation, deck, args.n, args.warm, args.cycles))
        if args.parent:
            cmd = [sys.executable, os.path.join(os.path.abspath(args.parent), "scripts", "history_cost.py"), "--loop-only", "--root",
                   os.path.abspath(args.parent), "--n", str(args.n), "--warm", str(args.warm), "--cycles", str(args.cycles)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=600)
            assert p.returncode == 0, "the parent's loop failed"
            parent.append(json.loads(p.stdout.decode().strip().split("\n")[-1]))
    assert all(r["time"] == off[0]["time"] and r["dt"] == off[0]["dt"] for r in off + parent), "the runs took different steps"
    res["c"] = dict(outputs_off=[r["zone_cycles_per_s"] for r in off], parent_outputs_off=[r["zone_cycles_per_s"] for r in parent],
                    parent_source_sha=parent[0]["source_sha"] if parent else None, bit_identical_steps=True)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
