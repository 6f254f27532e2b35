#!/usr/bin/env python3
"""What setting a run's state from arrays costs, and that the time loop of a run that never does is what it was (DESIGN.md
"Deck-driven outputs", scatter).

One MI355X, the flagship 256^3 Sedov deck of bench.py (inputs/blast/blast.in, Cartesian, gas only), one block:

  (a) one Simulation.scatter() of the five primitive components (gas.prim.density, .velocity, .sie) in double and in float,
      each as the median of repeated calls after warm-up calls, on the state after the warm-up cycles (the run scatters
      the state it holds), next to Simulation.gather() of the same variables in the same job.  These are CALL times, not
      kernel times: a scatter is the host-to-device copy of the arrays, artemis_hip_unpack_fields, PrimToCons, ConsToPrim,
      the ghost fill, PrimToCons and the timestep estimate, synchronised;
  (b) zone-cycles/s of --cycles cycles (one evolve() call, the driver's own device-synchronised wall clock); with --parent
      DIR the same loop also runs on the library and Python package of another checkout (the parent commit, built there)
      in a process of its own, alternating, --repeats times each.  Asserts that all of them took bit-identical steps.

Prints one JSON object keyed on artemis_hip_source_sha().  A machine without a GPU fails in capi.load() / Simulation().

    python3 scripts/scatter_cost.py [--n 256] [--cycles 200] [--repeats 3] [--parent DIR] [--out FILE]
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

PRIM = ["gas.prim.density", "gas.prim.velocity", "gas.prim.sie"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--parent", default=None, help="another checkout (built) whose loop is timed too")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, ROOT)
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    deck = os.path.join(ROOT, "inputs", "blast", "blast.in")
    res = dict(n=args.n, cycles=args.cycles, source_sha=capi.source_sha(), variables=PRIM)
    s = Simulation(deck, overrides(args.n))
    s.evolve(args.warm)

    def timed(f, warm, calls):
        for _ in range(warm):
            f()
        out = []
        for _ in range(calls):
            t0 = time.perf_counter()
            f()
            out.append(time.perf_counter() - t0)
        return dict(median=1e3 * statistics.median(out), min=1e3 * min(out), max=1e3 * max(out), calls=len(out))
    zones = s.total_zones
    g8, g4 = s.gather(PRIM), s.gather(PRIM, single=True)
    res["a"] = dict(what="call times in ms (copy + unpack + PrimToCons + ConsToPrim + ghost fill + PrimToCons + dt estimate), not kernel times",
                    scatter_f8_ms=timed(lambda: s.scatter(PRIM, g8), 2, args.calls),
                    scatter_f4_ms=timed(lambda: s.scatter(PRIM, g4), 2, args.calls),
                    gather_f8_ms=timed(lambda: s.gather(PRIM), 2, args.calls),
                    gather_f4_ms=timed(lambda: s.gather(PRIM, single=True), 2, args.calls),
                    bytes_in_f8=5 * 8 * zones, bytes_in_f4=5 * 4 * zones, bytes_written=5 * 8 * zones)
    s.scatter(PRIM, g8)
    assert (s.gather(PRIM) == g8).all(), "the scattered state did not come back"  # (a floored state is a fixed point)
    s.close()
    here, parent = [], []
    loop(Simulation, deck, args.n, args.warm, args.cycles)  # (warms every shape of the loop)
    for _ in range(args.repeats):
        here.append(loop(Simulation, deck, args.n, args.warm, args.cycles))
        if args.parent:
            cmd = [sys.executable, os.path.join(os.path.abspath(args.parent), "scripts", "history_cost.py"), "--loop-only", "--root",
                   os.path.abspath(args.parent), "--n", str(args.n), "--warm", str(args.warm), "--cycles", str(args.cycles)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=600)
            assert p.returncode == 0, "the parent's loop failed"
            parent.append(json.loads(p.stdout.decode().strip().split("\n")[-1]))
    assert all(r["time"] == here[0]["time"] and r["dt"] == here[0]["dt"] for r in here + parent), "the runs took different steps"
    rates = [r["zone_cycles_per_s"] for r in here], [r["zone_cycles_per_s"] for r in parent]
    res["b"] = dict(this_library=rates[0], parent_library=rates[1], parent_source_sha=parent[0]["source_sha"] if parent else None,
                    spread_this=(max(rates[0]) - min(rates[0])) / min(rates[0]),
                    spread_parent=(max(rates[1]) - min(rates[1])) / min(rates[1]) if parent else None,
                    identical_steps=True, end_time=here[0]["time"], end_dt=here[0]["dt"])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
