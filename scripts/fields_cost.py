#!/usr/bin/env python3
"""What a field dump costs, and that the time loop without one is what it was (DESIGN.md "Deck-driven outputs").

One MI355X, the flagship 256^3 Sedov deck of bench.py (inputs/blast/blast.in, Cartesian, gas only), one block:

  (a) one Simulation.gather() of the three shipped variables (gas.prim.density, .velocity, .pressure: five components;
      artemis_hip_pack_fields into the staging buffer, one d2h copy, synchronised) in double and in float, and one
      Simulation.write_fields() of them to a local temporary directory, each as the median of repeated calls after warm-up
      calls, on the state after the warm-up cycles -- next to Simulation.field("gas.prim", 0), the route there was before;
  (b) zone-cycles/s of --cycles cycles (one evolve() call, the driver's own device-synchronised wall clock) with outputs
      off; with --parent DIR the same loop also runs on the library and Python package of another checkout (the parent
      commit, built there) in a process of its own, alternating, --repeats times each.

Prints one JSON object; nothing is asserted.  A machine without a GPU fails in capi.load() / Simulation().

    python3 scripts/fields_cost.py [--n 256] [--cycles 200] [--repeats 3] [--parent DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from history_cost import loop, overrides  # noqa: E402

SHIPPED = ["gas.prim.density", "gas.prim.velocity", "gas.prim.pressure"]


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
    res = dict(n=args.n, cycles=args.cycles, source_sha=capi.source_sha(), variables=SHIPPED)
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
    a = dict(gather_f8_ms=timed(lambda: s.gather(SHIPPED), 2, args.calls), gather_f4_ms=timed(lambda: s.gather(SHIPPED, single=True), 2, args.calls),
             bytes_read=5 * 8 * zones, bytes_out_f8=5 * 8 * zones, bytes_out_f4=5 * 4 * zones)
    with tempfile.TemporaryDirectory() as d:
        a["write_fields_f8_ms"] = timed(lambda: s.write_fields(os.path.join(d, "dump.fld"), SHIPPED), 1, max(3, args.calls // 2))
        a["write_fields_f4_ms"] = timed(lambda: s.write_fields(os.path.join(d, "dump4.fld"), SHIPPED, single=True), 1, max(3, args.calls // 2))
    a["field_gas_prim_ms"] = timed(lambda: s.field("gas.prim", 0), 1, 3)  # (whole-mesh PrimToCons once, then 6 arrays with ghosts)
    res["a"] = a
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
    res["b"] = dict(outputs_off=[r["zone_cycles_per_s"] for r in off], parent_outputs_off=[r["zone_cycles_per_s"] for r in parent],
                    parent_source_sha=parent[0]["source_sha"] if parent else None)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
