#!/usr/bin/env python3
"""What a field dump at a coarser refinement level costs next to the full one, and that the time loop is what it was
(DESIGN.md "Field outputs at a level").

One MI355X, the flagship 256^3 Sedov deck of bench.py (inputs/blast/blast.in, Cartesian, gas only), one block:

  (a) Simulation.gather() of the three shipped variables (gas.prim.density, .velocity, .pressure: five components) at level
      None (artemis_hip_pack_fields), -1 and -2 (artemis_hip_pack_fields_level: 128^3 and 64^3 zones leave the device), in
      double and in float, and Simulation.write_fields() at the same levels to a local temporary directory: each the median
      of --calls calls after 2 warm-up calls, on the state after the warm-up cycles.  These are CALL times -- kernel, the
      device-to-host copy into pageable memory, synchronisation, and for write_fields the file -- not kernel times;
  (b) zone-cycles/s of --cycles cycles (one evolve() call, the driver's own device-synchronised wall clock) with outputs
      off; with --parent DIR the same loop also runs on the library and Python package of another checkout (the parent
      commit, built there) in a process of its own, alternating, --repeats times each; the runs must take bit-identical steps.

Prints one JSON object.  A machine without a GPU fails in capi.load() / Simulation().

    python3 scripts/fields_level_cost.py [--n 256] [--cycles 200] [--repeats 3] [--parent DIR] [--out FILE]
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
LEVELS = (None, -1, -2)


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
               note="call times (kernel + device-to-host copy + synchronisation [+ file]), not kernel times")
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
    a = dict(bytes_read=5 * 8 * zones)
    with tempfile.TemporaryDirectory() as d:
        for level in LEVELS:
            tag = "full" if level is None else "level%d" % level
            out_zones = zones if level is None else zones >> (3 * -level)
            a[tag] = dict(bytes_out_f8=5 * 8 * out_zones, bytes_out_f4=5 * 4 * out_zones,
                          gather_f8_ms=timed(lambda: s.gather(SHIPPED, level=level), 2, args.calls),
                          gather_f4_ms=timed(lambda: s.gather(SHIPPED, single=True, level=level), 2, args.calls),
                          write_fields_f8_ms=timed(lambda: s.write_fields(os.path.join(d, tag + ".fld"), SHIPPED, level=level), 2, args.calls),
                          write_fields_f4_ms=timed(lambda: s.write_fields(os.path.join(d, tag + "4.fld"), SHIPPED, single=True, level=level),
                                                   2, args.calls))
    # the within-job check: the levelled gather against the full one of the same job
    a["level-1_over_full_f8"] = a["level-1"]["gather_f8_ms"]["median"] / a["full"]["gather_f8_ms"]["median"]
    a["level-2_over_full_f8"] = a["level-2"]["gather_f8_ms"]["median"] / a["full"]["gather_f8_ms"]["median"]
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
                    parent_source_sha=parent[0]["source_sha"] if parent else None, bit_identical_steps=True)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
