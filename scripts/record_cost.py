#!/usr/bin/env python3
"""What a recorder costs the time loop, and what it saves ("recorded time series").

One MI355X, the 256^3 Sedov deck of bench.py (one block), --warm cycles first, then `evolve(--cycles)` timed by the wall clock
around the call (it synchronises the device at both ends), --repeats times per process.  Four modes, each a process of its
own:

  plain      evolve(cycles) with no recorder.  With --root DIR the library and the Python package of another checkout run
             (the parent commit, built there): (a); this commit: (b)
  record     a recorder of gas.prim.density on the 256^2 midplane lattice, every cycle, attached before the call: (c)
  stepping   the only way a library without recorders produces that series: cycles x (evolve(1) + plan.values): (d);
             it runs on the parent with --root

Every process prints one JSON object and writes it to --out;

    python3 scripts/record_cost.py --combine a1.json b1.json c1.json d1.json a2.json ...

writes profiles/record_cost.json from such files (the processes of the two libraries alternating in one job): the median
zone-cycles/s of every process, and per mode the median, minimum and maximum over the processes.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from history_cost import overrides  # noqa: E402

DENSITY = ["gas.prim.density"]


def combine(files, out):
    runs = [json.load(open(f)) for f in files]
    res = dict(note="scripts/record_cost.py: zone-cycles/s of evolve(cycles) on the 256^3 Sedov by the wall clock; every mode in "
                    "processes of its own, the parent's and this commit's libraries alternating in one job", runs=runs, summary={})
    for label in ("a_parent", "b_no_recorder", "c_recording", "d_parent_stepping"):
        mine = [statistics.median(r["zone_cycles_per_s"]) for r in runs if r["label"] == label]
        if mine:
            res["summary"][label] = dict(median=statistics.median(mine), min=min(mine), max=max(mine), processes=len(mine))
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res["summary"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["plain", "record", "stepping"])
    ap.add_argument("--label", default=None)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library and package run")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", nargs="+", default=None)
    args = ap.parse_args()
    if args.combine:
        return combine(args.combine, args.out or os.path.join(os.path.dirname(HERE), "profiles", "record_cost.json"))
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import numpy as np
    from artemis_amd import capi
    from artemis_amd import sample as smp
    from artemis_amd.driver import Simulation
    s = Simulation(os.path.join(root, "inputs", "blast", "blast.in"), overrides(args.n))
    s.evolve(args.warm)
    b = np.array([s.block_bounds(q) for q in range(s.nblocks)]).reshape(-1, 6)
    lo, hi = b[:, 0::2].min(axis=0), b[:, 1::2].max(axis=0)
    dz, k = (hi[2] - lo[2]) / args.n, args.n // 2
    pts = smp.lattice((lo[0], lo[1], lo[2] + k * dz), (hi[0], hi[1], lo[2] + (k + 1) * dz), (args.n, args.n, 1))
    res = dict(label=args.label or args.mode, mode=args.mode, source_sha=capi.source_sha(), has_record=hasattr(s, "record"), zones=s.total_zones,
               cycles=args.cycles, points=len(pts), zone_cycles_per_s=[], seconds=[])
    rec = s.record(pts, DENSITY) if args.mode == "record" else None
    plan = s.sample_plan(pts) if args.mode == "stepping" else None
    for rep in range(args.repeats + 1):  # (the first call is a warm-up of the mode itself and is not kept)
        t0 = time.perf_counter()
        if args.mode == "stepping":
            rows = []
            for _ in range(args.cycles):
                s.evolve(1)
                rows.append(plan.values(DENSITY))
        else:
            assert s.evolve(args.cycles) == args.cycles
        dt = time.perf_counter() - t0
        if rec is not None:
            ts = rec.read(clear=True)
            assert len(ts.cycle) == args.cycles and ts.cycle[-1] == s.ncycle and ts.time[-1] == s.time
            res["rows_bytes"] = int(ts.values.nbytes)
        if rep:
            res["seconds"].append(dt), res["zone_cycles_per_s"].append(s.total_zones * args.cycles / dt)
    if rec is not None:  # the last row is the sample of the final state
        assert np.array_equal(ts.values[-1].view(np.uint64), s.sample_plan(pts).values(DENSITY).view(np.uint64))
        res["capacity"] = rec.capacity
    s.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
