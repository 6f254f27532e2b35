#!/usr/bin/env python3
"""What an integral recorder costs the time loop, and what it saves ("recorded history integrals").

One MI355X, the 256^3 Sedov deck of bench.py (one block), --warm cycles first, then `evolve(--cycles)` timed by the wall clock
around the call (it synchronises the device at both ends), --repeats times per process.  Every mode is a process of its own:

  plain      evolve(cycles) with no recorder.  With --root DIR the library and the Python package of another checkout run
             (the parent commit, built there): (a); this commit: (b)
  record     record_integrals(every=--every) with --windows windows, attached before the call: (c) set 0 alone every cycle,
             (c') set 0 and four windows, (c'') every = 10
  stepping   the only way a library without integral recorders produces the series: cycles x (evolve(1) + history_device()):
             (d); it runs on the parent with --root

Every process prints one JSON object and writes it to --out;

    python3 scripts/record_integrals_cost.py --combine a1.json b1.json c1.json ... a2.json ...

writes profiles/record_integrals_cost.json from such files (the processes of the two libraries alternating in one job): the
median zone-cycles/s of every process, and per label the median, minimum and maximum over the processes.
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

LABELS = ("a_parent", "b_nothing_attached", "c_set0_every_cycle", "c1_set0_and_four_windows", "c2_set0_every_10", "d_parent_stepping")


def combine(files, out):
    runs = [json.load(open(f)) for f in files]
    res = dict(note="scripts/record_integrals_cost.py: zone-cycles/s of evolve(cycles) on the 256^3 Sedov by the wall clock; every mode "
                    "in processes of its own, the parent's and this commit's libraries alternating in one job", runs=runs, summary={})
    for label in LABELS:
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
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--windows", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", nargs="+", default=None)
    args = ap.parse_args()
    if args.combine:
        return combine(args.combine, args.out or os.path.join(os.path.dirname(HERE), "profiles", "record_integrals_cost.json"))
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import numpy as np
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    s = Simulation(os.path.join(root, "inputs", "blast", "blast.in"), overrides(args.n))
    s.evolve(args.warm)
    b = np.array([s.block_bounds(q) for q in range(s.nblocks)]).reshape(-1, 6)
    lo, hi = b[:, 0::2].min(axis=0), b[:, 1::2].max(axis=0)
    # nested boxes about the centre: shells of the blast, each cutting tiles along all three directions
    win = np.array([[[0.5 * (lo[d] + hi[d]) - f * (hi[d] - lo[d]), 0.5 * (lo[d] + hi[d]) + f * (hi[d] - lo[d])] for d in range(3)]
                    for f in (0.0626, 0.1251, 0.2501, 0.3751, 0.4376, 0.4688, 0.4844)[:args.windows]]).reshape(-1, 3, 2)
    res = dict(label=args.label or args.mode, mode=args.mode, source_sha=capi.source_sha(), has_record_integrals=hasattr(s, "record_integrals"),
               zones=s.total_zones, cycles=args.cycles, every=args.every, windows=args.windows, zone_cycles_per_s=[], seconds=[])
    rec = s.record_integrals(every=args.every, windows=win) if args.mode == "record" else None
    for rep in range(args.repeats + 1):  # (the first call is a warm-up of the mode itself and is not kept)
        t0 = time.perf_counter()
        if args.mode == "stepping":
            rows = []
            for _ in range(args.cycles):
                s.evolve(1)
                rows.append(s.history_device())
        else:
            assert s.evolve(args.cycles) == args.cycles
        dt = time.perf_counter() - t0
        if rec is not None:
            ts = rec.read(clear=True)
            assert len(ts.cycle) == args.cycles // args.every and ts.cycle[-1] == s.ncycle and ts.time[-1] == s.time
        if rep:
            res["seconds"].append(dt), res["zone_cycles_per_s"].append(s.total_zones * args.cycles / dt)
    if rec is not None:  # the last row is the history of the final state
        assert np.array_equal(ts.integrals[-1, 0].view(np.uint64), s.history_device().view(np.uint64))
        res["capacity"] = rec.capacity
    s.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
