#!/usr/bin/env python3
"""What a history row costs, and what switched-on outputs cost the time loop (DESIGN.md "Deck-driven outputs").

One MI355X, the flagship 256^3 Sedov deck of bench.py (inputs/blast/blast.in, Cartesian, gas only):

  (a) one Simulation.history_device() call (device sums + the d2h copy of the 6 doubles, synchronised) and one
      Simulation.history() call (whole-mesh PrimToCons, download of the conserved arrays, host loop), each as the median
      of repeated calls after warm-up calls, on the state after the warm-up cycles;
  (b) zone-cycles/s of --cycles cycles (one evolve() call, the driver's own device-synchronised wall clock) with outputs
      off and with an `hst` block that fires roughly every --every cycles, alternating, --repeats times each; with --parent
      DIR the outputs-off loop also runs on the library and Python package of another checkout (the parent commit, built
      there) in a process of its own, alternating with the others.

Prints one JSON object; nothing is asserted.  A machine without a GPU fails in capi.load() / Simulation().

    python3 scripts/history_cost.py [--n 256] [--cycles 200] [--every 20] [--repeats 3] [--parent DIR] [--out FILE]
    python3 scripts/history_cost.py --loop-only --root DIR ...     (internal: the outputs-off loop of the checkout at DIR)
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


def overrides(n, extra=()):
    half = n / 256.0  # dx = 2/256 whatever the size, like bench.py
    ov = ["gas/riemann=hllc", "problem/symmetry=spherical", "problem/radius=0.03", "problem/samples=0",
          "parthenon/time/tlim=-1.0", "parthenon/time/nlim=-1"]
    for d in (1, 2, 3):
        ov += [f"parthenon/mesh/nx{d}={n}", f"parthenon/meshblock/nx{d}={n}", f"parthenon/mesh/x{d}min={-half}",
               f"parthenon/mesh/x{d}max={half}"]
    return ov + list(extra)


def loop(Simulation, deck, n, warm, cycles, extra=(), outdir=None):
    """zone-cycles/s of `cycles` cycles after `warm` warm-up cycles; also the mean dt of the timed cycles"""
    s = Simulation(deck, overrides(n, extra))
    if outdir is not None:
        s.enable_outputs(outdir)
    s.evolve(warm)
    t0 = s.time
    assert s.evolve(cycles) == cycles
    wall = s.last_wall_seconds
    res = dict(zone_cycles_per_s=s.total_zones * cycles / wall, wall_s=wall, mean_dt=(s.time - t0) / cycles, time=s.time, dt=s.dt)
    if outdir is not None:
        res["rows"] = [b["written"] for b in s.outputs()["blocks"]]
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="timed history_device() calls (history(): a quarter of them)")
    ap.add_argument("--parent", default=None, help="another checkout (built) whose outputs-off loop is timed too")
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()

    sys.path.insert(0, args.root)
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    deck = os.path.join(args.root, "inputs", "blast", "blast.in")
    if args.loop_only:
        print(json.dumps(dict(loop(Simulation, deck, args.n, args.warm, args.cycles), source_sha=capi.source_sha())))
        return

    res = dict(n=args.n, cycles=args.cycles, source_sha=capi.source_sha())
    # (a) one row's worth of sums, device against host
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
        return out
    td = timed(s.history_device, 3, args.calls)
    th = timed(s.history, 1, max(3, args.calls // 4))
    dev, host = s.history_device(), s.history()
    res["a"] = dict(history_device_ms=dict(median=1e3 * statistics.median(td), min=1e3 * min(td), max=1e3 * max(td), calls=len(td)),
                    history_ms=dict(median=1e3 * statistics.median(th), min=1e3 * min(th), max=1e3 * max(th), calls=len(th)),
                    bytes_read=5 * 8 * s.total_zones, max_rel_difference=float(max(abs(dev - host)[[0, 4, 5]] / abs(host)[[0, 4, 5]])))
    s.close()
    # (b) the loop with outputs off / on (/ on the parent's library), alternating
    off, on, parent = [], [], []
    mean_dt = loop(Simulation, deck, args.n, args.warm, args.cycles)["mean_dt"]  # (also warms every shape of the loop)
    block = ["parthenon/output0/file_type=hst", "parthenon/output0/dt=%r" % (args.every * mean_dt)]
    for _ in range(args.repeats):
        off.append(loop(Simulation, deck, args.n, args.warm, args.cycles))
        with tempfile.TemporaryDirectory() as d:
            on.append(loop(Simulation, deck, args.n, args.warm, args.cycles, block, d))
        if args.parent:
            cmd = [sys.executable, os.path.abspath(__file__), "--loop-only", "--root", os.path.abspath(args.parent), "--n", str(args.n),
                   "--warm", str(args.warm), "--cycles", str(args.cycles)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=600)
            assert p.returncode == 0, "the parent's loop failed"
            parent.append(json.loads(p.stdout.decode().strip().split("\n")[-1]))
    assert all(r["time"] == off[0]["time"] and r["dt"] == off[0]["dt"] for r in off + on + parent), "the runs took different steps"
    res["b"] = dict(hst_dt=args.every * mean_dt, outputs_off=[r["zone_cycles_per_s"] for r in off],
                    outputs_on=[r["zone_cycles_per_s"] for r in on], rows_written=[r["rows"] for r in on],
                    parent_outputs_off=[r["zone_cycles_per_s"] for r in parent],
                    parent_source_sha=parent[0]["source_sha"] if parent else None)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
