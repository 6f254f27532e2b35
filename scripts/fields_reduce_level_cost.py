#!/usr/bin/env python3
"""What a reduced field output on a chosen level costs on a mesh of many small blocks, and that the time loop is what it was
(DESIGN.md "Reduced field outputs on a chosen level").

One MI355X, one job:

  (a) the four-level disk with a planet of `bench.py --workload disk_amr` (inputs/disk/disk_nbody_cyl.in, cylindrical,
      adaptive, blocks of 16^3: thousands of them), after --warm cycles, the three shipped variables (gas.prim.density,
      .velocity, .pressure: five components): Simulation.gather(reduce="x3", reduce_level=L) for L = the coarsest and the
      finest level of the mesh (artemis_hip_reduce_fields_level: the reduce passes, then resample_reduced_kernel in launches
      of 192 blocks), against gather(level=L) (artemis_hip_pack_fields_level) and gather() (artemis_hip_pack_fields) of the
      same state, in double and in float: median, minimum and maximum of --calls calls after 2 warm-up calls.  These are
      CALL times -- kernels, the device-to-host copy into pageable memory, synchronisation -- not kernel times.  The question
      is whether the reduced gather stays near one read of the primitives where launch latency and the by-value batches count;
  (b) zone-cycles/s of --cycles cycles of the 256^3 Sedov deck of bench.py (one evolve() call, the driver's own
      device-synchronised wall clock) with outputs off; with --parent DIR the same loop also runs on the library and Python
      package of another checkout (the parent commit, built there) in a process of its own, alternating, --repeats times
      each; the runs must take bit-identical steps (asserted).

Prints one JSON object.  A machine without a GPU fails in capi.load() / Simulation().

    python3 scripts/fields_reduce_level_cost.py [--only a|b] [--cycles 200] [--repeats 3] [--parent DIR] [--out FILE]

A job runs each part in a process of its own under its own time limit, the second only after the first succeeded:

    timeout -k 10 300 python3 scripts/fields_reduce_level_cost.py --only a --out a.json && \\
    timeout -k 10 300 python3 scripts/fields_reduce_level_cost.py --only b --parent DIR --out b.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fields_reduce_cost import SHIPPED, timed  # noqa: E402
from history_cost import loop  # noqa: E402

# bench.py --workload disk_amr on one GPU, blocks of 16^3
DISK_AMR = ["parthenon/mesh/nx1=128", "parthenon/mesh/nx2=128", "parthenon/mesh/nx3=16", "parthenon/mesh/x3min=-0.2",
            "parthenon/mesh/x3max=0.2", "parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=16",
            "parthenon/mesh/refinement=adaptive", "parthenon/mesh/numlevel=4", "parthenon/mesh/derefine_count=5",
            "gas/refine_field=pressure", "gas/refine_type=gradient", "gas/refine_thr=2.0",
            "physics/rotating_frame=true", "rotating_frame/omega=1.0",
            "physics/dust=true", "dust/nspecies=1", "dust/cfl=0.3", "dust/reconstruct=plm", "dust/riemann=hlle",
            "dust/dfloor=1e-10", "physics/drag=true", "drag/type=simple_dust", "dust/stopping_time/type=constant",
            "dust/stopping_time/tau=0.1", "dust/sizes=1.0",
            "nbody/particle2/mass=1.0e-2", "nbody/particle2/couple=1", "nbody/particle2/soft/type=plummer",
            "nbody/particle2/soft/radius=0.03", "nbody/particle2/initialize/x=1.0", "nbody/particle2/initialize/vy=1.0",
            "parthenon/time/nlim=-1"]


def part_a(Simulation, warm, calls):
    s = Simulation(os.path.join(ROOT, "inputs", "disk", "disk_nbody_cyl.in"), DISK_AMR)
    s.evolve(warm)
    levels = [s.block_level(b) for b in range(s.nblocks)]
    res = dict(blocks=s.nblocks, zones=s.total_zones, block=[16, 16, 16], bytes_read=5 * 8 * s.total_zones,
               blocks_per_level={str(l): levels.count(l) for l in sorted(set(levels))})

    def both(f):
        return dict(gather_f8_ms=timed(lambda: f(False), 2, calls), gather_f4_ms=timed(lambda: f(True), 2, calls))
    out = s.gather(SHIPPED)
    res["full"] = dict(bytes_out_f8=out.nbytes, **both(lambda single: s.gather(SHIPPED, single=single)))
    for L in (min(levels), max(levels)):
        lev = s.gather(SHIPPED, level=L)
        red = s.gather(SHIPPED, reduce="x3", reduce_level=L)
        row = dict(level=dict(bytes_out_f8=sum(x.nbytes for x in lev), **both(lambda single: s.gather(SHIPPED, single=single, level=L))),
                   reduce_x3=dict(bytes_out_f8=sum(x.nbytes for x in red),
                                  **both(lambda single: s.gather(SHIPPED, single=single, reduce="x3", reduce_level=L))))
        for k in ("level", "reduce_x3"):
            row[k]["over_full_f8"] = row[k]["gather_f8_ms"]["median"] / res["full"]["gather_f8_ms"]["median"]
        res["L%d" % L] = row
    res["reduce_x3_own_levels"] = dict(note="gather(reduce='x3'): every block on its own zone size, the existing kernels alone",
                                       **both(lambda single: s.gather(SHIPPED, single=single, reduce="x3")))
    s.close()
    return res


def part_b(Simulation, args):
    deck = os.path.join(ROOT, "inputs", "blast", "blast.in")
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
    return dict(n=args.n, cycles=args.cycles, outputs_off=[r["zone_cycles_per_s"] for r in off],
                parent_outputs_off=[r["zone_cycles_per_s"] for r in parent],
                parent_source_sha=parent[0]["source_sha"] if parent else None, bit_identical_steps=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["a", "b"], default=None)
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
    res = dict(source_sha=capi.source_sha(), variables=SHIPPED,
               note="call times (kernels + device-to-host copy + synchronisation), not kernel times")
    if args.only in (None, "a"):
        res["a"] = part_a(Simulation, args.warm, args.calls)
    if args.only in (None, "b"):
        res["b"] = part_b(Simulation, args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
