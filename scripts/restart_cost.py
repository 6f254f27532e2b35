#!/usr/bin/env python3
"""What a checkpoint costs next to a cycle: one save and one restore of bench.py's `disk_amr` mesh (disk_nbody_cyl.in +
planet + dust + drag + four adaptive levels, 7 064 blocks of 16^3 on one MI355X), with where the time goes -- device
copies, checksums, file writes or reads -- as the driver itself accounts it (artemis_sim_checkpoint_seconds).  Written
down, not gated: a report for profiles/restart_cost.txt.
    python scripts/restart_cost.py [--dir DIRECTORY] [--cycles N] [--out FILE]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bench.py --workload disk_amr, one GPU, 16^3 blocks
OVERRIDES = ["parthenon/mesh/nx1=128", "parthenon/mesh/nx2=128", "parthenon/mesh/nx3=16", "parthenon/mesh/x3min=-0.2",
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None, help="where the checkpoint goes (default: a temporary directory, removed afterwards)")
    ap.add_argument("--cycles", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import numpy as np
    from artemis_amd.driver import Simulation
    work = args.dir or tempfile.mkdtemp(prefix="artemis_restart_cost_")
    ck = os.path.join(work, "checkpoint")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    t0 = time.perf_counter()
    s = Simulation(os.path.join(ROOT, "inputs", "disk", "disk_nbody_cyl.in"), OVERRIDES)
    say("mesh: %d blocks of %d x %d x %d zones (with ghosts), %d gas + %d dust species; built in %.2f s"
        % (s.nblocks_global, s.ni, s.nj, s.nk, s.ns_gas, s.ns_dust, time.perf_counter() - t0))
    s.evolve(3)
    t0 = time.perf_counter()  # (an adaptive run steps one cycle per inner call: evolve() returns device-synchronised)
    s.evolve(args.cycles)
    cycle = (time.perf_counter() - t0) / args.cycles
    say("cycle: %.1f ms (mean of %d, remesh checks included)" % (1e3 * cycle, args.cycles))
    s.save(ck)
    tot, copy, chk, io = s.checkpoint_seconds()
    size = sum(os.path.getsize(os.path.join(ck, f)) for f in os.listdir(ck))
    say("save: %.3f s = %.1f cycle-times for %.2f GB: device copies %.3f s, checksums %.3f s, file writes %.3f s, rest %.3f s"
        % (tot, tot / cycle, size / 1e9, copy, chk, io, tot - copy - chk - io))
    ref = [s.field("gas.prim", b) for b in (0, s.nblocks // 2, s.nblocks - 1)]
    clock = (s.time, s.dt, s.ncycle, s.remeshes)
    s.close()
    r = Simulation.restore(ck)
    tot, copy, chk, io = r.checkpoint_seconds()
    say("restore: %.3f s = %.1f cycle-times: file reads %.3f s, checksums %.3f s, device copies %.3f s, building the state "
        "from the deck and the rest %.3f s" % (tot, tot / cycle, io, chk, copy, tot - copy - chk - io))
    same = clock == (r.time, r.dt, r.ncycle, r.remeshes) and all(
        np.array_equal(a, r.field("gas.prim", b)) for a, b in zip(ref, (0, r.nblocks // 2, r.nblocks - 1)))
    say("restored state equals the saved one (clock and three sampled blocks): %s" % same)
    r.close()
    if args.dir is None:
        shutil.rmtree(work, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
