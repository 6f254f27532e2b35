"""Worker of tests/test_restart_cpu.py: one rank (of a gloo world, or alone) running the product's host driver against
the CPU test double through a list of actions, so one process can run a straight reference, save a checkpoint and
continue from it.  Actions, as JSON lists:
    ["create"] | ["restore", path, [overrides]] | ["evolve", n] | ["path", "fused"|"unfused"] | ["dump", tag(, nbody)]
    ["save", path] | ["close"] | ["refuse", tag, path, [overrides]] | ["describe", tag, path]
"dump" records the clock and, per block, bounds, level and the whole arrays of every field under `tag`; "refuse" records
the message of the RuntimeError a restore must raise (or None if it did not) and goes on."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def dump(sim, tag, meta, arrays, nbody=True):
    m = dict(time=sim.time, dt=sim.dt, ncycle=sim.ncycle, nblocks=sim.nblocks, stage_kernel=sim.stage_kernel,
             remeshes=sim.remeshes, levels=[sim.block_level(b) for b in range(sim.nblocks)],
             interior=[sim.ks, sim.ke, sim.js, sim.je, sim.is_, sim.ie], errors=list(sim.errors()),
             nblocks_global=sim.nblocks_global)
    if nbody:  # (reading the sums moves the device accumulators into the host rows: a run that is read regroups its additions)
        m["nbody"] = sim.nbody_force().tolist()
    fields = ["gas.prim", "gas.cons"] + (["dust.prim", "dust.cons"] if sim.ns_dust else [])
    m["fields"] = fields
    for b in range(sim.nblocks):
        arrays["%s.bounds.%d" % (tag, b)] = np.array(sim.block_bounds(b))
        for f in fields:
            arrays["%s.%s.%d" % (tag, f, b)] = sim.field(f, b)
    meta[tag] = m


def main():
    spec = json.loads(sys.argv[1])
    from artemis_amd.driver import Simulation, TorchComm
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libartemis_cpudouble.so"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    comm = None
    if world > 1:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["MASTER_PORT"],
                                rank=rank, world_size=world)
        comm = TorchComm(torch.device("cpu"))
    meta, arrays, sim = {}, {}, None
    for act in spec["actions"]:
        op = act[0]
        if op == "create":
            sim = Simulation(os.path.join(ROOT, "inputs", *spec["deck"]), spec["overrides"], comm=comm, lib=lib)
        elif op == "restore":
            sim = Simulation.restore(act[1], act[2], comm=comm, lib=lib)
        elif op == "evolve":
            sim.evolve(act[1])
        elif op == "path":
            sim.set_path(act[1])
        elif op == "dump":
            dump(sim, act[1], meta, arrays, *act[2:])
        elif op == "save":
            sim.save(act[1])
        elif op == "close":
            sim.close()
            sim = None
        elif op == "refuse":
            try:
                Simulation.restore(act[2], act[3], comm=comm, lib=lib).close()
                meta[act[1]] = None
            except RuntimeError as e:
                meta[act[1]] = str(e)
        elif op == "describe":
            meta[act[1]] = Simulation.describe_checkpoint(act[2], lib=lib)
        else:
            raise ValueError(op)
    np.savez(spec["out"] + ".rank%d.npz" % rank, meta=json.dumps(meta), **arrays)
    if sim is not None:
        sim.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
