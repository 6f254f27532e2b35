"""Worker of tests/test_fields_cpu.py: one rank (of a gloo world, or alone) running the product's host driver against the
CPU test double through a list of actions.  The double does not define artemis_hip_pack_fields, so every gather goes
through the driver's host loop over the downloaded primitives.  Actions, as JSON lists:
    ["create"] | ["enable", dir] | ["evolve", n] | ["close"]
    ["track", tag]               evolve(1) until the run ends; records (ncycle, time, dt) per cycle in the JSON result and
                                 the interiors of field("gas.prim") of every local block per cycle in <out>.<tag>.rank<r>.npz
                                 (key "c<ncycle>": [nblocks, 6 ns, nz, ny, nx])
    ["snap", tag]                clock and outputs() as they are now
    ["state", tag]               whole field("gas.prim") of every local block -> <out>.<tag>.rank<r>.npz (key "prim")
    ["gather", tag, variables, single]   Simulation.gather -> <out>.<tag>.rank<r>.npz (key "a")
    ["write", path, variables, single]   Simulation.write_fields"""
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


def prims(sim, interior):
    a = np.stack([sim.field("gas.prim", b) for b in range(sim.nblocks)])
    return sim.interior(a) if interior else a


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
    meta, sim = {}, None

    def npz(tag):
        return spec["out"] + ".%s.rank%d.npz" % (tag, rank)

    for act in spec["actions"]:
        op = act[0]
        if op == "create":
            sim = Simulation(os.path.join(ROOT, "inputs", *spec["deck"]), spec["overrides"], comm=comm, lib=lib)
        elif op == "enable":
            sim.enable_outputs(act[1])
        elif op == "evolve":
            sim.evolve(act[1])
        elif op == "track":
            rows, arrays = [], {}
            while True:
                rows.append(dict(ncycle=sim.ncycle, time=sim.time, dt=sim.dt))
                arrays["c%d" % sim.ncycle] = prims(sim, True)
                if sim.evolve(1) != 1:
                    break
            meta[act[1]] = rows
            np.savez(npz(act[1]), **arrays)
        elif op == "snap":
            meta[act[1]] = dict(time=sim.time, dt=sim.dt, ncycle=sim.ncycle, outputs=sim.outputs(), nblocks=sim.nblocks,
                                bounds=[sim.block_bounds(b) for b in range(sim.nblocks)])
        elif op == "state":
            np.savez(npz(act[1]), prim=prims(sim, False))
        elif op == "gather":
            np.savez(npz(act[1]), a=sim.gather(act[2], single=act[3]))
        elif op == "write":
            sim.write_fields(act[1], act[2], single=act[3])
        elif op == "close":
            sim.close()
            sim = None
        else:
            raise ValueError(op)
    with open(spec["out"] + ".rank%d.json" % rank, "w") as f:
        json.dump(meta, f)
    if sim is not None:
        sim.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
