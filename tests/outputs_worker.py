"""Worker of tests/test_outputs_cpu.py: one rank (of a gloo world, or alone) running the product's host driver against
the CPU test double through a list of actions.  The double does not define artemis_hip_history_sums, so history rows come
from the driver's host sum.  Actions, as JSON lists:
    ["create"] | ["restore", path, [overrides]] | ["enable", dir] | ["evolve", n] | ["close"]
    ["track", tag]     evolve(1) until the run ends; records per cycle (ncycle, time, dt, nblocks_global) and, per entry of
                       the history layout, this rank's bound factor max |M_d / D| (1 for masses and energies)
    ["snap", tag]      clock, outputs(), history_device() and history() as they are now
`dir` may contain "{rank}"."""
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


def factors(sim):
    """max |M_d / D| over this rank's interior zones for every momentum of the history layout, 1 elsewhere"""
    nsg, nsd = sim.ns_gas, sim.ns_dust
    f = np.ones(6 * nsg + 4 * nsd)
    for b in range(sim.nblocks):
        g = sim.interior(sim.field("gas.cons", b)) if nsg else None
        d = sim.interior(sim.field("dust.cons", b)) if nsd else None
        for n in range(nsg):
            for q in range(3):
                v = np.abs(g[nsg + 3 * n + q] / g[n]).max()
                f[6 * n + 1 + q] = v if b == 0 else max(f[6 * n + 1 + q], v)
        for n in range(nsd):
            for q in range(3):
                v = np.abs(d[nsd + 3 * n + q] / d[n]).max()
                f[6 * nsg + 4 * n + 1 + q] = v if b == 0 else max(f[6 * nsg + 4 * n + 1 + q], v)
    return f


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
    for act in spec["actions"]:
        op = act[0]
        if op == "create":
            sim = Simulation(os.path.join(ROOT, "inputs", *spec["deck"]), spec["overrides"], comm=comm, lib=lib)
        elif op == "restore":
            sim = Simulation.restore(act[1], act[2], comm=comm, lib=lib)
        elif op == "enable":
            sim.enable_outputs(act[1].replace("{rank}", str(rank)))
        elif op == "evolve":
            sim.evolve(act[1])
        elif op == "track":
            rows = [dict(ncycle=sim.ncycle, time=sim.time, dt=sim.dt, nblocks_global=sim.nblocks_global,
                         factors=factors(sim).tolist())]
            while sim.evolve(1) == 1:
                rows.append(dict(ncycle=sim.ncycle, time=sim.time, dt=sim.dt, nblocks_global=sim.nblocks_global,
                                 factors=factors(sim).tolist()))
            meta[act[1]] = rows
        elif op == "snap":
            meta[act[1]] = dict(time=sim.time, dt=sim.dt, ncycle=sim.ncycle, outputs=sim.outputs(), total_zones=sim.total_zones,
                                history_device=sim.history_device().tolist(), history=sim.history().tolist(),
                                remeshes=sim.remeshes, nblocks_global=sim.nblocks_global)
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
