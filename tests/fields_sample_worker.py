"""Worker of tests/test_fields_sample_cpu.py: one rank of a gloo world (or a process alone) running the product's host driver
against the CPU test double.  It evolves the case, samples the points of <out>.points.npy and leaves, in <out>.rank<r>.npz,
what its rank answers: block and zone of every point, the bounds and level of every local block, and the values in double
and in float."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402


def main():
    spec = json.loads(sys.argv[1])
    from artemis_amd.driver import Simulation, TorchComm
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libartemis_cpudouble.so"))
    comm = None
    if world > 1:
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["MASTER_PORT"], rank=rank, world_size=world)
        comm = TorchComm(torch.device("cpu"))
    sim = Simulation(os.path.join(ROOT, "inputs", *spec["deck"]), spec["overrides"], comm=comm, lib=lib)
    sim.evolve(spec["cycles"])
    points = np.load(spec["out"] + ".points.npy")
    plan = sim.sample_plan(points)
    np.savez(spec["out"] + ".rank%d.npz" % rank, block=plan.block, zone=plan.zone,
             bounds=np.array([sim.block_bounds(b) for b in range(sim.nblocks)]).reshape(-1, 6),
             values=plan.values(spec["variables"]), single=plan.values(spec["variables"], single=True), ncycle=sim.ncycle)
    plan.close()
    sim.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
