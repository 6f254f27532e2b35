"""Worker of tests/test_record_integrals_cpu.py: one rank of a gloo world (or a process alone) running the product's host driver
against the CPU test double.  It attaches an integral recorder with the windows of <out>.windows.npy, evolves the case in one
call and leaves, in <out>.rank<r>.npz, the rows its rank recorded -- cycle, time, dt, integrals -- and its zone count."""
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
    rec = sim.record_integrals(every=spec["every"], capacity=spec["capacity"], windows=np.load(spec["out"] + ".windows.npy"))
    assert sim.evolve(spec["cycles"]) == spec["cycles"]
    ts = rec.read()
    sim.L.artemis_sim_local_zones.restype = C.c_long
    np.savez(spec["out"] + ".rank%d.npz" % rank, cycle=ts.cycle, time=ts.time, dt=ts.dt, integrals=ts.integrals,
             zones=sim.L.artemis_sim_local_zones(sim.h))
    rec.close()
    sim.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
