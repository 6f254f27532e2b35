"""Worker of tests/test_fields_derived_cpu.py: one rank (of a gloo world, or alone) running the product's host driver against
the CPU test double through a list of actions; `reference` also serves tests/test_fields_derived.py.  Actions, as JSON lists:
    ["create"] | ["evolve", n] | ["close"] | ["save", path] | ["restore", path]
    ["snap", tag]                clock, and level and bounds of every local block
    ["state", tag]               whole field("gas.prim") of every local block -> <out>.<tag>.rank<r>.npz (key "prim")
    ["write", path, variables]   Simulation.write_fields (double)
    ["check", tag, variables]    gather(variables) of the derived names against the numpy definition (fields_derived_ref.py)
                                 formed from field() of every local block: records {"same": bool, "blocks": n}
    ["roll", variables]          scatter(variables, gather(variables) with the three velocity components of every species
                                 rolled by one): a new state that depends on the old one zone by zone only"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402


def reference(sim, names, coordinates):
    """[nblocks, ncomp, nz, ny, nx] of the derived `names` from the ghosted primitives of every local block"""
    from fields_derived_ref import BlockGeometry, block_components
    nx = (sim.ie - sim.is_ + 1, sim.je - sim.js + 1, sim.ke - sim.ks + 1)
    out = []
    for b in range(sim.nblocks):
        bd = sim.block_bounds(b)
        G = BlockGeometry(nx, bd[0::2], bd[1::2], sim.ng, coordinates)
        gas = sim.field("gas.prim", b) if sim.ns_gas else None
        dust = sim.field("dust.prim", b) if sim.ns_dust else None
        out.append(block_components(names, gas, dust, sim.ns_gas, sim.ns_dust, G))
    return np.stack(out)


def main():
    spec = json.loads(sys.argv[1])
    from artemis_amd.driver import Simulation, TorchComm
    from fields_level_ref import same_bits
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libartemis_cpudouble.so"))
    comm = None
    if world > 1:
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["MASTER_PORT"], rank=rank, world_size=world)
        comm = TorchComm(torch.device("cpu"))
    meta, sim = {}, None
    deck = os.path.join(ROOT, "inputs", *spec["deck"])

    for act in spec["actions"]:
        op = act[0]
        if op == "create":
            sim = Simulation(deck, spec["overrides"], comm=comm, lib=lib)
        elif op == "evolve":
            sim.evolve(act[1])
        elif op == "save":
            sim.save(act[1])
        elif op == "restore":
            sim = Simulation.restore(act[1], comm=comm, lib=lib)
        elif op == "snap":
            meta[act[1]] = dict(time=sim.time, dt=sim.dt, ncycle=sim.ncycle, nblocks=sim.nblocks,
                                bounds=[sim.block_bounds(b) for b in range(sim.nblocks)],
                                levels=[sim.block_level(b) for b in range(sim.nblocks)])
        elif op == "state":
            np.savez(spec["out"] + ".%s.rank%d.npz" % (act[1], rank), prim=np.stack([sim.field("gas.prim", b) for b in range(sim.nblocks)]))
        elif op == "write":
            sim.write_fields(act[1], act[2])
        elif op == "check":
            got = sim.gather(act[2])
            meta[act[1]] = dict(same=bool(same_bits(got, reference(sim, act[2], spec["coordinates"]))), blocks=sim.nblocks,
                                nonzero=bool(np.any(got != 0.0)))
        elif op == "roll":
            a = sim.gather(act[1])
            at = 0
            for v in act[1]:
                ns = sim.ns_dust if v.startswith("dust.") else sim.ns_gas
                if v.endswith("velocity"):
                    for n in range(ns):
                        a[:, at + 3 * n:at + 3 * n + 3] = np.roll(a[:, at + 3 * n:at + 3 * n + 3], 1, axis=1)
                at += (3 if v.endswith("velocity") else 1) * ns
            sim.scatter(act[1], np.ascontiguousarray(a))
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
