"""Worker of tests/test_scatter_cpu.py: one rank (of a gloo world, or alone) driving several simulations of the product's
host driver against the CPU test double through a list of actions.  The double does not define artemis_hip_unpack_fields
(nor artemis_hip_pack_fields), so every scatter goes through the driver's host loop over downloaded and uploaded
primitives.  Simulations and arrays are named; actions, as JSON lists:
    ["create", sim, extra overrides]            a Simulation of the spec's deck + overrides + the extra ones
    ["evolve", sim, n] | ["close", sim]
    ["snap", tag, sim]                          clock, kernel, block levels and bounds as they are now -> JSON result
    ["prims", tag, sim]                         interiors of field("gas.prim") (and "dust.prim") of every local block
                                                -> <out>.<tag>.rank<r>.npz (keys "gas", "dust")
    ["track", tag, sim, n]                      n times evolve(1); per cycle the clock and kernel in the JSON result and the
                                                interiors in <out>.<tag>.rank<r>.npz (keys "gas<ncycle>", "dust<ncycle>")
    ["gather", arr, sim, variables, single]     arr = sim.gather(...)
    ["scatter", sim, variables, arr, clock]     sim.scatter(variables, arr, time); clock = null (keep) or the name of the
                                                simulation whose time is taken
    ["mangle", arr, how]                        arr replaced by a wrong one: "shape", "dtype", "strided"
    ["write", sim, path, variables, single] | ["load", sim, path, clock]
    ["sizes", tag, sim, variables, single]      what artemis_sim_scatter_fields and artemis_sim_gather_fields return for host
                                                pointer NULL (bytes of the buffer), and the bytes of a gather
    ["raises", tag, action]                     runs the action; records the exception's type and text (null: none)"""
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


def interiors(sim):
    out = {"gas": np.stack([sim.interior(sim.field("gas.prim", b)) for b in range(sim.nblocks)])}
    if sim.ns_dust:
        out["dust"] = np.stack([sim.interior(sim.field("dust.prim", b)) for b in range(sim.nblocks)])
    return out


def clock_of(sim):
    return dict(time=sim.time, dt=sim.dt, ncycle=sim.ncycle, kernel=sim.stage_kernel, nblocks=sim.nblocks,
                levels=[sim.block_level(b) for b in range(sim.nblocks)], bounds=[sim.block_bounds(b) for b in range(sim.nblocks)])


def main():
    spec = json.loads(sys.argv[1])
    from artemis_amd.driver import Simulation, TorchComm
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libartemis_cpudouble.so"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["MASTER_PORT"], rank=rank, world_size=world)
    meta, sims, arrays = {}, {}, {}

    def npz(tag):
        return spec["out"] + ".%s.rank%d.npz" % (tag, rank)

    def do(act):
        op = act[0]
        if op == "create":
            comm = TorchComm(torch.device("cpu")) if world > 1 else None
            sims[act[1]] = Simulation(os.path.join(ROOT, "inputs", *spec["deck"]), spec["overrides"] + list(act[2]), comm=comm, lib=lib)
        elif op == "evolve":
            sims[act[1]].evolve(act[2])
        elif op == "close":
            sims.pop(act[1]).close()
        elif op == "snap":
            meta[act[1]] = clock_of(sims[act[2]])
        elif op == "prims":
            np.savez(npz(act[1]), **interiors(sims[act[2]]))
        elif op == "track":
            sim, rows, out = sims[act[2]], [], {}
            for _ in range(act[3]):
                assert sim.evolve(1) == 1
                rows.append(clock_of(sim))
                for k, v in interiors(sim).items():
                    out["%s%d" % (k, sim.ncycle)] = v
            meta[act[1]] = rows
            np.savez(npz(act[1]), **out)
        elif op == "gather":
            arrays[act[1]] = sims[act[2]].gather(act[3], single=act[4])
        elif op == "scatter":
            sims[act[1]].scatter(act[2], arrays[act[3]], time=None if act[4] is None else sims[act[4]].time)
        elif op == "mangle":
            a = arrays[act[1]]
            arrays[act[1]] = {"shape": lambda: a[:, :-1].copy(), "dtype": lambda: a.astype(np.int64),
                              "strided": lambda: a[..., ::2]}[act[2]]()
        elif op == "write":
            sims[act[1]].write_fields(act[2], act[3], single=act[4])
        elif op == "load":
            meta.setdefault("loaded", []).append(sims[act[1]].load_fields(act[2], clock=act[3]))
        elif op == "sizes":
            sim = sims[act[2]]
            names, n = sim._names(act[3])
            meta[act[1]] = [sim.L.artemis_sim_scatter_fields(sim.h, n, names, int(act[4]), None, float("nan")),
                            sim.L.artemis_sim_gather_fields(sim.h, n, names, int(act[4]), None), sim.gather(act[3], single=act[4]).nbytes]
        elif op == "raises":
            try:
                do(act[2])
                meta[act[1]] = None
            except Exception as e:  # noqa: BLE001 (the test asserts the type)
                meta[act[1]] = dict(type=type(e).__name__, text=str(e))
        else:
            raise ValueError(op)

    for act in spec["actions"]:
        do(act)
    with open(spec["out"] + ".rank%d.json" % rank, "w") as f:
        json.dump(meta, f)
    for s in list(sims.values()):
        s.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
