#!/usr/bin/env python3
"""What the stencil of the derived field outputs costs over a pointwise component, and that the plain path is what it was
("derived field outputs").

One MI355X.  Two states: the 256^3 Sedov deck of bench.py after --warm cycles (one block), and the four-level disk with a
planet of `bench.py --workload disk_amr` (blocks of 16^3: thousands of them) after --warm cycles.  On each:

  gather    Simulation.gather(...) of [gas.derived.vorticity, gas.derived.divergence] and of [gas.prim.velocity]: the whole
            call -- kernels, the device-to-host copy into pageable memory, synchronisation -- median, minimum and maximum of
            --calls calls after 2 warm-up calls, --repeats times.
  kernel    artemis_hip_pack_fields of the same two selections on a MeshBlockPack that holds the same blocks and the same
            primitives (copied out of the run, ghost zones included), between two HIP events on the launch's stream: the
            launches alone, --repeats repetitions of --calls launches each.

--root DIR runs the library and the Python package of another checkout (the parent commit, built there), which knows no
derived variable: the velocity rows only.  Prints one JSON object.

    timeout -k 10 400 python3 scripts/fields_derived_cost.py --state sedov --out new_sedov.json && \\
    timeout -k 10 400 python3 scripts/fields_derived_cost.py --state sedov --root PARENT --out parent_sedov.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fields_reduce_level_cost import DISK_AMR  # noqa: E402
from history_cost import overrides  # noqa: E402

DERIVED = ["gas.derived.vorticity", "gas.derived.divergence"]
VELOCITY = ["gas.prim.velocity"]


def spread(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), n=len(ms))


def gather_ms(s, names, calls):
    for _ in range(2):
        s.gather(names)
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        s.gather(names)
        out.append(1e3 * (time.perf_counter() - t0))
    return spread(out)


def pack_of(s, coordinates):
    """a MeshBlockPack with the blocks and the primitives of the run, ghost zones included"""
    import numpy as np
    import torch
    from artemis_amd.pack import MeshBlockPack
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    bounds = [s.block_bounds(b) for b in range(s.nblocks)]
    mb = MeshBlockPack(s.nblocks, nx, [b[0::2] for b in bounds], [b[1::2] for b in bounds], ng=s.ng, ns_gas=s.ns_gas, ns_dust=s.ns_dust,
                       coordinates=coordinates, with_fluxes=False)
    for b in range(s.nblocks):
        mb.gas_prim[b].copy_(torch.from_numpy(np.ascontiguousarray(s.field("gas.prim", b))))
    return mb


def kernel_ms(mb, names, calls, repeats):
    import torch
    from artemis_amd import capi
    codes = {**capi.FIELD_VAR, **getattr(capi, "DERIVED_FIELD_VAR", {})}  # (the parent's package has no derived names)
    sel = (C.c_int * len(names))(*[codes[n] for n in names])
    nbytes = mb.L.artemis_hip_pack_fields_bytes(C.byref(mb.pack), len(names), sel, 0)
    assert nbytes > 0
    out = torch.empty(nbytes // 8, dtype=torch.float64, device=mb.dev)

    def launch():
        assert mb.L.artemis_hip_pack_fields(C.byref(mb.pack), 0, mb.nb, len(names), sel, 0, C.c_void_p(out.data_ptr()), mb._stream()) == 0
    launch(), launch()
    torch.cuda.synchronize()
    reps = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            launch()
        e1.record()
        e1.synchronize()
        reps.append(e0.elapsed_time(e1) / calls)
    return dict(spread(reps), bytes_out=nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=["sedov", "disk_amr"], required=True)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library and package run")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    if args.state == "sedov":
        s = Simulation(os.path.join(root, "inputs", "blast", "blast.in"), overrides(args.n))
        coordinates = "cartesian"
    else:
        s = Simulation(os.path.join(root, "inputs", "disk", "disk_nbody_cyl.in"), DISK_AMR)
        coordinates = "cylindrical"
    s.evolve(args.warm)
    has_derived = hasattr(capi, "DERIVED_FIELD_VAR")
    res = dict(source_sha=capi.source_sha(), state=args.state, blocks=s.nblocks, zones=s.total_zones, cycle=s.ncycle,
               note="gather: whole calls (kernels + copy + synchronisation); kernel: HIP events around artemis_hip_pack_fields launches")
    selections = dict(velocity=VELOCITY, **(dict(derived=DERIVED) if has_derived else {}))
    res["gather_ms"] = {k: [gather_ms(s, v, args.calls) for _ in range(args.repeats)] for k, v in selections.items()}
    mb = pack_of(s, coordinates)
    s.close()
    res["kernel_ms"] = {k: kernel_ms(mb, v, args.calls, args.repeats) for k, v in selections.items()}
    if has_derived:
        res["derived_over_velocity"] = dict(kernel=res["kernel_ms"]["derived"]["median"] / res["kernel_ms"]["velocity"]["median"],
                                            gather=statistics.median(r["median"] for r in res["gather_ms"]["derived"]) /
                                            statistics.median(r["median"] for r in res["gather_ms"]["velocity"]))
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
