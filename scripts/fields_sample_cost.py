#!/usr/bin/env python3
"""What a point sample costs beside the full gather it replaces ("point samples").

One MI355X.  Two states, each in a process of its own per library:

  sedov      the 256^3 Sedov deck of bench.py after --warm cycles (one block).  The 256^2 midplane lattice: plan creation
             (upload, locate kernel, the locations back, the host sort, the order up), values("gas.prim.density") on it, and
             the values kernel alone -- artemis_hip_sample_fields on a MeshBlockPack that holds the run's primitives, between
             two HIP events -- against gather("gas.prim.density") of the same state.
  disk_amr   the four-level disk with a planet of `bench.py --workload disk_amr` (thousands of blocks of 16^3) after --warm
             cycles.  A 1024^2 from_cartesian image of the midplane: plan creation and values, against gather.

--root DIR runs the library and the Python package of another checkout (the parent commit, built there), which has no
sample: its gather is the only way it can produce the slice, and that is the yardstick.  Whole calls are timed with the
wall clock (kernels, copies into pageable memory, synchronisation): median, minimum and maximum of --calls calls after 2
warm-up calls, --repeats times.  Every process prints one JSON object and writes it to --out;

    python3 scripts/fields_sample_cost.py --combine new_sedov.json parent_sedov.json new_disk.json parent_disk.json

writes profiles/fields_sample_cost.json from such files (runs of the two libraries alternating in one job).
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

DENSITY = ["gas.prim.density"]


def spread(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), n=len(ms))


def timed(fn, calls, repeats, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(repeats):
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        out.append(spread(ms))
    return out


def mesh_box(s):
    import numpy as np
    b = np.array([s.block_bounds(q) for q in range(s.nblocks)]).reshape(-1, 6)
    return b, b[:, 0::2].min(axis=0), b[:, 1::2].max(axis=0)


def table_stats(L, bounds, hi, nx):
    """blocks, cells and listed blocks of the locate table: the containment tests of a point are the length of its cell's
    list, those of a scan over all blocks the block count"""
    import numpy as np
    active = sum(1 << d for d in range(3) if nx[d] > 1)
    b = np.ascontiguousarray(bounds, dtype=np.float64)
    ch = (C.c_double * 3)(*hi)
    bp = b.ctypes.data_as(C.POINTER(C.c_double))
    nbytes = L.artemis_hip_locate_table_bytes(len(b), bp, ch, active)
    host = np.zeros(nbytes // 8)
    assert L.artemis_hip_locate_table_build(len(b), bp, ch, active, host.ctypes.data, nbytes) == 0
    head = host[:8].view(np.int64)  # magic, nblocks, ncell, nentries, n[3], active
    ncell, nentries = int(head[2]), int(head[3])
    return dict(table_bytes=int(nbytes), blocks=len(b), cells=ncell, listed=nentries, tests_per_point=nentries / ncell,
                scan_over_table=len(b) / (nentries / ncell))


def kernel_ms(s, plan, coordinates, calls, repeats):
    """artemis_hip_sample_fields alone, HIP events around `calls` launches, on a pack that holds the run's blocks"""
    import numpy as np
    import torch
    from fields_derived_cost import pack_of
    mb = pack_of(s, coordinates)
    loc = np.ascontiguousarray(np.concatenate([plan.block[:, None], plan.zone], axis=1).astype(np.int32))
    order = np.lexsort((loc[:, 3], loc[:, 2], loc[:, 1], np.where(loc[:, 0] < 0, 1 << 30, loc[:, 0]))).astype(np.int64)
    ld, od = torch.from_numpy(loc.reshape(-1)).to(mb.dev), torch.from_numpy(order).to(mb.dev)
    sel = (C.c_int * 1)(0)
    out = torch.empty(len(loc), dtype=torch.float64, device=mb.dev)
    res = {}
    for tag, o in (("sorted", C.c_void_p(od.data_ptr())), ("caller_order", None)):
        def launch():
            assert mb.L.artemis_hip_sample_fields(C.byref(mb.pack), len(loc), C.c_void_p(ld.data_ptr()), o, 1, sel, 0,
                                                  C.c_void_p(out.data_ptr()), mb._stream()) == 0
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
        res[tag] = spread(reps)
    return res


def combine(files, out):
    runs = [json.load(open(f)) for f in files]
    res = dict(note="scripts/fields_sample_cost.py: whole calls by the wall clock, ms; the parent's and this commit's libraries in "
                    "processes of their own, alternating in one job", runs=runs, summary={})
    med = lambda rows: statistics.median(r["median"] for r in rows)
    for state in ("sedov", "disk_amr"):
        mine = [r for r in runs if r["state"] == state and r["has_sample"]]
        theirs = [r for r in runs if r["state"] == state and not r["has_sample"]]
        if not mine or not theirs:
            continue
        g_parent = statistics.median(med(r["gather_ms"]) for r in theirs)
        res["summary"][state] = dict(points=mine[0]["points"], blocks=mine[0]["blocks"], zones=mine[0]["zones"],
                                     parent_gather_ms=g_parent, gather_ms=statistics.median(med(r["gather_ms"]) for r in mine),
                                     plan_create_ms=statistics.median(med(r["plan_create_ms"]) for r in mine),
                                     values_ms=statistics.median(med(r["values_ms"]) for r in mine),
                                     values_over_parent_gather=statistics.median(med(r["values_ms"]) for r in mine) / g_parent,
                                     locate=mine[0]["locate"], **({"kernel_ms": mine[0]["kernel_ms"]} if "kernel_ms" in mine[0] else {}))
    text = json.dumps(res, indent=1)
    with open(out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res["summary"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=["sedov", "disk_amr"])
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library and package run")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--image", type=int, default=1024)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-kernel", action="store_true", help="skip the HIP-event timing of the kernel alone")
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", nargs="+", default=None)
    args = ap.parse_args()
    if args.combine:
        return combine(args.combine, args.out or os.path.join(os.path.dirname(HERE), "profiles", "fields_sample_cost.json"))
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import numpy as np
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    if args.state == "sedov":
        s = Simulation(os.path.join(root, "inputs", "blast", "blast.in"), overrides(args.n))
        coordinates = "cartesian"
    else:
        s = Simulation(os.path.join(root, "inputs", "disk", "disk_nbody_cyl.in"), DISK_AMR)
        coordinates = "cylindrical"
    s.evolve(args.warm)
    has_sample = hasattr(s, "sample_plan")
    res = dict(source_sha=capi.source_sha(), state=args.state, has_sample=has_sample, blocks=s.nblocks, zones=s.total_zones, cycle=s.ncycle)
    res["gather_ms"] = timed(lambda: s.gather(DENSITY), args.calls, args.repeats)
    if has_sample:
        from artemis_amd import sample as smp
        bounds, lo, hi = mesh_box(s)
        nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
        if args.state == "sedov":
            dz = (hi[2] - lo[2]) / args.n
            k = args.n // 2
            pts = smp.lattice((lo[0], lo[1], lo[2] + k * dz), (hi[0], hi[1], lo[2] + (k + 1) * dz), (args.n, args.n, 1))
        else:
            xyz = smp.lattice((-hi[0], -hi[0], 0.0), (hi[0], hi[0], 0.0), (args.image, args.image, 1))
            pts = smp.from_cartesian("cylindrical", xyz, lo, hi)
        res["points"] = len(pts)
        plans = []

        def create():
            plans.append(s.sample_plan(pts))
            if len(plans) > 1:
                plans.pop(0).close()
        res["plan_create_ms"] = timed(create, args.calls, args.repeats)
        plan = plans[-1]
        res["found"] = int((plan.block >= 0).sum())
        res["values_ms"] = timed(lambda: plan.values(DENSITY), args.calls, args.repeats)
        res["locate"] = table_stats(s.L, bounds, hi, nx)
        # the values are the gather's: the slice of a whole dump, bit for bit
        q = s.gather(DENSITY)
        f = plan.block >= 0
        z = plan.zone[f]
        assert np.array_equal(plan.values(DENSITY)[0, f].view(np.uint64), q[plan.block[f], 0, z[:, 0], z[:, 1], z[:, 2]].view(np.uint64))
        if args.state == "sedov" and not args.no_kernel:
            res["kernel_ms"] = kernel_ms(s, plan, coordinates, 20, args.repeats)
    s.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
