"""Point sampling -- Simulation.sample_plan / sample (include/artemis_driver.h "sampling at points"; the definition is
include/artemis_hip_sample.h) -- on the CPU test double: no GPU.  The double defines neither kernel, so the points are located
by the host loop of csrc/driver/sample.cpp -- the same search (csrc/locate_table.hpp, one copy for the device and the host)
-- and the values come from the gather's host loop.  The definition is emulated in numpy (tests/fields_sample_ref.py): a scan
over the blocks, searchsorted over the faces, and a pick out of gather's array.  Conditions, not tolerances: every in-domain
point is found, block and zone equal the reference's, and every value comparison is bitwise.  The GPU cases are
tests/test_fields_sample.py.

A one-rank case runs in a process of its own (`isolated`: this file as a script runs one `check_*` function), like the other
CPU suites; the rank cases run tests/fields_sample_worker.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import amr_cases
import fields_sample_ref as ref
from fields_sample_ref import same_bits
from test_fields_derived_cpu import blast3d
from test_multirank_cpu import free_port
from test_outputs_cpu import blast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from artemis_amd import sample as smp  # noqa: E402

GAS = ["gas.prim.density", "gas.cons.momentum", "gas.derived.vorticity"]
DUSTY = GAS + ["dust.prim.velocity"]
PRIM = ["gas.prim.density", "gas.prim.velocity", "gas.prim.sie"]


@pytest.fixture(scope="module", autouse=True)
def double_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_double"), "-s"])


def isolated(check, *args):
    """run check(*args) (a function of this module, JSON-able arguments) in a fresh interpreter"""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), check.__name__, json.dumps(args)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, p.stdout.decode()[-4000:]


def simulation(case, extra=()):
    from artemis_amd.driver import Simulation
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libartemis_cpudouble.so"))
    return Simulation(os.path.join(ROOT, "inputs", *case["deck"]), list(case["overrides"]) + list(extra), lib=lib)


def mesh_of(sim):
    """(bounds [nb, 6], zones of a block, lower and upper corner of what this process holds)"""
    sim._refresh_dims()
    bounds = np.array([sim.block_bounds(b) for b in range(sim.nblocks)]).reshape(-1, 6)
    nx = (sim.ie - sim.is_ + 1, sim.je - sim.js + 1, sim.ke - sim.ks + 1)
    return bounds, nx, bounds[:, 0::2].min(axis=0), bounds[:, 1::2].max(axis=0)


def agree(sim, points, names, every_found=None, tag=""):
    """a plan of `points` against the definition: block, zone, who is found, and the values in double and in float"""
    bounds, nx, lo, hi = mesh_of(sim)
    loc = ref.locate(points, bounds, nx, sim.ng, hi)
    plan = sim.sample_plan(np.ascontiguousarray(points))
    try:
        assert np.array_equal(plan.block, loc[:, 0]) and np.array_equal(plan.zone, loc[:, 1:]), tag
        assert plan.block.dtype == np.int32 and plan.zone.shape == (len(points), 3)
        assert np.array_equal(loc[:, 0] >= 0, ref.in_domain(points, lo, hi, nx)), tag  # found if and only if in the domain
        if every_found is not None:
            assert bool((loc[:, 0] >= 0).all()) == every_found, tag
        q = sim.gather(names)
        for single in (False, True):
            got = plan.values(names, single=single)
            assert got.shape == (q.shape[1], len(points)) and got.dtype == (np.float32 if single else np.float64)
            assert same_bits(got, ref.pick(q, loc, single)), (tag, single)
        one, blk = sim.sample(names, np.ascontiguousarray(points))
        assert same_bits(one, ref.pick(q, loc)) and np.array_equal(blk, loc[:, 0])
    finally:
        plan.close()
    return loc, q


def check_eight_block_blast():
    """16^3 zones in 2 x 2 x 2 blocks after 4 cycles, all five point families"""
    sim = simulation(blast3d(True))
    try:
        sim.evolve(4)
        assert sim.nblocks == 8 and sim.ncycle == 4
        bounds, nx, lo, hi = mesh_of(sim)
        fam = ref.families(bounds, nx, sim.ng, lo, hi)
        assert len(fam["centres"]) == 4096 and len(fam["uniform"]) == 4096 and len(fam["corners"]) == 64
        # every zone centre once, shuffled: gather's array, permuted
        perm = np.random.default_rng(7).permutation(4096)
        q = sim.gather(GAS)
        got, blk = sim.sample(GAS, fam["centres"])
        flat = np.moveaxis(q, 1, 0).reshape(q.shape[1], -1)  # [ncomp][block][k][j][i]
        assert same_bits(got, flat[:, perm]) and (blk >= 0).all() and np.any(got[4:] != 0.0)
        for name in ("centres", "faces", "corners", "uniform"):
            loc, _ = agree(sim, fam[name], GAS, every_found=True, tag=name)
        assert len(np.unique(loc[:, 0])) == 8
        agree(sim, fam["outside"], GAS, every_found=False, tag="outside")
        assert (sim.sample(GAS, fam["outside"])[1] == -1).all() and np.isnan(sim.sample(GAS, fam["outside"])[0]).all()
        # the closed upper corner of the mesh lies in the last block's last zone, a shared face in the upper block's first
        loc = ref.locate(np.array([hi, 0.5 * (lo + hi)]), bounds, nx, sim.ng, hi)
        blk, zone = sim.sample_plan(np.array([hi, 0.5 * (lo + hi)])).block, sim.sample_plan(np.array([hi, 0.5 * (lo + hi)])).zone
        assert np.array_equal(blk, loc[:, 0]) and np.array_equal(zone, loc[:, 1:])
        assert tuple(zone[0]) == (7, 7, 7) and tuple(zone[1]) == (0, 0, 0) and blk[0] == 7 and blk[1] == 7
        everything = np.concatenate(list(fam.values()))
        agree(sim, everything, GAS + ["gas.prim.pressure", "gas.derived.divergence"], tag="all")
    finally:
        sim.close()


def check_blast2d_ignores_x3():
    """the 2-D blast: one active direction fewer, the x3 coordinate of the points is garbage and is ignored"""
    sim = simulation(blast())
    try:
        sim.evolve(4)
        bounds, nx, lo, hi = mesh_of(sim)
        assert nx[2] == 1 and sim.nblocks == 4
        fam = ref.families(bounds, nx, sim.ng, lo, hi, count=1024)
        for name in ("centres", "faces", "corners", "uniform"):
            pts = fam[name].copy()
            pts[0::2, 2], pts[1::2, 2] = 1e300, np.nan
            agree(sim, pts, GAS, every_found=True, tag=name)
        agree(sim, fam["outside"], GAS, every_found=False)
    finally:
        sim.close()


def refined_case(name):
    if name == "blast_amr":
        c = amr_cases.blast_amr(n=64)
        return dict(deck=list(c["deck"]), overrides=c["overrides"]), 2, GAS, 3
    c = amr_cases.disk_planet_dust_amr(**amr_cases.THICK_DISK)
    return dict(deck=list(c["deck"]), overrides=c["overrides"]), 1, DUSTY, 3


def straddling_lattice(sim, bounds, nx):
    """zone centres, at the finest level's zone size, of a box three blocks wide (one block to each side along every active
    direction) around a finest block that a coarser block touches"""
    levels = np.array([sim.block_level(b) for b in range(sim.nblocks)])
    act = [d for d in range(3) if nx[d] > 1]
    for b in np.flatnonzero(levels == levels.max()):
        bd = bounds[b]
        ext = bd[1::2] - bd[0::2]
        lo, hi = bd[0::2].copy(), bd[1::2].copy()
        shape = list(nx)
        for d in act:
            lo[d], hi[d], shape[d] = lo[d] - ext[d], hi[d] + ext[d], 3 * nx[d]
        coarser = [c for c in np.flatnonzero(levels < levels.max())
                   if all(bounds[c][2 * d] < hi[d] - 0.25 * ext[d] and bounds[c][2 * d + 1] > lo[d] + 0.25 * ext[d] for d in act)]
        if coarser:
            return smp.lattice(lo, hi, shape), levels
    raise AssertionError("no finest block next to a coarser one")


def check_refined(name):
    """a refined mesh: the centres of every leaf zone, every block's faces (the coarse-fine ones among them) and a lattice
    of finest-level zone centres that straddles a coarse-fine boundary, in double and in float"""
    case, cycles, names, nlevels = refined_case(name)
    sim = simulation(case)
    try:
        sim.evolve(cycles)
        bounds, nx, lo, hi = mesh_of(sim)
        lat, levels = straddling_lattice(sim, bounds, nx)
        assert len(set(levels)) >= nlevels, set(levels)
        loc, q = agree(sim, ref.centre_points(bounds, nx, sim.ng), names, every_found=True, tag="centres")
        assert np.array_equal(loc[:, 0], np.repeat(np.arange(sim.nblocks), nx[0] * nx[1] * nx[2]))
        agree(sim, ref.face_points(bounds, nx, sim.ng), names, every_found=True, tag="faces")
        loc, _ = agree(sim, lat, names, tag="lattice")
        assert len(set(levels[loc[loc[:, 0] >= 0, 0]])) >= 2  # the lattice reads blocks of more than one level
        agree(sim, ref.uniform_points(lo, hi, 2048, 3), names, every_found=True, tag="uniform")
    finally:
        sim.close()


def check_plan_lifetime():
    """a plan made before force_refine and before an evolve that remeshes answers by the fresh definition afterwards (.block
    included); it survives scatter; after close() it raises; npoints = 0 and npoints = 1 work"""
    c = amr_cases.blast_amr(n=64, derefine_count=2)
    sim = simulation(dict(deck=list(c["deck"]), overrides=c["overrides"]))
    try:
        bounds, nx, lo, hi = mesh_of(sim)
        pts = np.concatenate([ref.uniform_points(lo, hi, 2048, 11), ref.centre_points(bounds, nx, sim.ng)[::7]])
        plan = sim.sample_plan(pts)
        before, nb0 = plan.block.copy(), sim.nblocks
        levels = [sim.block_level(b) for b in range(sim.nblocks)]
        gid = int(np.argmin(levels))  # (one rank: the local index is the global one) a coarsest leaf
        assert sim.force_refine(gid) and sim.nblocks > nb0
        for stage in ("forced", "evolved"):
            b2, nx2, _, hi2 = mesh_of(sim)
            loc = ref.locate(pts, b2, nx2, sim.ng, hi2)
            assert np.array_equal(plan.block, loc[:, 0]) and np.array_equal(plan.zone, loc[:, 1:]), stage
            assert same_bits(plan.values(GAS), ref.pick(sim.gather(GAS), loc)), stage
            assert not np.array_equal(plan.block, before)
            if stage == "forced":
                before, r0 = plan.block.copy(), sim.remeshes
                for _ in range(40):
                    sim.evolve(1)
                    if sim.remeshes > r0:
                        break
                assert sim.remeshes > r0
        # scatter sets a new state on the same mesh: the plan stays located and reads the new values
        a = sim.gather(PRIM)
        a[:, 0] *= 1.5
        sim.scatter(PRIM, np.ascontiguousarray(a))
        b2, nx2, _, hi2 = mesh_of(sim)
        loc = ref.locate(pts, b2, nx2, sim.ng, hi2)
        assert np.array_equal(plan.block, loc[:, 0])
        assert same_bits(plan.values(["gas.prim.density"]), ref.pick(sim.gather(["gas.prim.density"]), loc))
        assert same_bits(plan.values(["gas.prim.density"]), ref.pick(a[:, 0:1], loc))
        plan.close()
        for use in (lambda: plan.values(GAS), lambda: plan.block, lambda: plan.zone):
            with pytest.raises(RuntimeError, match="closed"):
                use()
        plan.close()  # (closing twice is no error)
        empty = sim.sample_plan(np.empty((0, 3)))
        assert empty.values(GAS).shape == (7, 0) and empty.block.shape == (0,) and empty.zone.shape == (0, 3)
        one = sim.sample_plan(np.array([0.5 * (lo + hi)]))
        loc = ref.locate(np.array([0.5 * (lo + hi)]), b2, nx2, sim.ng, hi2)
        assert one.block[0] == loc[0, 0] >= 0 and same_bits(one.values(GAS, single=True), ref.pick(sim.gather(GAS), loc, True))
    finally:
        sim.close()


def check_refusals():
    from artemis_amd.driver import SamplePlan
    sim = simulation(blast())
    try:
        good = np.zeros((4, 3))
        for bad in (good.astype(np.float32), np.zeros((4, 2)), np.zeros(12), np.zeros((3, 4)).T, np.zeros((4, 6))[:, ::2], [[0.0, 0.0, 0.0]]):
            with pytest.raises(ValueError):
                sim.sample_plan(bad)
            with pytest.raises(ValueError):
                sim.sample(GAS, bad)
        plan = sim.sample_plan(good)
        assert isinstance(plan, SamplePlan)
        with pytest.raises(RuntimeError, match="unknown variable gas.prim.temperature"):
            plan.values(["gas.prim.temperature"])
        with pytest.raises(RuntimeError, match="unknown variable dust.prim.velocity"):
            plan.values(["gas.prim.density", "dust.prim.velocity"])
        with pytest.raises(RuntimeError, match="unknown variable dust.derived.vorticity"):
            sim.sample(["dust.derived.vorticity"], good)
        assert plan.values([]).shape == (0, 4)
        assert plan.values("gas.prim.density").shape == (1, 4)  # (a single name, as gather takes one)
    finally:
        sim.close()


def check_from_cartesian_image():
    """pixel centres of a 32^2 image over the cylindrical disk equal the reference lookup; pixels inside the inner radius (and
    beyond the outer one) are not found"""
    case = dict(deck=["disk", "disk_cyl.in"],
                overrides=["parthenon/mesh/nx1=16", "parthenon/mesh/nx2=8", "parthenon/mesh/nx3=6", "parthenon/meshblock/nx1=8",
                           "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=3", "parthenon/mesh/x1min=0.8", "parthenon/mesh/x1max=4.3",
                           "parthenon/mesh/x3min=-1.0", "parthenon/mesh/x3max=1.0", "parthenon/time/nlim=3"])
    sim = simulation(case)
    try:
        sim.evolve(2)
        bounds, nx, lo, hi = mesh_of(sim)
        assert abs((hi[1] - lo[1]) - 2.0 * np.pi) < 1e-12  # the whole circle
        xyz = smp.lattice((-4.0, -4.0, 0.1), (4.0, 4.0, 0.1), (32, 32, 1))
        pts = smp.from_cartesian("cylindrical", xyz, lo, hi)
        assert pts.shape == (1024, 3) and pts.flags["C_CONTIGUOUS"] and (pts[:, 1] >= lo[1]).all() and (pts[:, 1] < hi[1]).all()
        assert np.allclose(pts[:, 0] * np.cos(pts[:, 1]), xyz[:, 0]) and np.allclose(pts[:, 0] * np.sin(pts[:, 1]), xyz[:, 1])
        loc, _ = agree(sim, pts, GAS, tag="image")
        R = np.hypot(xyz[:, 0], xyz[:, 1])
        assert np.array_equal(loc[:, 0] >= 0, (R >= lo[0]) & (R <= hi[0]))
        assert (loc[R < lo[0], 0] == -1).all() and (R < lo[0]).sum() >= 4 and (loc[:, 0] >= 0).sum() > 500
        # the other systems: the inverse of ConvertCoordsToCart
        p = np.array([[1.0, 2.0, 3.0], [-2.0, 0.5, -1.0], [0.3, -0.4, 0.0]])
        s = smp.from_cartesian("spherical", p)
        assert np.allclose(np.stack([s[:, 0] * np.sin(s[:, 1]) * np.cos(s[:, 2]), s[:, 0] * np.sin(s[:, 1]) * np.sin(s[:, 2]), s[:, 0] * np.cos(s[:, 1])], 1), p)
        a = smp.from_cartesian("axisymmetric", p, lo=(0.0, -5.0, -np.pi), hi=(5.0, 5.0, np.pi))
        assert np.allclose(np.stack([a[:, 0] * np.cos(a[:, 2]), a[:, 0] * np.sin(a[:, 2]), a[:, 1]], 1), p) and (a[:, 2] >= -np.pi).all() and (a[:, 2] < np.pi).all()
        assert np.array_equal(smp.from_cartesian("cartesian", p), p)
        with pytest.raises(ValueError):
            smp.from_cartesian("toroidal", p)
    finally:
        sim.close()


def run_ranks(world, case, cycles, names, points, tmp_path, tag):
    """tests/fields_sample_worker.py on `world` ranks; returns what each rank left"""
    out = str(tmp_path / tag)
    np.save(out + ".points.npy", points)
    spec = dict(deck=list(case["deck"]), overrides=list(case["overrides"]), cycles=cycles, variables=names, out=out)
    threads = str(max(1, min(4, (os.cpu_count() or 1) // world)))
    for attempt in range(2):  # (the probed port can be taken between the probe and the rendezvous: one retry)
        port = str(free_port())
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS=threads)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "fields_sample_worker.py"), json.dumps(spec)],
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs = [p.communicate(timeout=900)[0].decode() for p in procs]
        rendezvous = any(p.returncode != 0 and ("Address already in use" in o or "Connection re" in o or "timed out" in o.lower()
                                                or "terminate called without an active exception" in o)
                         for p, o in zip(procs, outs))
        if not (rendezvous and attempt == 0):
            break
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [dict(np.load(out + ".rank%d.npz" % r)) for r in range(world)]


RANK_CASES = {"blast": (blast3d(True), 3, GAS, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),
              "blast_amr": (refined_case("blast_amr")[0], 2, GAS, (1.0, 0.0, 0.0), (5.0, 1.570796326794897, 0.0))}  # (the deck's quarter annulus)
_one_rank = {}


def one_rank(name, tmp_path):
    """the one-rank answer of a rank case (made once, shared, left unchanged) and its points"""
    if name not in _one_rank:
        case, cycles, names, lo, hi = RANK_CASES[name]
        lo, hi = np.array(lo), np.array(hi)
        pts = np.concatenate([ref.uniform_points(lo, hi, 3000, 5), np.array([lo, hi, 0.5 * (lo + hi)]),
                              ref.uniform_points(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), 300, 6)])
        res = run_ranks(1, case, cycles, names, pts, tmp_path, name + "_one")[0]
        for a in res.values():
            a.setflags(write=False)
        _one_rank[name] = (pts, res)
    return _one_rank[name]


# (the 2 x 2 x 2 block grid of the uniform blast has no split over three ranks: the driver refuses to create such a run)
@pytest.mark.parametrize("name,world", [("blast", 2), ("blast_amr", 2), ("blast_amr", 3)])
def test_ranks_answer_for_their_own_blocks_and_their_union_is_the_one_rank_answer(tmp_path, name, world):
    """two and three gloo ranks: every in-domain point is found on exactly one rank, in the block (by its bounds) and zone the
    one-rank run finds it in, and the union of the ranks' values is the one-rank array, bit for bit; the rest is NaN"""
    case, cycles, names, _, _ = RANK_CASES[name]
    pts, one = one_rank(name, tmp_path)
    res = run_ranks(world, case, cycles, names, pts, tmp_path, "%s_%d" % (name, world))
    found = np.stack([r["block"] >= 0 for r in res])
    assert np.array_equal(found.sum(axis=0), (one["block"] >= 0).astype(int)) and 3000 <= found.sum() < len(pts)
    assert all(r["block"].max() >= 0 for r in res) and sum(len(r["bounds"]) for r in res) == len(one["bounds"])
    union, usingle = np.full_like(one["values"], np.nan), np.full_like(one["single"], np.nan)
    for r in res:
        f = r["block"] >= 0
        assert np.isnan(r["values"][:, ~f]).all() and (r["zone"][~f] == -1).all()
        assert np.array_equal(r["bounds"][r["block"][f]], one["bounds"][one["block"][f]]) and np.array_equal(r["zone"][f], one["zone"][f])
        union[:, f], usingle[:, f] = r["values"][:, f], r["single"][:, f]
    assert same_bits(union, one["values"]) and same_bits(usingle, one["single"]) and int(one["ncycle"]) == cycles


def test_eight_block_blast():
    isolated(check_eight_block_blast)


def test_blast2d_ignores_x3():
    isolated(check_blast2d_ignores_x3)


@pytest.mark.parametrize("name", ["blast_amr", "thick_disk"])
def test_refined(name):
    isolated(check_refined, name)


def test_plan_lifetime():
    isolated(check_plan_lifetime)


def test_refusals():
    isolated(check_refusals)


def test_from_cartesian_image():
    isolated(check_from_cartesian_image)


if __name__ == "__main__":
    globals()[sys.argv[1]](*json.loads(sys.argv[2]))
