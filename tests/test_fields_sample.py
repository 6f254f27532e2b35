"""GPU tests of point sampling (include/artemis_hip_sample.h): artemis_hip_locate_points and artemis_hip_sample_fields on packs
with random primitives in every zone, ghost zones included, and Simulation.sample_plan / sample on the host driver.  Only
repository code runs here.

The block and zone of every point are held against the numpy definition (tests/fields_sample_ref.py: a scan over the blocks,
searchsorted over the faces); the values against the pack definition's own bits, artemis_hip_pack_fields of the same pack
picked at those zones, for every code, plain and derived, in double and in float.  Every comparison is bitwise.  The packs
are the smallest on which a lane can go wrong: a row longer than a wave, several blocks, one to three active directions,
every coordinate system with several species, and blocks of two sizes side by side."""
import ctypes as C
import os

import numpy as np
import pytest

import amr_cases
import fields_sample_ref as ref
from fields_sample_ref import same_bits
from test_fields import BLAST32
from test_fields_derived import code_of, device_fields

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)
NG = 2
GAS = ["gas.prim.density", "gas.cons.momentum", "gas.derived.vorticity"]
DUSTY = GAS + ["dust.prim.velocity"]


def side_by_side(nb, lo, hi):
    edges = np.linspace(lo[0], hi[0], nb + 1)
    return [[edges[b], edges[b + 1], lo[1], hi[1], lo[2], hi[2]] for b in range(nb)]


def mixed(three_d):
    """one block on [0, 1]^d and 2^d half-size blocks tiling [1, 2] x [0, 1]^(d - 1)"""
    z = [(0.0, 0.5), (0.5, 1.0)] if three_d else [(-0.5, 0.5)]
    out = [[0.0, 1.0, 0.0, 1.0, 0.0 if three_d else -0.5, 1.0 if three_d else 0.5]]
    for z0, z1 in z:
        for y0 in (0.0, 0.5):
            for x0 in (1.0, 1.5):
                out.append([x0, x0 + 0.5, y0, y0 + 0.5, z0, z1])
    return out


# name: (bounds [nb][6], nx, ns_gas, ns_dust, coordinates); two ghost zones everywhere
PACKS = {
    "cart3d": (side_by_side(1, (-1, -0.5, 0.25), (1, 0.8, 0.95)), (70, 6, 3), 1, 0, "cartesian"),  # a row of a wave and a ragged tail
    "three": (side_by_side(3, (-1, -0.5, 0.25), (2, 0.8, 0.95)), (70, 6, 3), 1, 1, "cartesian"),
    "cart1d": (side_by_side(1, (0, -0.5, -0.5), (1, 0.5, 0.5)), (8, 1, 1), 1, 0, "cartesian"),
    "cyl3d": (side_by_side(1, (0.5, 0.0, -1.0), (2.0, 6.0, 1.0)), (8, 5, 3), 1, 2, "cylindrical"),  # gas and two dust species
    "sph3d": (side_by_side(1, (0.3, 0.7, 0.0), (1.7, 2.5, 6.0)), (8, 5, 3), 2, 0, "spherical"),     # two gas species
    "mixed2d": (mixed(False), (8, 4, 1), 1, 0, "cartesian"),
    "mixed3d": (mixed(True), (8, 4, 4), 1, 1, "cartesian"),
}


def codes_of(nsd):
    """every code the pack has a fluid for, plain and derived"""
    return list(range(8)) + [16, 17] + (list(range(8, 12)) + [18, 19] if nsd else [])


def make_pack(name, seed=13):
    """the pack with random primitives in every zone, ghost zones included; (pack, bounds [nb, 6], lower and upper corner)"""
    import torch
    from artemis_amd.pack import MeshBlockPack
    bounds, nx, nsg, nsd, coords = PACKS[name]
    bounds = np.array(bounds, dtype=np.float64)
    mb = MeshBlockPack(len(bounds), nx, bounds[:, 0::2], bounds[:, 1::2], ng=NG, ns_gas=nsg, ns_dust=nsd, gamma=1.4, dfloor=0.7, siefloor=0.75,
                       dust_dfloor=0.65, coordinates=coords, with_fluxes=False)
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.5, 2.0, size=tuple(mb.gas_prim.shape))
    g[:, nsg:4 * nsg] = rng.uniform(-1.5, 1.5, size=g[:, nsg:4 * nsg].shape)
    d = rng.uniform(0.5, 2.0, size=tuple(mb.dust_prim.shape))
    d[:, nsd:] = rng.uniform(-1.5, 1.5, size=d[:, nsd:].shape)
    mb.gas_prim.copy_(torch.from_numpy(g))
    mb.dust_prim.copy_(torch.from_numpy(d))
    return mb, bounds, bounds[:, 0::2].min(axis=0), bounds[:, 1::2].max(axis=0)


def pack_points(name, bounds, nx, lo, hi):
    """the five families of the pack in one list whose length is no multiple of 64"""
    fam = ref.families(bounds, nx, NG, lo, hi, count=1000)
    pts = np.concatenate([fam[k] for k in ("centres", "faces", "corners", "outside", "uniform")])
    if nx[2] == 1:  # an inactive direction: its coordinate is garbage
        pts[0::2, 2], pts[1::2, 2] = 1e300, np.nan
    if nx[1] == 1:
        pts[0::3, 1], pts[1::3, 1] = -1e300, np.nan
    return np.ascontiguousarray(pts[:len(pts) - 1] if len(pts) % 64 == 0 else pts)


@pytest.fixture(scope="module")
def definition():
    """name -> (points, the definition's loc, the pack definition's values [nb, ncomp, nz, ny, nx] of every code): formed once
    per pack, shared, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            mb, bounds, lo, hi = make_pack(name)
            pts = pack_points(name, bounds, mb.nx, lo, hi)
            codes = codes_of(mb.nsd)
            shape = (mb.nx[2], mb.nx[1], mb.nx[0])
            q = np.stack(blocks_of_codes(mb, device_fields(mb, codes), codes, [shape] * mb.nb))
            loc = ref.locate(pts, bounds, mb.nx, NG, hi)
            for a in (pts, loc, q):
                a.setflags(write=False)
            cache[name] = (pts, loc, q)
        return cache[name]
    return get


def ncomp_of_codes(mb, codes):
    return sum((3 if c in (1, 5, 9, 11, 17, 19) else 1) * (mb.nsd if (8 <= c < 12 or c >= 18) else mb.nsg) for c in codes)


def blocks_of_codes(mb, flat, codes, shapes):
    out, at = [], 0
    for shape in shapes:
        full = (ncomp_of_codes(mb, codes),) + tuple(shape)
        out.append(flat[at:at + int(np.prod(full))].reshape(full))
        at += int(np.prod(full))
    assert at == flat.size
    return out


def device_table(mb, bounds, hi):
    """the locate table of these blocks, built on the host and copied to the device"""
    import torch
    nb = len(bounds)
    active = sum(1 << d for d in range(3) if mb.nx[d] > 1)
    b = np.ascontiguousarray(bounds, dtype=np.float64)
    ch = (C.c_double * 3)(*hi)
    bp = b.ctypes.data_as(C.POINTER(C.c_double))
    nbytes = mb.L.artemis_hip_locate_table_bytes(nb, bp, ch, active)
    assert nbytes > 0 and nbytes % 8 == 0
    host = np.zeros(nbytes // 8)
    assert mb.L.artemis_hip_locate_table_build(nb, bp, ch, active, host.ctypes.data, nbytes) == 0, mb.L.artemis_hip_last_error()
    return torch.from_numpy(host).to(mb.dev), ch


GUARD = 4096


def device_locate(mb, bounds, hi, pts, expect=0, npoints=None):
    """artemis_hip_locate_points: loc [npoints, 4]; the buffer behind it is checked to be untouched"""
    import torch
    table, ch = device_table(mb, bounds, hi)
    n = len(pts) if npoints is None else npoints
    p = torch.from_numpy(np.array(pts, dtype=np.float64).reshape(-1)).to(mb.dev) if len(pts) else torch.zeros(3, dtype=torch.float64, device=mb.dev)
    loc = torch.full((4 * max(len(pts), 0) + GUARD,), -7, dtype=torch.int32, device=mb.dev)
    rc = mb.L.artemis_hip_locate_points(C.byref(mb.pack), C.c_void_p(table.data_ptr()), ch, n, C.c_void_p(p.data_ptr()),
                                        C.c_void_p(loc.data_ptr()), mb._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, mb.L.artemis_hip_last_error().decode())
    flat = loc.cpu().numpy()
    if expect or n == 0:
        assert (flat == -7).all()
        return flat
    assert (flat[4 * n:] == -7).all()
    return flat[:4 * n].reshape(n, 4)


def payload_nan(count, single, dev):
    """a buffer of NaNs that carry a payload no kernel writes: what is still there was not written"""
    import torch
    if single:
        return torch.full((count,), 0x7fc0dead, dtype=torch.int32, device=dev)
    return torch.full((count,), 0x7ff8deadbeef0000, dtype=torch.int64, device=dev)


def device_sample(mb, loc, codes, single=False, order=None, expect=0, npoints=None, nsel=None):
    """artemis_hip_sample_fields at loc [npoints, 4]: [ncomp, npoints]; the output is filled with payload NaNs beforehand, with
    a guard region behind it: all of it is written and nothing past its end"""
    import torch
    n = len(loc) if npoints is None else npoints
    ncomp = ncomp_of_codes(mb, codes) if expect == 0 else 0
    sel = (C.c_int * max(len(codes), 1))(*[code_of(c) for c in codes])
    ld = torch.from_numpy(np.array(loc, dtype=np.int32).reshape(-1)).to(mb.dev) if len(loc) else torch.zeros(4, dtype=torch.int32, device=mb.dev)
    od = None if order is None else torch.from_numpy(np.array(order, dtype=np.int64)).to(mb.dev)
    out = payload_nan(ncomp * max(n, 0) + GUARD, single, mb.dev)
    before = out.cpu().numpy().copy()
    rc = mb.L.artemis_hip_sample_fields(C.byref(mb.pack), n, C.c_void_p(ld.data_ptr()), C.c_void_p(od.data_ptr()) if od is not None else None,
                                        len(codes) if nsel is None else nsel, sel, int(single), C.c_void_p(out.data_ptr()), mb._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, mb.L.artemis_hip_last_error().decode())
    raw = out.cpu().numpy()
    if expect or n == 0:
        assert np.array_equal(raw, before)  # untouched
        return raw
    assert np.array_equal(raw[ncomp * n:], before[ncomp * n:]) and not (raw[:ncomp * n] == before[0]).any()
    return raw[:ncomp * n].view(np.float32 if single else np.float64).reshape(ncomp, n)


def sorted_order(loc):
    return np.lexsort((np.arange(len(loc)), loc[:, 3], loc[:, 2], loc[:, 1], np.where(loc[:, 0] < 0, 1 << 30, loc[:, 0]))).astype(np.int64)


@pytest.mark.parametrize("name", list(PACKS))
def test_locate_points_equals_the_definition(hiplib, definition, name):
    """{block, k, j, i} of every family: zone centres, every face coordinate (lower-inclusive, shared faces, the closed upper
    edge), block corners, points outside and not finite, uniform points; garbage along the inactive directions; a list of 0
    and of 1 points; and the same bits from one workgroup's grid-stride trips"""
    from artemis_amd import capi
    mb, bounds, lo, hi = make_pack(name)
    pts, loc, _ = definition(name)
    assert len(pts) % 64 != 0
    got = device_locate(mb, bounds, hi, pts)
    assert np.array_equal(got, loc), np.flatnonzero((got != loc).any(axis=1))[:10]
    assert np.array_equal(loc[:, 0] >= 0, ref.in_domain(pts, lo, hi, mb.nx)) and len(np.unique(loc[:, 0])) == mb.nb + 1
    with capi.option("grid_cap", 1):
        assert np.array_equal(device_locate(mb, bounds, hi, pts), loc)
    device_locate(mb, bounds, hi, pts[:0])
    assert np.array_equal(device_locate(mb, bounds, hi, pts[:1]), loc[:1])


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name", list(PACKS))
def test_sample_fields_equals_the_pack_definition(hiplib, definition, name, single):
    """every code, plain and derived, in one selection: the bits artemis_hip_pack_fields stores for the zone, NaN where the
    point is not found; with order_dev NULL, the sorted order and a reversed one; nothing is written to the pack"""
    mb, bounds, lo, hi = make_pack(name)
    pts, loc, q = definition(name)
    codes = codes_of(mb.nsd)
    want = ref.pick(q, loc, single)
    assert np.isnan(want).any() and np.any(want[:, loc[:, 0] >= 0] != 0.0)
    g0, d0 = mb.gas_prim.cpu().numpy().copy(), mb.dust_prim.cpu().numpy().copy()
    order = sorted_order(loc)
    for o in (None, order, order[::-1].copy()):
        got = device_sample(mb, loc, codes, single, o)
        assert same_bits(got, want), (name, o is None)
    plain = [c for c in codes if c < 16]
    rows = np.concatenate([np.arange(ncomp_of_codes(mb, codes[:e]), ncomp_of_codes(mb, codes[:e + 1])) for e, c in enumerate(codes) if c < 16])
    assert same_bits(device_sample(mb, loc, plain, single, order), want[rows])  # a request without derived codes
    assert np.array_equal(mb.gas_prim.cpu().numpy(), g0) and np.array_equal(mb.dust_prim.cpu().numpy(), d0)


def test_sample_fields_small_lists_and_grid_stride_trips(hiplib, definition):
    from artemis_amd import capi
    mb, bounds, lo, hi = make_pack("three")
    pts, loc, q = definition("three")
    codes = codes_of(mb.nsd)
    want = ref.pick(q, loc)
    with capi.option("grid_cap", 1):
        assert same_bits(device_sample(mb, loc, codes, False, sorted_order(loc)), want)
    device_sample(mb, loc[:0], codes)
    found = int(np.flatnonzero(loc[:, 0] >= 0)[0])
    assert same_bits(device_sample(mb, loc[found:found + 1], codes), want[:, found:found + 1])
    assert device_sample(mb, loc, []).shape == (0, len(loc))  # no variables: succeeds, touches nothing
    # locations outside the pack and order entries outside the list touch nothing they should not
    bad = loc.copy()
    bad[0], bad[1], bad[2] = (mb.nb, 0, 0, 0), (0, 0, 0, mb.nx[0]), (0, -1, 0, 0)
    got = device_sample(mb, bad, codes)
    assert np.isnan(got[:, :3]).all() and same_bits(got[:, 3:], want[:, 3:])


def test_refusals_leave_the_buffers_untouched(hiplib, definition):
    from artemis_amd import capi
    gas_only, bounds, lo, hi = make_pack("sph3d")
    pts, loc, _ = definition("sph3d")
    for code in (12, 15, 20, 1000, -1):
        device_sample(gas_only, loc, [0, code], expect=capi.EINVAL)
        assert b"unknown variable code" in gas_only.L.artemis_hip_last_error()
    for code in (8, 11, 18, 19):
        device_sample(gas_only, loc, [16, code], expect=capi.EINVAL)
        assert b"a dust variable on a pack without dust" in gas_only.L.artemis_hip_last_error()
    device_sample(gas_only, loc, [0], expect=capi.EINVAL, nsel=33)
    device_sample(gas_only, loc, [0], expect=capi.EINVAL, nsel=-1)
    device_sample(gas_only, loc, [0], expect=capi.EINVAL, npoints=-1)
    device_locate(gas_only, bounds, hi, pts, expect=capi.EINVAL, npoints=-1)
    ch = (C.c_double * 3)(*hi)
    bp = np.ascontiguousarray(bounds).ctypes.data_as(C.POINTER(C.c_double))
    L = gas_only.L
    assert L.artemis_hip_locate_table_bytes(0, bp, ch, 7) == 0 and L.artemis_hip_locate_table_bytes(1, bp, ch, 8) == 0
    small = np.zeros(2)
    assert L.artemis_hip_locate_table_build(1, bp, ch, 7, small.ctypes.data, 16) == capi.EINVAL and (small == 0).all()
    assert b"smaller than" in L.artemis_hip_last_error()


# ---- host driver ------------------------------------------------------------------------------------------------------
def mesh_of(s):
    s._refresh_dims()
    bounds = np.array([s.block_bounds(b) for b in range(s.nblocks)]).reshape(-1, 6)
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    return bounds, nx, bounds[:, 0::2].min(axis=0), bounds[:, 1::2].max(axis=0)


def agree(s, pts, names, tag=""):
    """a plan against the definition and the gather of the same state, in double and in float"""
    bounds, nx, lo, hi = mesh_of(s)
    loc = ref.locate(pts, bounds, nx, s.ng, hi)
    plan = s.sample_plan(np.ascontiguousarray(pts))
    assert np.array_equal(plan.block, loc[:, 0]) and np.array_equal(plan.zone, loc[:, 1:]), tag
    assert np.array_equal(loc[:, 0] >= 0, ref.in_domain(pts, lo, hi, nx)), tag
    q = s.gather(names)
    for single in (False, True):
        assert same_bits(plan.values(names, single=single), ref.pick(q, loc, single)), (tag, single)
    plan.close()
    return loc


def prims(s):
    return [s.field("gas.prim", b)[[0, 1, 2, 3, 5]] for b in range(s.nblocks)]  # (the pressure slot of a ghost zone is no state)


def test_midplane_slice_on_the_tuned_sedov_path_and_the_run_is_not_disturbed(hiplib):
    """32^3 blast in 2 x 2 x 2 blocks on the tuned kernel: mid-run the values of a midplane lattice equal the cut of gather,
    a list larger than a 1 MiB staging buffer goes through in chunks with the same bits, and the run's final state with and
    without sampling is the same, bit for bit"""
    from artemis_amd import capi, sample as smp
    from artemis_amd.driver import Simulation
    ov = BLAST32 + ["parthenon/time/nlim=6"]
    a, b = Simulation(DECK("blast", "blast.in"), ov), Simulation(DECK("blast", "blast.in"), ov)
    assert a.uses_tuned_kernel and a.nblocks == 8
    bounds, nx, lo, hi = mesh_of(a)
    dz = (hi[2] - lo[2]) / 32
    mid = smp.lattice((lo[0], lo[1], lo[2] + 16 * dz), (hi[0], hi[1], lo[2] + 17 * dz), (32, 32, 1))  # the plane of zones k = 16
    plan = a.sample_plan(mid)
    a.evolve(3), b.evolve(3)
    q = a.gather(GAS)
    cut = np.full((q.shape[1], 32, 32), np.nan)
    for blk in range(a.nblocks):
        bd = bounds[blk]
        i0, j0, k0 = (int(round((bd[2 * d] - lo[d]) / (hi[d] - lo[d]) * 32)) for d in range(3))
        if k0 <= 16 < k0 + nx[2]:
            cut[:, j0:j0 + nx[1], i0:i0 + nx[0]] = q[blk][:, 16 - k0]
    got = plan.values(GAS)
    assert same_bits(got.reshape(-1, 32, 32), cut) and not np.isnan(got).any() and np.any(got[4:] != 0.0)
    assert same_bits(plan.values(GAS, single=True), got.astype(np.float32))
    allpts = ref.centre_points(bounds, nx, a.ng)
    loc = agree(a, allpts, GAS, "whole mesh")
    with capi.option("fields_stage_mb", 1):  # 32768 points x 7 components x 8 bytes: two chunks of the sorted order
        p2 = a.sample_plan(allpts)
        assert same_bits(p2.values(GAS), ref.pick(q, loc))
        p2.close()
    a.evolve(), b.evolve()
    assert same_bits(plan.values(["gas.prim.density"]), ref.pick(a.gather(["gas.prim.density"]), ref.locate(mid, bounds, nx, a.ng, hi)))
    assert (a.time, a.dt, a.ncycle, a.stage_kernel) == (b.time, b.dt, b.ncycle, b.stage_kernel) and a.ncycle == 6
    for x, y in zip(prims(a), prims(b)):
        assert same_bits(x, y)
    a.close(), b.close()


@pytest.mark.parametrize("name", ["blast_amr", "disk_dust_amr"])
def test_refined_meshes(hiplib, name):
    """the refined cylindrical blast (three levels) and the refined dusty disk: every leaf zone's centre, every block's faces
    (the coarse-fine ones among them), uniform points; a plan made before a remesh answers by the new blocks afterwards"""
    from artemis_amd.driver import Simulation
    case, names, cycles = ((amr_cases.blast_amr(), GAS, 3) if name == "blast_amr" else (amr_cases.disk_planet_dust_amr(), DUSTY, 6))
    s = Simulation(DECK(*case["deck"]), case["overrides"])
    bounds, nx, lo, hi = mesh_of(s)
    early = s.sample_plan(ref.uniform_points(lo, hi, 4099, 4))
    s.evolve(cycles)
    bounds, nx, lo, hi = mesh_of(s)
    assert len({s.block_level(b) for b in range(s.nblocks)}) >= 2
    agree(s, ref.centre_points(bounds, nx, s.ng), names, "centres")
    agree(s, ref.face_points(bounds, nx, s.ng), names, "faces")
    pts = ref.uniform_points(lo, hi, 4099, 4)
    loc = agree(s, pts, names, "uniform")
    assert np.array_equal(early.block, loc[:, 0]) and same_bits(early.values(names), ref.pick(s.gather(names), loc))
    s.close()


def test_loop_back_communicator_gives_the_one_rank_values(hiplib, option):
    """the blocks' ghost slabs routed through the communicator: same blocks, same bits, the derived components included"""
    from artemis_amd.driver import RcclComm, Simulation
    ov = BLAST32 + ["parthenon/time/nlim=3"]
    one = Simulation(DECK("blast", "blast.in"), ov)
    one.evolve()
    bounds, nx, lo, hi = mesh_of(one)
    pts = ref.uniform_points(lo, hi, 2051, 9)
    want, blk = one.sample(GAS, pts)
    option("loopback_comm", 1)
    comm = RcclComm(0, 1)
    try:
        sim = Simulation(DECK("blast", "blast.in"), ov, comm=comm)
        sim.evolve()
        got, blk2 = sim.sample(GAS, pts)
        assert same_bits(got, want) and np.array_equal(blk, blk2) and (blk >= 0).all()
        agree(sim, pts, GAS)
        sim.close()
    finally:
        comm.close()
        one.close()
