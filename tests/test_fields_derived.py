"""GPU tests of the derived field outputs -- gas/dust.derived.divergence and .vorticity (codes 16 .. 19; include/artemis_hip.h,
"derived variables") -- through artemis_hip_pack_fields, _pack_fields_level, _reduce_fields and _reduce_fields_level on packs
and through Simulation.gather / write_fields and the deck's `fld` blocks on the host driver.  Only repository code runs here.

Every comparison is bitwise: the definition is emulated in numpy (tests/fields_derived_ref.py) from the pack's ghosted
primitives, the oracle's areas and volumes and the metric tables, and its q goes through the numpy emulations of the level
and reduce modes.  The ghost zones of the packs hold random values like the interiors, so a kernel that read the wrong
neighbour, a corner, or an interior value in place of a ghost one could not agree.  The shapes are the smallest on which the
64 x 4 tiling can go wrong."""
import ctypes as C
import os

import numpy as np
import pytest

import amr_cases
from fields_derived_ref import DUST_DIV, DUST_VORT, GAS_DIV, GAS_VORT, BlockGeometry, block_components
from fields_derived_worker import reference
from fields_level_ref import resample, same_bits
from fields_reduce_level_ref import out_shape_level, reduce_block_level
from fields_reduce_ref import reduce_block, subsets
from test_fields import BLAST32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)
GAS = [GAS_DIV, GAS_VORT]
ALL = [GAS_VORT, DUST_DIV, GAS_DIV, DUST_VORT]

# name: (nblocks, nx, lo, hi, ns_gas, ns_dust, coordinates); two ghost zones everywhere
PACKS = {
    "cart3d": (1, (70, 6, 3), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 0, "cartesian"),  # two 64-wide tiles with a ragged tail, FTY ragged
    "cart2d": (1, (8, 5, 1), (-1, -0.5, -0.5), (1, 0.8, 0.5), 1, 0, "cartesian"),
    "cart1d": (1, (8, 1, 1), (0, -0.5, -0.5), (1, 0.5, 0.5), 1, 0, "cartesian"),
    "cyl2d": (1, (8, 5, 1), (0.5, 0.0, -0.5), (2.0, 6.0, 0.5), 1, 0, "cylindrical"),
    "cyl3d": (1, (8, 5, 3), (0.5, 0.0, -1.0), (2.0, 6.0, 1.0), 1, 2, "cylindrical"),  # gas and two dust species
    "axi2d": (1, (8, 5, 1), (0.5, -1.0, -0.5), (2.0, 1.0, 0.5), 1, 0, "axisymmetric"),
    "sph1d": (1, (8, 1, 1), (0.3, 0.0, -0.5), (1.7, 3.0, 0.5), 1, 0, "spherical"),
    "sph2d": (1, (8, 5, 1), (0.3, 0.7, -0.5), (1.7, 2.5, 0.5), 1, 0, "spherical"),
    "sph3d": (1, (8, 5, 3), (0.3, 0.7, 0.0), (1.7, 2.5, 6.0), 2, 0, "spherical"),  # two gas species
    "three": (3, (70, 6, 3), (-1, -0.5, 0.25), (2, 0.8, 0.95), 1, 1, "cartesian"),  # block ranges
    "levels3d": (5, (16, 8, 8), (0.5, 0.0, -1.0), (5.5, 6.0, 1.0), 1, 1, "cylindrical"),
    "levels2d": (5, (16, 8, 1), (-1, -0.5, -0.5), (4.0, 0.8, 0.5), 1, 0, "cartesian"),
}
NG = 2


def block_bounds(name):
    nb, nx, lo, hi = PACKS[name][:4]
    edges = np.linspace(lo[0], hi[0], nb + 1)  # the blocks side by side along x1
    return [[edges[b], lo[1], lo[2]] for b in range(nb)], [[edges[b + 1], hi[1], hi[2]] for b in range(nb)]


def make_pack(name, seed=13):
    """(pack, host copies of its primitive arrays): random primitives in every zone, ghost zones included"""
    import torch
    from artemis_amd.pack import MeshBlockPack
    nb, nx, lo, hi, nsg, nsd, coords = PACKS[name]
    xmin, xmax = block_bounds(name)
    mb = MeshBlockPack(nb, nx, xmin, xmax, ng=NG, ns_gas=nsg, ns_dust=nsd, gamma=1.4, dfloor=0.7, siefloor=0.75, dust_dfloor=0.65,
                       coordinates=coords, with_fluxes=False)
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.5, 2.0, size=tuple(mb.gas_prim.shape))
    g[:, nsg:4 * nsg] = rng.uniform(-1.5, 1.5, size=g[:, nsg:4 * nsg].shape)
    d = rng.uniform(0.5, 2.0, size=tuple(mb.dust_prim.shape))
    d[:, nsd:] = rng.uniform(-1.5, 1.5, size=d[:, nsd:].shape)
    mb.gas_prim.copy_(torch.from_numpy(g))
    mb.dust_prim.copy_(torch.from_numpy(d))
    mb.gas_u0.fill_(-555.0), mb.dust_u0.fill_(-555.0)  # no conserved array is read
    return mb, g, d


@pytest.fixture(scope="module")
def definition():
    """name -> ({derived variable: [nb, ncomp, nz, ny, nx]}, volumes per block): formed once per pack, shared, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            nb, nx, lo, hi, nsg, nsd, coords = PACKS[name]
            _, g, d = make_pack(name)
            xmin, xmax = block_bounds(name)
            geo = [BlockGeometry(nx, xmin[b], xmax[b], NG, coords) for b in range(nb)]
            want = {v: np.stack([block_components([v], g[b], d[b], nsg, nsd, geo[b]) for b in range(nb)])
                    for v in (ALL if nsd else GAS)}
            vols = [G.volumes() for G in geo]
            for a in list(want.values()) + vols:
                a.setflags(write=False)
            cache[name] = (want, vols)
        return cache[name]
    return get


def code_of(name):
    from artemis_amd import capi
    return name if isinstance(name, int) else {**capi.FIELD_VAR, **capi.DERIVED_FIELD_VAR}[name]


def device_fields(mb, names, block0=0, nblocks=None, single=False, axes=0, shifts=None, expect=0):
    """One of the four entry points -- axes: artemis_hip_reduce_fields*, shifts: *_level -- on blocks [block0, block0 + nblocks):
    the filled part of the output as a flat array (the NaN-filled buffer as the call left it where expect != 0)"""
    import torch
    nblocks = (mb.nb - block0 if shifts is None else len(shifts)) if nblocks is None else nblocks
    sel = (C.c_int * max(len(names), 1))(*[code_of(n) for n in names])
    head = (C.byref(mb.pack), block0, nblocks, len(names), sel, int(single))
    tail = ([axes] if axes else []) + ([(C.c_int * max(len(shifts), 1))(*shifts)] if shifts is not None else [])
    stem = "artemis_hip_" + ("reduce_fields" if axes else "pack_fields") + ("_level" if shifts is not None else "")
    esz = 4 if single else 8
    if stem == "artemis_hip_pack_fields":
        nbytes = mb.L.artemis_hip_pack_fields_bytes(C.byref(mb.pack), len(names), sel, int(single)) // mb.nb * max(nblocks, 0)
    else:
        nbytes = getattr(mb.L, stem + "_bytes")(*head, *tail)
    wbytes = getattr(mb.L, stem + "_work_bytes")(*head, *tail) if axes else 0
    out = torch.full((nbytes // esz + 4096,), float("nan"), dtype=torch.float32 if single else torch.float64, device=mb.dev)
    work = torch.full((wbytes // 8 + 4096,), float("nan"), dtype=torch.float64, device=mb.dev)
    args = head + tuple(tail) + (C.c_void_p(out.data_ptr()),) + ((C.c_void_p(work.data_ptr()),) if axes else ()) + (mb._stream(),)
    rc = getattr(mb.L, stem)(*args)
    torch.cuda.synchronize()
    assert rc == expect, (rc, mb.L.artemis_hip_last_error().decode())
    flat = out.cpu().numpy()
    if expect:
        assert nbytes == 0 or nblocks < 0
        return flat
    assert np.isnan(flat[nbytes // esz:]).all() and not np.isnan(flat[:nbytes // esz]).any()  # all of it and nothing past the end
    return flat[:nbytes // esz]


def ncomp_of(mb, names):
    return sum((3 if n.endswith(("velocity", "momentum", "vorticity")) else 1) * (mb.nsd if n.startswith("dust") else mb.nsg) for n in names)


def blocks_of(mb, flat, names, shapes, extra=0):
    """the per-block arrays [ncomp + extra, nz', ny', nx'] of a flat output"""
    out, at = [], 0
    for shape in shapes:
        full = (ncomp_of(mb, names) + extra,) + tuple(shape)
        out.append(flat[at:at + int(np.prod(full))].reshape(full))
        at += int(np.prod(full))
    assert at == flat.size
    return out


SYSTEMS = ["cart3d", "cart2d", "cart1d", "cyl2d", "cyl3d", "axi2d", "sph1d", "sph2d", "sph3d", "three"]


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_pack_fields_equals_the_definition(hiplib, definition, name, single):
    """every coordinate system in 1-D / 2-D / 3-D, several species, block ranges with block0 > 0, both precisions; nothing is
    written to the pack"""
    mb, g, d = make_pack(name)
    want, _ = definition(name)
    names = ALL if mb.nsd else [GAS_VORT, GAS_DIV]
    shape = (mb.nx[2], mb.nx[1], mb.nx[0])
    ranges = [(0, 2), (2, 1), (1, 2)] if name == "three" else [(0, mb.nb)]
    for b0, n in ranges:
        got = np.stack(blocks_of(mb, device_fields(mb, names, b0, n, single), names, [shape] * n))
        ref = np.concatenate([want[v][b0:b0 + n] for v in names], axis=1)
        assert same_bits(got, ref.astype(np.float32) if single else ref), (name, b0, np.abs(got - ref).max())
    assert np.any(ref != 0.0)
    if mb.nx[1] == 1:  # a one-zone direction gives the literal +0.0 terms: w_1 of a 1-D pack has no other
        w1 = np.stack(blocks_of(mb, device_fields(mb, [GAS_VORT]), [GAS_VORT], [shape] * mb.nb))[:, 0]
        assert same_bits(w1, np.zeros_like(w1))
    assert np.array_equal(mb.gas_prim.cpu().numpy(), g) and np.array_equal(mb.dust_prim.cpu().numpy(), d)
    assert (mb.gas_u0 == -555.0).all()


def test_pack_fields_by_grid_stride_trips(hiplib, definition):
    """GRID_CAP = 1: one workgroup walks every tile of the three blocks"""
    from artemis_amd import capi
    mb, _, _ = make_pack("three")
    want, _ = definition("three")
    with capi.option("grid_cap", 1):
        got = device_fields(mb, ALL)
    assert same_bits(got, np.concatenate([want[v] for v in ALL], axis=1).reshape(-1))


MIXED = [GAS_VORT, "gas.prim.density", GAS_DIV, "gas.cons.momentum"]


def mixed_reference(mb, want):
    """[nb, 8, nz, ny, nx]: the components of MIXED -- the definition's for the derived, the plain kernel's own for the plain"""
    shape = (mb.nx[2], mb.nx[1], mb.nx[0])
    plain = np.stack(blocks_of(mb, device_fields(mb, [MIXED[1], MIXED[3]]), [MIXED[1], MIXED[3]], [shape] * mb.nb))
    return np.concatenate([want[GAS_VORT], plain[:, 0:1], want[GAS_DIV], plain[:, 1:4]], axis=1)


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name", ["levels3d", "levels2d"])
def test_pack_fields_level_takes_the_derived_components(hiplib, definition, name, single):
    """shifts +1, +2, +3, -1, -2 mixed in one call, derived and plain codes in one selection"""
    mb, _, _ = make_pack(name)
    want, vols = definition(name)
    q = mixed_reference(mb, want)
    shifts = (1, 2, 3, -1, -2)
    shapes = [out_shape_level(mb.nx, 0, s) for s in shifts]
    got = blocks_of(mb, device_fields(mb, MIXED, single=single, shifts=shifts), MIXED, shapes)
    plain = blocks_of(mb, device_fields(mb, [MIXED[1], MIXED[3]], single=single, shifts=shifts), [MIXED[1], MIXED[3]], shapes)
    for b, s in enumerate(shifts):
        assert same_bits(got[b], resample(q[b], vols[b], s, single)), (name, b, s)
        assert same_bits(got[b][[3, 5, 6, 7]], plain[b]), (name, b, s)  # the plain components of a call without the derived ones
    if mb.nsd:
        dust = blocks_of(mb, device_fields(mb, [DUST_VORT], single=single, shifts=shifts), [DUST_VORT], shapes)
        for b, s in enumerate(shifts):
            assert same_bits(dust[b], resample(want[DUST_VORT][b], vols[b], s, single)), (name, b, s)


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name", ["cart3d", "levels3d", "levels2d", "cart1d"])
def test_reduce_fields_takes_the_derived_components(hiplib, definition, name, single):
    """every subset of the active directions (a row of 70 is a chunk of 64 and a tail), then s = +1 and -1 on a chosen level"""
    mb, _, _ = make_pack(name)
    want, vols = definition(name)
    q = mixed_reference(mb, want)
    for axes in subsets(mb.nx):
        shape = out_shape_level(mb.nx, axes, 0)
        got = blocks_of(mb, device_fields(mb, MIXED, single=single, axes=axes), MIXED, [shape] * mb.nb, extra=1)
        for b in range(mb.nb):
            assert same_bits(got[b], reduce_block(q[b], vols[b], axes, single)), (name, axes, b)
        only = blocks_of(mb, device_fields(mb, [GAS_DIV], single=single, axes=axes), [GAS_DIV], [shape] * mb.nb, extra=1)
        for b in range(mb.nb):  # a selection of derived codes alone: the volume row comes from the derived pass
            assert same_bits(only[b], got[b][[4, 8]]), (name, axes, b)
        if name.startswith("levels"):
            shifts = (1, -1, 0, 1, -1)
            lv = blocks_of(mb, device_fields(mb, MIXED, single=single, axes=axes, shifts=shifts), MIXED,
                           [out_shape_level(mb.nx, axes, s) for s in shifts], extra=1)
            for b, s in enumerate(shifts):
                assert same_bits(lv[b], reduce_block_level(q[b], vols[b], axes, s, single)), (name, axes, b, s)


def test_codes_the_entry_points_refuse_and_the_sizes_they_report(hiplib):
    from artemis_amd import capi
    gas_only, _, _ = make_pack("sph3d")  # two gas species, no dust
    dusty, _, _ = make_pack("cyl3d")     # one gas and two dust species
    for code in (12, 13, 14, 15, 20, 1000, -1):
        device_fields(gas_only, [0, code], expect=capi.EINVAL)
        assert b"unknown variable code" in gas_only.L.artemis_hip_last_error()
    for code in (18, 19):
        device_fields(gas_only, [16, code], expect=capi.EINVAL)
        assert b"a dust variable on a pack without dust" in gas_only.L.artemis_hip_last_error()
        device_fields(gas_only, [code], axes=1, expect=capi.EINVAL)
        device_fields(gas_only, [code], shifts=(0,), expect=capi.EINVAL)
    zones = 8 * 5 * 3
    sel = lambda *c: (C.c_int * len(c))(*c)
    L = dusty.L
    assert L.artemis_hip_pack_fields_bytes(C.byref(gas_only.pack), 2, sel(16, 17), 0) == (1 + 3) * 2 * zones * 8
    assert L.artemis_hip_pack_fields_bytes(C.byref(dusty.pack), 4, sel(16, 17, 18, 19), 1) == ((1 + 3) + (1 + 3) * 2) * zones * 4
    assert L.artemis_hip_pack_fields_level_bytes(C.byref(dusty.pack), 0, 1, 1, sel(19), 0, sel(-1)) == 6 * zones * 8 * 8
    assert L.artemis_hip_reduce_fields_bytes(C.byref(dusty.pack), 0, 1, 2, sel(17, 18), 0, 1) == (3 + 2 + 1) * 5 * 3 * 8
    assert L.artemis_hip_reduce_fields_level_bytes(C.byref(dusty.pack), 0, 1, 1, sel(16), 0, 4, sel(0)) == 2 * 8 * 5 * 8
    assert L.artemis_hip_reduce_fields_work_bytes(C.byref(dusty.pack), 0, 1, 1, sel(16), 0, 7) > 0
    import torch
    buf = torch.zeros(64 * zones, dtype=torch.float64, device=dusty.dev)
    for code in (16, 17, 18, 19):
        rc = L.artemis_hip_unpack_fields(C.byref(dusty.pack), 0, 1, 4, sel(0, 1, 3, code), 0, C.c_void_p(buf.data_ptr()), dusty._stream())
        assert rc == capi.EINVAL and b"is an output, not part of a state" in L.artemis_hip_last_error()
    rc = L.artemis_hip_unpack_fields(C.byref(dusty.pack), 0, 1, 1, sel(12), 0, C.c_void_p(buf.data_ptr()), dusty._stream())
    assert rc == capi.EINVAL and b"unknown variable code 12" in L.artemis_hip_last_error()


# ---- host driver ------------------------------------------------------------------------------------------------------
def prims(s):
    return [s.field("gas.prim", b)[[0, 1, 2, 3, 5]] for b in range(s.nblocks)]  # (the pressure slot of a ghost zone is no state)


@pytest.mark.parametrize("split", [False, True], ids=["one_block", "eight_blocks"])
def test_gather_on_the_tuned_sedov_path_and_a_block_due_mid_run(hiplib, tmp_path, split):
    """32^3 blast on the tuned kernel (outflow faces: the stage loop leaves ghost zones for later), in one block and in 2 x 2 x 2:
    gather after evolve(3) equals the definition formed from field(); a `fld` block with a derived variable that comes due
    mid-run holds, in every dump, the gather of a run stopped at that cycle, and the run's final state equals that of the run
    without outputs, bit for bit"""
    from artemis_amd.driver import Simulation
    from artemis_amd.fields import read_fields
    ov = (BLAST32 if split else [o for o in BLAST32 if "meshblock" not in o] +
          ["parthenon/meshblock/nx%d=32" % d for d in (1, 2, 3)]) + ["parthenon/time/nlim=6"]
    names = [GAS_VORT, "gas.prim.density", GAS_DIV]
    fld = ["parthenon/output1/file_type=fld", "parthenon/output1/dt=0.005", "parthenon/output1/variables=" + ", ".join(names)]
    a, b = Simulation(DECK("blast", "blast.in"), ov), Simulation(DECK("blast", "blast.in"), ov + fld)
    assert a.uses_tuned_kernel and a.nblocks == (8 if split else 1)
    b.enable_outputs(tmp_path)
    a.evolve(3)
    got = a.gather(GAS)
    assert same_bits(got, reference(a, GAS, "cartesian")) and np.abs(got).max() > 0.0
    assert same_bits(a.gather(GAS, single=True), got.astype(np.float32))
    a.evolve(), b.evolve()
    assert (a.time, a.dt, a.ncycle, a.stage_kernel) == (b.time, b.dt, b.ncycle, b.stage_kernel) and a.ncycle == 6
    for x, y in zip(prims(a), prims(b)):
        assert same_bits(x, y)
    assert {blk["index"]: blk["status"] for blk in b.outputs()["blocks"]}[1] == "active"
    dumps = sorted(f for f in os.listdir(tmp_path) if "final" not in f)
    cycles = [read_fields(tmp_path / f).cycle for f in dumps]
    assert len(dumps) >= 3 and cycles[0] == 0 and 0 < cycles[1] < 6
    c = Simulation(DECK("blast", "blast.in"), ov)
    for f, cycle in zip(dumps, cycles):
        c.evolve(cycle - c.ncycle)
        fd = read_fields(tmp_path / f)
        want = reference(c, GAS, "cartesian")
        assert same_bits(fd.get(GAS_DIV), want[:, 0:1]) and same_bits(fd.get(GAS_VORT), want[:, 1:4]), f
        assert same_bits(fd.get("gas.prim.density"), c.gather(["gas.prim.density"]))
    for s in (a, b, c):
        s.close()


def test_strat_conditions_inside_the_row_march(hiplib):
    """ssheet.in in 2-D: the row march forms the x1 `extrap` and x2 `inflow` conditions on the rows it loads and fills no ghost
    zone between cycles; a derived request fills them first.  Gas and one dust species."""
    from artemis_amd.driver import Simulation
    ov = ["parthenon/mesh/nx1=61", "parthenon/mesh/nx2=40", "parthenon/meshblock/nx1=61", "parthenon/meshblock/nx2=40", "parthenon/time/nlim=6",
          "physics/dust=true", "physics/drag=true", "dust/nspecies=1", "dust/cfl=0.3", "dust/reconstruct=plm", "dust/riemann=hlle",
          "dust/dfloor=1.0e-10", "dust/stopping_time/type=constant", "dust/stopping_time/tau=0.1", "drag/type=simple_dust"]
    a, b = Simulation(DECK("ssheet", "ssheet.in"), ov), Simulation(DECK("ssheet", "ssheet.in"), ov)
    a.evolve(3), b.evolve(3)
    assert a.stage_kernel == "stage2d_kernel"
    got = a.gather(ALL)
    assert same_bits(got, reference(a, ALL, "cartesian")) and np.abs(got).max() > 0.0
    a.evolve(), b.evolve()
    assert a.ncycle == b.ncycle == 6 and a.dt == b.dt
    assert same_bits(a.field("gas.prim")[[0, 1, 2, 3, 5]], b.field("gas.prim")[[0, 1, 2, 3, 5]]) and same_bits(a.field("dust.prim"), b.field("dust.prim"))
    a.close(), b.close()


def test_refined_disk_with_dust_where_coarse_fine_ghost_values_enter(hiplib):
    """amr_cases.disk_planet_dust_amr at its test size (n = 32: the cylindrical disk with a planet, `ic` conditions, the
    rotating frame, gas and one dust species, four levels): all four names equal the definition formed from field() -- the
    neighbour across a coarse-fine boundary is the prolongated or restricted ghost value, for the dust as for the gas -- and
    level = L and reduce with reduce_level go through the same q"""
    from artemis_amd.driver import Simulation
    case = amr_cases.disk_planet_dust_amr()
    s = Simulation(DECK(*case["deck"]), case["overrides"])
    s.evolve(6)
    levels = [s.block_level(b) for b in range(s.nblocks)]
    assert len(set(levels)) >= 2 and s.ns_dust == 1
    q = s.gather(ALL)
    assert q.shape[1] == 8 and same_bits(q, reference(s, ALL, "cylindrical"))
    assert all(np.abs(q[:, c]).max() > 0.0 for c in (2, 3, 4, 7))  # w_3 and div of the gas and of the dust
    assert same_bits(s.gather(ALL, single=True), q.astype(np.float32))
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    vols = []
    for b in range(s.nblocks):
        bd = s.block_bounds(b)
        vols.append(BlockGeometry(nx, bd[0::2], bd[1::2], s.ng, "cylindrical").volumes())
    L = max(levels) - 1
    lev, red = s.gather(ALL, level=L), s.gather(ALL, reduce=("x2",), reduce_level=L)
    own = s.gather(ALL, reduce=("x1",))
    for b in range(s.nblocks):
        assert same_bits(lev[b], resample(q[b], vols[b], levels[b] - L)), b
        assert same_bits(red[b], reduce_block_level(q[b], vols[b], 2, levels[b] - L)), b
        assert same_bits(own[b], reduce_block(q[b], vols[b], 1)), b
    s.close()


def test_refined_blast_where_coarse_fine_ghost_values_enter(hiplib):
    """blast_amr.in at its test size (cylindrical, gas only, outflow faces, three levels), beside the disk above: the neighbour
    across a coarse-fine boundary is the prolongated or restricted ghost value of field(); level = L and reduce with
    reduce_level go through the same q"""
    from artemis_amd.driver import Simulation
    case = amr_cases.blast_amr()
    s = Simulation(DECK(*case["deck"]), case["overrides"])
    s.evolve(3)
    levels = [s.block_level(b) for b in range(s.nblocks)]
    assert len(set(levels)) >= 2
    q = s.gather(GAS)
    assert same_bits(q, reference(s, GAS, "cylindrical")) and np.abs(q).max() > 0.0
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    vols = []
    for b in range(s.nblocks):
        bd = s.block_bounds(b)
        vols.append(BlockGeometry(nx, bd[0::2], bd[1::2], s.ng, "cylindrical").volumes())
    at1, red = s.gather(GAS, level=1), s.gather(GAS, reduce=("x2",), reduce_level=1)
    for b in range(s.nblocks):
        assert same_bits(at1[b], resample(q[b], vols[b], levels[b] - 1)), b
        assert same_bits(red[b], reduce_block_level(q[b], vols[b], 2, levels[b] - 1)), b
    s.close()


def test_loop_back_communicator_gives_the_one_rank_arrays(hiplib, option):
    """the blocks' ghost slabs routed through the communicator (two virtual halves of the block list): same bits"""
    from artemis_amd.driver import RcclComm, Simulation
    ov = BLAST32 + ["parthenon/time/nlim=3"]
    ref = Simulation(DECK("blast", "blast.in"), ov)
    ref.evolve()
    want = ref.gather(GAS)
    option("loopback_comm", 1)
    comm = RcclComm(0, 1)
    try:
        sim = Simulation(DECK("blast", "blast.in"), ov, comm=comm)
        sim.evolve()
        got = sim.gather(GAS)
        assert same_bits(got, want) and same_bits(got, reference(sim, GAS, "cartesian"))
        sim.close()
    finally:
        comm.close()
        ref.close()
