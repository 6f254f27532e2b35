"""GPU tests of the field outputs: artemis_hip_pack_fields (kernels_fields.hip) on packs, Simulation.gather / write_fields and
the deck's `fld` blocks on the host driver.  Only repository code runs here.

Every comparison is bitwise: the kernel forms each value with PrimToCons's expressions and operation order, so it has to
equal what artemis_hip_prim_to_cons leaves in the arrays of a copy of the pack (double), or np.float32 of that (float: one
correctly rounded narrowing).  The shapes are the smallest at which the 64 x 4 tiling, its masking and the curvilinear scale
factors can go wrong: no extent is a multiple of the tile, one has several tiles along x1, 1-D / 2-D / 3-D."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import amr_cases
from test_outputs import BLAST_CART, state_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)

GAS = ["gas.prim.density", "gas.prim.velocity", "gas.prim.pressure", "gas.prim.sie", "gas.cons.density", "gas.cons.momentum",
       "gas.cons.total_energy", "gas.cons.internal_energy"]
DUST = ["dust.prim.density", "dust.prim.velocity", "dust.cons.density", "dust.cons.momentum"]
SHIPPED = ["gas.prim.density", "gas.prim.velocity", "gas.prim.pressure"]

# name: (nblocks, nx, lo, hi, ns_gas, ns_dust, coordinates, ng)
PACKS = {
    "cart3d": (1, (20, 6, 5), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 2, "cartesian", 2),
    "cart2d": (1, (61, 40, 1), (-1, -0.5, -0.5), (1, 0.8, 0.5), 1, 0, "cartesian", 3),
    "cart1d": (1, (131, 1, 1), (0, -0.5, -0.5), (1, 0.5, 0.5), 2, 0, "cartesian", 2),
    "cyl3d": (1, (16, 8, 6), (0.5, 0.0, -1.0), (2.0, 6.0, 1.0), 1, 1, "cylindrical", 2),
    "sph3d": (1, (16, 8, 6), (0.3, 0.7, 0.0), (1.7, 2.5, 6.0), 1, 0, "spherical", 2),
    "three_blocks": (3, (20, 6, 5), (-1, -0.5, 0.25), (2, 0.8, 0.95), 1, 1, "cartesian", 2),
}
# floors that bind: densities and sie are drawn from [0.5, 2), so about a seventh of the zones sit below each
DFLOOR, SIEFLOOR, DUST_DFLOOR = 0.7, 0.75, 0.65


def make_pack(name, seed=7):
    """(pack, host copies of its primitive arrays): random primitives in every zone, ghost zones included"""
    import torch
    from artemis_amd.pack import MeshBlockPack
    nb, nx, lo, hi, nsg, nsd, coords, ng = PACKS[name]
    edges = np.linspace(lo[0], hi[0], nb + 1)  # the blocks side by side along x1
    xmin = [[edges[b], lo[1], lo[2]] for b in range(nb)]
    xmax = [[edges[b + 1], hi[1], hi[2]] for b in range(nb)]
    mb = MeshBlockPack(nb, nx, xmin, xmax, ng=ng, ns_gas=nsg, ns_dust=nsd, gamma=1.4, dfloor=DFLOOR, siefloor=SIEFLOOR,
                       dust_dfloor=DUST_DFLOOR, coordinates=coords, with_fluxes=False)
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.5, 2.0, size=tuple(mb.gas_prim.shape))
    g[:, nsg:4 * nsg] = rng.uniform(-1.5, 1.5, size=g[:, nsg:4 * nsg].shape)
    g[:, 4 * nsg:5 * nsg] = -777.0  # the stored pressure is stale: nothing may read it
    d = rng.uniform(0.5, 2.0, size=tuple(mb.dust_prim.shape))
    d[:, nsd:] = rng.uniform(-1.5, 1.5, size=d[:, nsd:].shape)
    mb.gas_prim.copy_(torch.from_numpy(g))
    mb.dust_prim.copy_(torch.from_numpy(d))
    mb.gas_u0.fill_(-555.0), mb.dust_u0.fill_(-555.0)  # ... and no conserved array either
    return mb, g, d


def interior(mb, a):
    return a[:, :, mb.ks:mb.ke + 1, mb.js:mb.je + 1, mb.is_:mb.ie + 1]


@pytest.fixture(scope="module")
def expected():
    """name -> {variable: [nb, ncomp, nx3, nx2, nx1]}: the interiors of what artemis_hip_prim_to_cons leaves in a copy of the
    pack; computed once per pack and shared"""
    import torch
    cache = {}

    def get(name):
        if name not in cache:
            ref, _, _ = make_pack(name)
            ref.PrimToCons()
            torch.cuda.synchronize()
            gp, gu = interior(ref, ref.gas_prim.cpu().numpy()), interior(ref, ref.gas_u0.cpu().numpy())
            dp, du = interior(ref, ref.dust_prim.cpu().numpy()), interior(ref, ref.dust_u0.cpu().numpy())
            n, m = ref.nsg, ref.nsd
            want = {"gas.prim.density": gp[:, 0:n], "gas.prim.velocity": gp[:, n:4 * n], "gas.prim.pressure": gp[:, 4 * n:5 * n],
                    "gas.prim.sie": gp[:, 5 * n:6 * n], "gas.cons.density": gu[:, 0:n], "gas.cons.momentum": gu[:, n:4 * n],
                    "gas.cons.total_energy": gu[:, 4 * n:5 * n], "gas.cons.internal_energy": gu[:, 5 * n:6 * n],
                    "dust.prim.density": dp[:, 0:m], "dust.prim.velocity": dp[:, m:4 * m], "dust.cons.density": du[:, 0:m],
                    "dust.cons.momentum": du[:, m:4 * m]}
            cache[name] = {k: np.ascontiguousarray(v) for k, v in want.items()}
        return cache[name]
    return get


def pack_fields(mb, names, block0=0, nblocks=None, single=False, expect=0):
    """artemis_hip_pack_fields of blocks [block0, block0 + nblocks) as a numpy array [nblocks, ncomp, nx3, nx2, nx1]"""
    import torch
    from artemis_amd import capi
    nblocks = mb.nb - block0 if nblocks is None else nblocks
    sel = (C.c_int * max(len(names), 1))(*[n if isinstance(n, int) else capi.FIELD_VAR[n] for n in names])
    zones = mb.nx[0] * mb.nx[1] * mb.nx[2]
    nbytes = mb.L.artemis_hip_pack_fields_bytes(C.byref(mb.pack), len(names), sel, int(single))
    esz = 4 if single else 8
    if expect:
        assert nbytes == 0 or nblocks < 0 or block0 < 0 or block0 + nblocks > mb.nb
    assert nbytes % (mb.nb * zones * esz) == 0
    ncomp = nbytes // (mb.nb * zones * esz)
    out = torch.full((max(nblocks, 1), max(ncomp, 1)) + (mb.nx[2], mb.nx[1], mb.nx[0]), float("nan"),
                     dtype=torch.float32 if single else torch.float64, device=mb.dev)
    rc = mb.L.artemis_hip_pack_fields(C.byref(mb.pack), block0, nblocks, len(names), sel, int(single), C.c_void_p(out.data_ptr()),
                                      mb._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, mb.L.artemis_hip_last_error().decode())
    return out.cpu().numpy()[:max(nblocks, 0), :ncomp]


def names_of(mb):
    return GAS + (DUST if mb.nsd else [])


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name", list(PACKS))
def test_pack_fields_equals_prim_to_cons(hiplib, expected, name, single):
    mb, g, d = make_pack(name)
    want = expected(name)
    names = names_of(mb)
    shuffled = [names[q] for q in np.random.default_rng(3).permutation(len(names))] + [names[2]]  # (a name may repeat)
    assert shuffled[:len(names)] != names
    for order in (names, shuffled):
        ranges = [(0, 2), (2, 1)] if name == "three_blocks" else [(0, mb.nb)]
        got = np.concatenate([pack_fields(mb, order, b0, n, single) for b0, n in ranges], axis=0)
        ref = np.concatenate([want[v] for v in order], axis=1)
        ref = ref.astype(np.float32) if single else ref
        assert got.dtype == ref.dtype and got.shape == ref.shape and not np.isnan(got).any()
        at = 0
        for v in order:
            n = want[v].shape[1]
            assert np.array_equal(got[:, at:at + n], ref[:, at:at + n]), (name, v)
            at += n
    # nothing was written to the pack, ghost zones included, and nothing was read from the pressure slot or from cons
    assert np.array_equal(mb.gas_prim.cpu().numpy(), g) and np.array_equal(mb.dust_prim.cpu().numpy(), d)
    assert (mb.gas_u0 == -555.0).all() and (mb.dust_u0 == -555.0).all()


def test_floors_bind_and_the_derived_values_follow_them(hiplib, expected):
    mb, g, d = make_pack("cart3d")
    raw_rho, raw_sie = interior(mb, g)[:, 0:1], interior(mb, g)[:, 5:6]
    vel = interior(mb, g)[:, 1:4]
    low_rho, low_sie = raw_rho < DFLOOR, raw_sie < SIEFLOOR
    assert low_rho.sum() > 20 and low_sie.sum() > 20 and (low_rho & low_sie).sum() > 2
    rho, sie, pres, eint, etot, mom = [pack_fields(mb, [v]) for v in ("gas.prim.density", "gas.prim.sie", "gas.prim.pressure",
                                                                     "gas.cons.internal_energy", "gas.cons.total_energy",
                                                                     "gas.cons.momentum")]
    assert np.array_equal(rho, np.maximum(raw_rho, DFLOOR)) and np.array_equal(sie, np.maximum(raw_sie, SIEFLOOR))
    assert np.all(rho[low_rho] == DFLOOR) and np.all(sie[low_sie] == SIEFLOOR)
    assert np.array_equal(pres, (1.4 - 1.0) * rho * sie) and np.array_equal(eint, sie * rho)
    assert np.array_equal(etot, eint + 0.5 * rho * (vel[:, 0:1] ** 2 + vel[:, 1:2] ** 2 + vel[:, 2:3] ** 2))
    assert np.array_equal(mom, rho * vel * 1.0)
    drho = pack_fields(mb, ["dust.cons.density"])
    assert np.array_equal(drho, np.maximum(interior(mb, d)[:, 0:2], DUST_DFLOOR)) and (drho == DUST_DFLOOR).sum() > 20
    assert np.array_equal(pack_fields(mb, ["gas.prim.pressure"]), expected("cart3d")["gas.prim.pressure"])


def test_bad_arguments_are_refused(hiplib):
    from artemis_amd import capi
    gas_only, _, _ = make_pack("sph3d")
    three, _, _ = make_pack("three_blocks")
    for code in (12, -1, 1000):
        pack_fields(gas_only, [0, code], expect=capi.EINVAL)
    pack_fields(gas_only, ["gas.prim.density", "dust.prim.density"], expect=capi.EINVAL)  # a dust code on a pack without dust
    pack_fields(gas_only, ["dust.cons.momentum"], expect=capi.EINVAL)
    for b0, n in ((0, 4), (2, 2), (3, 1), (-1, 1), (0, -1), (4, 0)):
        pack_fields(three, SHIPPED, b0, n, expect=capi.EINVAL)
    assert pack_fields(three, SHIPPED, 3, 0).shape[0] == 0  # an empty range at the end is no error


# ---- host driver ------------------------------------------------------------------------------------------------------
BLAST32 = [o for o in BLAST_CART if "nx" not in o] + ["parthenon/mesh/nx1=32", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32",
                                                     "parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=16",
                                                     "parthenon/meshblock/nx3=16"]


def prim_interiors(s):
    """[nblocks, 6 ns, nz, ny, nx] of field("gas.prim"), which materialises the pressure slot"""
    return np.stack([s.interior(s.field("gas.prim", b)) for b in range(s.nblocks)])


def split(s, a):
    n = s.ns_gas
    return {"gas.prim.density": a[:, 0:n], "gas.prim.velocity": a[:, n:4 * n], "gas.prim.pressure": a[:, 4 * n:5 * n]}


def test_gather_equals_field_and_does_not_disturb_the_run(hiplib):
    """32^3 blast in 16^3 blocks on the tuned kernel: a gather after 3 cycles (before anything has materialised the
    conserved state), the run continued, against a second simulation that never gathers -- same kernel family, clock and
    fields afterwards.  The same gather through a 1 MiB staging buffer (8 blocks of 160 KiB: two block ranges) and in
    float."""
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    a = Simulation(DECK("blast", "blast.in"), BLAST32 + ["parthenon/time/nlim=6"])
    b = Simulation(DECK("blast", "blast.in"), BLAST32 + ["parthenon/time/nlim=6"])
    assert a.uses_tuned_kernel and a.nblocks == 8
    a.evolve(3), b.evolve(3)
    ga = a.gather(SHIPPED)
    assert ga.shape == (8, 5, 16, 16, 16) and ga.dtype == np.float64 and 8 * 5 * 16 ** 3 * 8 > (1 << 20)
    with capi.option("fields_stage_mb", 1):
        chunked = a.gather(SHIPPED)
        chunked32 = a.gather(SHIPPED, single=True)
    assert np.array_equal(chunked, ga) and np.array_equal(chunked32, ga.astype(np.float32)) and chunked32.dtype == np.float32
    assert np.array_equal(a.gather(SHIPPED, single=True), chunked32)
    want = prim_interiors(b)  # (b materialises here; a has not)
    assert np.array_equal(ga, np.concatenate([split(b, want)[v] for v in SHIPPED], axis=1))
    assert np.array_equal(a.gather("gas.prim.pressure")[:, 0], want[:, 4]) and want[:, 4].min() > 0.0
    a.evolve(), b.evolve()
    (ca, fa), (cb, fb) = state_of(a), state_of(b)
    assert ca == cb and ca[2] == 6 and ca[3] == "stage_fused_kernel"
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y)
    with pytest.raises(RuntimeError, match="unknown variable dust.prim.density"):
        a.gather(["gas.prim.density", "dust.prim.density"])
    a.close(), b.close()


def test_pressure_is_formed_where_no_stage_stores_it(hiplib):
    """The PPM tile march (kernels_ppm.hip) leaves the pressure slot alone, so after a few cycles the stored values are those
    of the initial condition: the gathered pressure still equals what a materialising field() of a second run shows, and
    differs from the initial one."""
    from artemis_amd.driver import Simulation
    ov = BLAST32 + ["gas/reconstruct=ppm", "parthenon/mesh/nghost=4", "parthenon/time/nlim=4"]
    a, b = Simulation(DECK("blast", "blast.in"), ov), Simulation(DECK("blast", "blast.in"), ov)
    p0 = a.gather("gas.prim.pressure")
    a.evolve(), b.evolve()
    assert a.stage_kernel == "stage_ppm_kernel" == b.stage_kernel and a.ncycle == 4
    p = a.gather("gas.prim.pressure")
    want = prim_interiors(b)
    assert np.array_equal(p[:, 0], want[:, 4]) and not np.array_equal(p, p0)
    a.close(), b.close()


def test_fld_block_through_enable_outputs(hiplib, tmp_path):
    """The deck-driven block: same clock and fields as the run without outputs, dumps where the schedule puts them, the last
    one equal to a gather at that moment."""
    from artemis_amd.driver import Simulation
    from artemis_amd.fields import read_fields
    from test_outputs import due_cycles
    ov = BLAST32 + ["parthenon/time/nlim=6"]
    blocks = ["parthenon/output1/file_type=fld", "parthenon/output1/dt=0.005", "parthenon/output1/variables=" + ", ".join(SHIPPED),
              "parthenon/output2/file_type=hdf5", "parthenon/output2/dt=0.01", "parthenon/output2/variables=" + ", ".join(SHIPPED)]
    a = Simulation(DECK("blast", "blast.in"), ov + blocks)
    a.enable_outputs(tmp_path)
    a.evolve()
    b = Simulation(DECK("blast", "blast.in"), ov)
    clock = [(0, 0.0)]
    while b.evolve(1) == 1:
        clock.append((b.ncycle, b.time))
    last = read_fields(tmp_path / "blast_cart.out1.final.fld")
    ga = a.gather(SHIPPED)
    assert np.array_equal(np.concatenate([last.get(v) for v in SHIPPED], axis=1), ga)
    assert (last.time, last.dt, last.cycle) == (a.time, a.dt, 6) and last.uniform("gas.prim.density").shape == (1, 32, 32, 32)
    (ca, fa), (cb, fb) = state_of(a), state_of(b)
    assert ca == cb and ca[3] == "stage_fused_kernel"
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y)
    assert np.array_equal(ga, np.concatenate([split(b, prim_interiors(b))[v] for v in SHIPPED], axis=1))
    due = due_cycles(clock, 0.005)
    assert len(due) >= 3 and due[0] == 0
    assert sorted(os.listdir(tmp_path)) == ["blast_cart.out1.%05d.fld" % q for q in range(len(due))] + ["blast_cart.out1.final.fld"]
    assert [read_fields(tmp_path / ("blast_cart.out1.%05d.fld" % q)).cycle for q in range(len(due))] == due
    st = {blk["index"]: blk for blk in a.outputs()["blocks"]}
    assert st[1]["status"] == "active" and st[1]["written"] == len(due) + 1 and st[2]["status"] == "skipped: hdf5 is not built"
    a.close(), b.close()


def test_refined_mesh_dump(hiplib, tmp_path):
    """blast_amr.in at its test size (cylindrical, three levels): meta.json carries the levels and bounds of the blocks, the
    values are the interiors of field(), and blocks on several levels do not make one uniform array."""
    from artemis_amd.driver import Simulation
    from artemis_amd.fields import read_fields
    case = amr_cases.blast_amr()
    s = Simulation(DECK(*case["deck"]), case["overrides"])
    s.evolve(3)
    s.write_fields(tmp_path / "amr.fld", SHIPPED)
    fd = read_fields(tmp_path / "amr.fld")
    assert len(fd.blocks) == s.nblocks == s.nblocks_global and fd.coordinates == "cylindrical" and fd.cycle == 3
    assert [b["level"] for b in fd.blocks] == [s.block_level(b) for b in range(s.nblocks)] and len({b["level"] for b in fd.blocks}) >= 2
    assert [b["bounds"] for b in fd.blocks] == [s.block_bounds(b) for b in range(s.nblocks)]
    meta = json.load(open(tmp_path / "amr.fld" / "meta.json"))
    assert [b["gid"] for b in meta["blocks"]] == list(range(s.nblocks)) == [b["index"] for b in meta["blocks"]]
    want = split(s, prim_interiors(s))
    for v in SHIPPED:
        assert np.array_equal(fd.get(v), want[v]), v
    with pytest.raises(ValueError, match="levels"):
        fd.uniform("gas.prim.density")
    s.close()
