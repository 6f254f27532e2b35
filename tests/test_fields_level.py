"""GPU tests of field outputs at a refinement level: artemis_hip_pack_fields_level (kernels_fields.hip) on packs,
Simulation.gather / write_fields with level=L and a deck's `level = L` on the host driver.

The definition (include/artemis_hip.h) is emulated in numpy (tests/fields_level_ref.py): the full-resolution components
are what artemis_hip_prim_to_cons leaves in a copy of the pack, as in tests/test_fields.py; the volumes are the CPU
oracle's face_areas(0) of a block with the same bounds (tests/test_parity_geometry.py holds the device's volumes to those).
Every comparison of values is bitwise, -0.0 included.  The shapes are the smallest at which the 64-lane tiling, the lane
groups, their alignment to the interior start and the inactive directions can go wrong."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import amr_cases
from fields_level_ref import oracle_volumes, place, resample, same_bits
from test_fields import BLAST32, DFLOOR, DUST, DUST_DFLOOR, GAS, SIEFLOOR, interior
from test_outputs import gamma, state_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)

# name: (nblocks, nx, lo, hi, ns_gas, ns_dust, coordinates, ng)
PACKS = {
    "cart3d": (1, (72, 12, 4), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 2, "cartesian", 2),  # a full tile + a tail of whole groups
    "cart3d8": (1, (72, 8, 8), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 0, "cartesian", 2),
    "cart2d": (1, (40, 24, 1), (-1, -0.5, -0.5), (1, 0.8, 0.5), 1, 0, "cartesian", 3),  # odd interior start
    "cart1d": (1, (136, 1, 1), (0, -0.5, -0.5), (1, 0.5, 0.5), 2, 0, "cartesian", 2),
    "cyl3d": (1, (16, 8, 6), (0.5, 0.0, -1.0), (2.0, 6.0, 1.0), 1, 1, "cylindrical", 2),
    "sph3d": (1, (16, 8, 6), (0.3, 0.7, 0.0), (1.7, 2.5, 6.0), 1, 0, "spherical", 2),
    "three": (3, (24, 6, 4), (-1, -0.5, 0.25), (2, 0.8, 0.95), 1, 1, "cartesian", 2),
}
# (pack, the shift of every block)
CASES = [("cart3d", (1,)), ("cart3d", (2,)), ("cart3d8", (3,)), ("cart2d", (1,)), ("cart2d", (2,)), ("cart2d", (3,)),
         ("cart1d", (1,)), ("cart1d", (2,)), ("cart1d", (3,)), ("cyl3d", (1,)), ("sph3d", (1,)), ("three", (1, 0, -1)),
         ("cart2d", (-1,)), ("cart2d", (-2,)), ("cart2d", (-3,))]


def block_bounds(name):
    nb, nx, lo, hi = PACKS[name][:4]
    edges = np.linspace(lo[0], hi[0], nb + 1)  # the blocks side by side along x1
    return [[edges[b], lo[1], lo[2]] for b in range(nb)], [[edges[b + 1], hi[1], hi[2]] for b in range(nb)]


def make_pack(name, seed=11):
    """(pack, host copies of its primitive arrays): random primitives in every zone, floors that bind, the pressure slot
    and cons poisoned -- as tests/test_fields.py builds its packs"""
    import torch
    from artemis_amd.pack import MeshBlockPack
    nb, nx, lo, hi, nsg, nsd, coords, ng = PACKS[name]
    xmin, xmax = block_bounds(name)
    mb = MeshBlockPack(nb, nx, xmin, xmax, ng=ng, ns_gas=nsg, ns_dust=nsd, gamma=1.4, dfloor=DFLOOR, siefloor=SIEFLOOR,
                       dust_dfloor=DUST_DFLOOR, coordinates=coords, with_fluxes=False)
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.5, 2.0, size=tuple(mb.gas_prim.shape))
    g[:, nsg:4 * nsg] = rng.uniform(-1.5, 1.5, size=g[:, nsg:4 * nsg].shape)
    g[:, 4 * nsg:5 * nsg] = -777.0
    d = rng.uniform(0.5, 2.0, size=tuple(mb.dust_prim.shape))
    d[:, nsd:] = rng.uniform(-1.5, 1.5, size=d[:, nsd:].shape)
    mb.gas_prim.copy_(torch.from_numpy(g))
    mb.dust_prim.copy_(torch.from_numpy(d))
    mb.gas_u0.fill_(-555.0), mb.dust_u0.fill_(-555.0)
    return mb, g, d


def full_components(mb):
    """{variable: [nb, ncomp, nx3, nx2, nx1]} of a pack's CURRENT primitives: the interiors of what artemis_hip_prim_to_cons
    leaves in the arrays (the pack's cons arrays are overwritten)"""
    import torch
    mb.PrimToCons()
    torch.cuda.synchronize()
    gp, gu = interior(mb, mb.gas_prim.cpu().numpy()), interior(mb, mb.gas_u0.cpu().numpy())
    dp, du = interior(mb, mb.dust_prim.cpu().numpy()), interior(mb, mb.dust_u0.cpu().numpy())
    n, m = mb.nsg, mb.nsd
    want = {"gas.prim.density": gp[:, 0:n], "gas.prim.velocity": gp[:, n:4 * n], "gas.prim.pressure": gp[:, 4 * n:5 * n],
            "gas.prim.sie": gp[:, 5 * n:6 * n], "gas.cons.density": gu[:, 0:n], "gas.cons.momentum": gu[:, n:4 * n],
            "gas.cons.total_energy": gu[:, 4 * n:5 * n], "gas.cons.internal_energy": gu[:, 5 * n:6 * n],
            "dust.prim.density": dp[:, 0:m], "dust.prim.velocity": dp[:, m:4 * m], "dust.cons.density": du[:, 0:m],
            "dust.cons.momentum": du[:, m:4 * m]}
    return {k: np.ascontiguousarray(v) for k, v in want.items()}


@pytest.fixture(scope="module")
def reference():
    """name -> (full-resolution components, volumes per block); computed once per pack and shared, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            nb, nx, lo, hi, nsg, nsd, coords, ng = PACKS[name]
            xmin, xmax = block_bounds(name)
            cache[name] = (full_components(make_pack(name)[0]), [oracle_volumes(nx, xmin[b], xmax[b], ng, coords) for b in range(nb)])
        return cache[name]
    return get


def out_shape(nx, s):
    return tuple(m if m == 1 else (m >> s if s >= 0 else m << -s) for m in nx)[::-1]


def pack_fields_level(mb, names, shifts, block0=0, single=False, expect=0):
    """artemis_hip_pack_fields_level of blocks [block0, block0 + len(shifts)) as a list of [ncomp, nz', ny', nx'] arrays; with
    expect != 0 the NaN-filled buffer as the call left it"""
    import torch
    from artemis_amd import capi
    sel = (C.c_int * max(len(names), 1))(*[capi.FIELD_VAR[n] for n in names])
    sh = (C.c_int * max(len(shifts), 1))(*shifts)
    nbytes = mb.L.artemis_hip_pack_fields_level_bytes(C.byref(mb.pack), block0, len(shifts), len(names), sel, int(single), sh)
    esz = 4 if single else 8
    if expect:
        assert nbytes == 0
    out = torch.full((max(nbytes // esz, 4096),), float("nan"), dtype=torch.float32 if single else torch.float64, device=mb.dev)
    rc = mb.L.artemis_hip_pack_fields_level(C.byref(mb.pack), block0, len(shifts), len(names), sel, int(single), sh,
                                            C.c_void_p(out.data_ptr()), mb._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, mb.L.artemis_hip_last_error().decode())
    flat = out.cpu().numpy()
    if expect:
        return flat
    assert np.isnan(flat[nbytes // esz:]).all()  # nothing past the end
    ncomp = sum((3 if n.endswith(("velocity", "momentum")) else 1) * (mb.nsd if n.startswith("dust") else mb.nsg) for n in names)
    blocks, at = [], 0
    for s in shifts:
        shape = (ncomp,) + out_shape(mb.nx, s)
        blocks.append(flat[at:at + int(np.prod(shape))].reshape(shape))
        at += int(np.prod(shape))
    assert at * esz == nbytes
    return blocks


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name,shifts", CASES, ids=["%s%s" % (n, "".join("%+d" % s for s in sh)) for n, sh in CASES])
def test_pack_fields_level_equals_the_numpy_tree(hiplib, reference, name, shifts, single):
    mb, g, d = make_pack(name)
    want, vols = reference(name)
    names = GAS + (DUST if mb.nsd else [])
    order = [names[q] for q in np.random.default_rng(5).permutation(len(names))]
    for sel in (names, order[:5]):
        got = pack_fields_level(mb, sel, shifts, single=single)
        full = np.concatenate([want[v] for v in sel], axis=1)
        for b, s in enumerate(shifts):
            assert same_bits(got[b], resample(full[b], vols[b], s, single)), (name, b, s)
    if len(shifts) > 1:  # a sub-range that starts behind block 0
        got = pack_fields_level(mb, names, shifts[1:], block0=1, single=single)
        full = np.concatenate([want[v] for v in names], axis=1)
        for b, s in enumerate(shifts[1:]):
            assert same_bits(got[b], resample(full[1 + b], vols[1 + b], s, single)), (name, b, s)
    # nothing was written to the pack, and nothing was read from the pressure slot or from cons
    assert np.array_equal(mb.gas_prim.cpu().numpy(), g) and np.array_equal(mb.dust_prim.cpu().numpy(), d)
    assert (mb.gas_u0 == -555.0).all() and (mb.dust_u0 == -555.0).all()


def test_a_negative_zero_sum_becomes_positive_zero(hiplib):
    """2-D pack: the x3 pair adds the literal 0.0 of the inactive direction as the reference does, so a group whose
    velocities are -0.0 and 0 gives +0.0 -- and one of all -0.0 too, where a tree without that addition would keep -0.0."""
    import torch
    mb, g, d = make_pack("cart2d")
    g[0, 1, mb.ks, mb.js:mb.js + 2, mb.is_:mb.is_ + 2] = 0.0
    g[0, 1, mb.ks, mb.js, mb.is_] = -0.0
    g[0, 2, mb.ks, mb.js:mb.js + 2, mb.is_:mb.is_ + 2] = -0.0
    mb.gas_prim.copy_(torch.from_numpy(g))
    got = pack_fields_level(mb, ["gas.prim.velocity"], (1,))[0]
    xmin, xmax = block_bounds("cart2d")
    vol = oracle_volumes(mb.nx, xmin[0], xmax[0], 3, "cartesian")
    assert same_bits(got, resample(interior(mb, g)[0, 1:4], vol, 1))
    for comp in (0, 1):
        assert got[comp, 0, 0, 0] == 0.0 and not np.signbit(got[comp, 0, 0, 0])


@pytest.mark.parametrize("name", ["cart3d", "sph3d"])
def test_shift_one_is_the_reference_operator(hiplib, reference, name):
    """s = 1 against Oracle.RestrictAverage applied to a field that holds the full-resolution components: pins "shift 1 is
    the reference's operator" independently of the numpy tree."""
    from oracle.oracle import Oracle
    nb, nx, lo, hi, nsg, nsd, coords, ng = PACKS[name]
    mb, _, _ = make_pack(name)
    want, _ = reference(name)
    got = pack_fields_level(mb, GAS, (1,))[0]
    full = np.concatenate([want[v] for v in GAS], axis=1)[0]
    kw = dict(ng=ng, ns_gas=1, ns_dust=0, gamma=1.4, coordinates=coords)
    of, oc = Oracle(nx, lo, hi, **kw), Oracle(tuple(n // 2 for n in nx), lo, hi, **kw)
    I = lambda o: (slice(o.ks, o.ke + 1), slice(o.js, o.je + 1), slice(o.is_, o.ie + 1))
    rr = ((oc.is_, oc.ie, oc.js, oc.je, oc.ks, oc.ke), (oc.is_, oc.js, oc.ks), (of.is_, of.js, of.ks))
    for at in range(0, full.shape[0], 6):
        n = min(6, full.shape[0] - at)
        of.gprim[:] = 0.0
        of.gprim[(slice(0, n),) + I(of)] = full[at:at + n]
        of.RestrictAverage(oc, *rr)
        assert same_bits(got[at:at + n], np.ascontiguousarray(oc.gprim[(slice(0, n),) + I(oc)])), (name, at)


def test_impossible_requests_are_refused_and_write_nothing(hiplib):
    from artemis_amd import capi
    mb, _, _ = make_pack("three")
    for shifts in ((4, 0, 0), (0, -4, 0), (0, 0, 2)):  # |shift| = 4; nx2 = 6 is not divisible by 4
        flat = pack_fields_level(mb, GAS[:2], shifts, expect=capi.EINVAL)
        assert np.isnan(flat).all()
        msg = mb.L.artemis_hip_last_error().decode()
        assert "block %d" % [abs(s) > 1 for s in shifts].index(True) in msg and "shift %d" % [s for s in shifts if s][0] in msg
    assert "nx2 = 6 is not divisible by 4" in mb.L.artemis_hip_last_error().decode()
    assert np.isnan(pack_fields_level(mb, [], (1, 0, 0), expect=capi.EINVAL)).all()  # an empty selection


# ---- host driver ------------------------------------------------------------------------------------------------------
NAMES = ["gas.prim.density", "gas.prim.velocity", "gas.cons.density", "gas.cons.total_energy"]


def block_volumes(s, coordinates):
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    out = []
    for b in range(s.nblocks):
        bd = s.block_bounds(b)
        out.append(oracle_volumes(nx, bd[0::2], bd[1::2], s.is_ if nx[0] > 1 else 2, coordinates))
    return out


def test_refined_mesh_at_every_level(hiplib, tmp_path):
    """blast_amr.in at its test size (cylindrical, three levels): gather(level=L) equals, block by block, the numpy tree or
    replication of gather(); write_fields(level=L) reads back as one uniform array of the root grid's shape x 2^L, placed
    independently by bounds; the mass of the level-0 array is the history's."""
    from artemis_amd.driver import Simulation
    from artemis_amd.fields import read_fields
    case = amr_cases.blast_amr()
    s = Simulation(DECK(*case["deck"]), case["overrides"])
    s.evolve(3)
    levels = [s.block_level(b) for b in range(s.nblocks)]
    assert set(levels) == {0, 1, 2}
    full, vols = s.gather(NAMES), block_volumes(s, "cylindrical")
    clock = (s.time, s.dt, s.ncycle)
    for L in (0, 1, 2):
        got = s.gather(NAMES, level=L)
        want = [resample(full[b], vols[b], levels[b] - L) for b in range(s.nblocks)]
        assert len(got) == s.nblocks and all(same_bits(a, w) for a, w in zip(got, want)), L
        got32 = s.gather(NAMES, single=True, level=L)
        assert all(same_bits(a, w.astype(np.float32)) for a, w in zip(got32, want)), L
        s.write_fields(tmp_path / ("L%d.fld" % L), NAMES, level=L)
        fd = read_fields(tmp_path / ("L%d.fld" % L))
        assert fd.level == L and fd.version == 2
        at = 0
        for v in NAMES:
            u, n = fd.uniform(v), fd.variables[v]
            assert u.shape == (n, 1, 128 << L, 128 << L)
            assert same_bits(u, place(fd.blocks, [w[at:at + n] for w in want]))
            at += n
        if L == 0:
            u0 = fd.uniform("gas.cons.density")[0, 0]
    assert (s.time, s.dt, s.ncycle) == clock
    # Conservation.  A zone of the level-0 array holds N / Vs: N the sum of rho V over the zones of the mesh under it, Vs
    # the sum of their V.  The history sums the same terms rho V in another order: 2 gamma_n sum|terms| (n the zones of the
    # mesh), the bound tests/test_outputs.py uses for the history sums.  This test multiplies by its own closed-form volume
    # V0 = 0.5 (r0 + r1) dr dphi dz of the level-0 zone instead of Vs, so V0 / Vs - 1 is added.  Both are products of face
    # differences, and a face r0 + i dr (device) or linspace (here) is within 2 u max|r| = 10 u of the exact one, so a
    # difference of width w is off by at most 20 u / w relative: 20 u / (4 / 512) = 2560 u on the finest level, 640 u for
    # V0; along phi (faces <= pi / 2) 4 u (pi / 2) / w = 2048 u and 512 u; the remaining products, the additions of Vs and
    # the division and product around them are below 40 u.  Sum: 5800 u, counted as 6000 u.
    r = np.linspace(1.0, 5.0, 129)
    phi = np.linspace(0.0, 1.570796326794897, 129)
    v0 = (0.5 * (r[:-1] + r[1:]) * np.diff(r))[None, :] * np.diff(phi)[:, None] * 1.0
    mass = s.history_device()[0]
    n_fine = 64 * s.nblocks
    bound = (2 * gamma(n_fine - 1) + 6000 * 2.0 ** -53) * np.sum(np.abs(u0 * v0))
    print("mass of the level-0 array %.17g, history %.17g, difference %.3e, bound %.3e" % (np.sum(u0 * v0), mass, abs(np.sum(u0 * v0) - mass), bound))
    assert abs(np.sum(u0 * v0) - mass) <= bound
    s.close()


def test_coarser_than_the_root_grid_and_the_run_is_not_disturbed(hiplib):
    """32^3 blast in eight 16^3 blocks on the tuned kernel: level -1 and -2 equal the numpy tree of the full uniform array; a
    run that gathers at a level after every cycle -- also across a 1 MiB staging buffer, whose ranges are cut by bytes --
    takes the steps of one that never does."""
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    ov = BLAST32 + ["parthenon/time/nlim=4"]
    a, b = Simulation(DECK("blast", "blast.in"), ov), Simulation(DECK("blast", "blast.in"), ov)
    assert a.uses_tuned_kernel and a.nblocks == 8
    names = NAMES + ["gas.prim.pressure", "gas.cons.momentum"]  # 10 components: a block of 8^3 at level -1 is 40 KiB, all 8 fit;
    for cycle in range(4):                                        # at level 1 a block of 32^3 is 2.5 MiB: one block a range
        assert a.evolve(1) == 1 and b.evolve(1) == 1
        got = a.gather(names, level=-1)
        with capi.option("fields_stage_mb", 1):
            assert all(same_bits(x, y) for x, y in zip(a.gather(names, level=-1), got))
            fine = a.gather(names, level=1)
            same_level = a.gather(names, level=0)  # blocks of 320 KiB: ranges of 3, 3 and 2 blocks
        assert all(x.shape == (10, 32, 32, 32) for x in fine) and same_bits(np.stack(same_level), a.gather(names))
    full, vols = a.gather(names), block_volumes(a, "cartesian")
    blocks = [dict(bounds=a.block_bounds(q)) for q in range(8)]
    whole, vol = place(blocks, list(full)), place(blocks, [v[None] for v in vols])[0]
    assert whole.shape == (10, 32, 32, 32) and not np.isnan(whole).any()
    for L in (-1, -2):
        got = place(blocks, a.gather(names, level=L))
        assert same_bits(got, resample(whole, vol, -L)), L
    assert all(same_bits(x, np.repeat(np.repeat(np.repeat(y, 2, 1), 2, 2), 2, 3)) for x, y in zip(fine, full))
    (ca, fa), (cb, fb) = state_of(a), state_of(b)
    assert ca == cb and ca[2] == 4 and ca[3] == "stage_fused_kernel"
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y)
    a.close(), b.close()


def test_deck_block_with_a_level_and_the_refusals(hiplib, tmp_path):
    """A `fld` block with level = -1 beside one without: the plain block's dumps are byte-identical to those of the same run
    without the levelled block, the levelled ones are version 2 and hold the numpy tree of the plain ones.  load_fields
    refuses a levelled dump and leaves the run alone; a level that can need shift 4 is listed as skipped and writes nothing."""
    from artemis_amd.driver import Simulation
    from artemis_amd.fields import read_fields
    ov = BLAST32 + ["parthenon/time/nlim=4"]
    v = ", ".join(NAMES)
    plain = ["parthenon/output1/file_type=fld", "parthenon/output1/dt=0.005", "parthenon/output1/variables=" + v]
    lev = ["parthenon/output2/file_type=fld", "parthenon/output2/dt=0.005", "parthenon/output2/variables=" + v, "parthenon/output2/level=-1",
           "parthenon/output3/file_type=fld", "parthenon/output3/dt=0.005", "parthenon/output3/variables=" + v, "parthenon/output3/level=4"]
    a, b = Simulation(DECK("blast", "blast.in"), ov + plain + lev), Simulation(DECK("blast", "blast.in"), ov + plain)
    a.enable_outputs(tmp_path / "a"), b.enable_outputs(tmp_path / "b")
    a.evolve(), b.evolve()
    st = {q["index"]: q for q in a.outputs()["blocks"]}
    assert st[3]["status"] == "skipped: level 4: a block on level 0 would need shift -4, |shift| <= 3 is built"
    assert st[2]["status"] == "active" and st[2]["level"] == -1 and not [f for f in os.listdir(tmp_path / "a") if ".out3." in f]
    ones = sorted(os.listdir(tmp_path / "b"))
    assert ones == sorted(f for f in os.listdir(tmp_path / "a") if ".out1." in f) and len(ones) >= 2
    vols = block_volumes(a, "cartesian")
    for f in ones:
        for part in ("meta.json", "rank0.bin"):
            assert open(tmp_path / "a" / f / part, "rb").read() == open(tmp_path / "b" / f / part, "rb").read(), (f, part)
        fd, lv = read_fields(tmp_path / "a" / f), read_fields(tmp_path / "a" / f.replace(".out1.", ".out2."))
        assert json.load(open(tmp_path / "a" / f / "meta.json"))["version"] == 1 and lv.version == 2 and lv.level == -1
        for name in NAMES:
            for q, (got, full) in enumerate(zip(lv.get_blocks(name), fd.get(name))):
                assert same_bits(got, resample(full, vols[q], 1)), (f, name, q)
            assert lv.uniform(name).shape[1:] == (16, 16, 16)
    before = state_of(a)
    with pytest.raises(ValueError, match="resampled to level -1: not a state"):
        a.load_fields(tmp_path / "a" / "blast_cart.out2.final.fld")
    after = state_of(a)
    assert before[0] == after[0] and all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    with pytest.raises(RuntimeError, match="local block 0 .* on level 0 would need shift 4"):
        a.gather(NAMES, level=-4)
    a.close(), b.close()
