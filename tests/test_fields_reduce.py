"""GPU tests of reduced field outputs: artemis_hip_reduce_fields (kernels_reduce.hip) on packs, Simulation.gather /
write_fields with reduce=... and a deck's `reduce = x2,x3` on the host driver.

The definition (include/artemis_hip.h) is emulated in numpy (tests/fields_reduce_ref.py): the full-resolution components are
what artemis_hip_prim_to_cons leaves in a copy of the pack, as in tests/test_fields.py; the volumes are the CPU oracle's.
Every comparison of values is bitwise, -0.0 included.  Every zone of a pack is random, ghost zones included, the floors
bind, the pressure slot and cons are poisoned.  The shapes are the smallest at which the chunks of 64, their tail, their
alignment to the interior start, the walks along x2 / x3 and the passes over the work buffer can go wrong."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from fields_reduce_ref import assemble, names_of, oracle_volumes, out_shape, reduce_block, same_bits, subsets
from test_fields import BLAST32, DFLOOR, DUST, DUST_DFLOOR, GAS, SIEFLOOR, interior
from test_fields_level import full_components
from test_outputs import SUM_CASES, gamma, state_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)

# name: (nblocks, nx, lo, hi, ns_gas, ns_dust, coordinates, ng)
PACKS = {
    "x64": (1, (64, 6, 3), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 0, "cartesian", 2),      # one exact chunk
    "cart3d": (1, (72, 12, 4), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 2, "cartesian", 2),  # a chunk and a tail of 8
    "cart2d": (1, (40, 24, 1), (-1, -0.5, -0.5), (1, 0.8, 0.5), 1, 0, "cartesian", 3),   # a short chunk only, odd interior start
    "cart1d": (1, (136, 1, 1), (0, -0.5, -0.5), (1, 0.5, 0.5), 2, 0, "cartesian", 2),    # two chunks and a tail, two species
    "cyl3d": (1, (16, 8, 6), (0.5, 0.0, -1.0), (2.0, 6.0, 1.0), 1, 1, "cylindrical", 2),
    "sph3d": (1, (16, 8, 6), (0.3, 0.7, 0.0), (1.7, 2.5, 6.0), 1, 0, "spherical", 2),
    "three": (3, (24, 6, 4), (-1, -0.5, 0.25), (2, 0.8, 0.95), 1, 1, "cartesian", 2),
}
CASES = [(name, axes) for name in PACKS for axes in subsets(PACKS[name][1])]


def block_bounds(name):
    nb, nx, lo, hi = PACKS[name][:4]
    edges = np.linspace(lo[0], hi[0], nb + 1)  # the blocks side by side along x1
    return [[edges[b], lo[1], lo[2]] for b in range(nb)], [[edges[b + 1], hi[1], hi[2]] for b in range(nb)]


def make_pack(name, seed=11):
    """(pack, host copies of its primitive arrays): random primitives in every zone, floors that bind, the pressure slot
    and cons poisoned -- as tests/test_fields_level.py builds its packs"""
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


def ncomp_of(mb, names):
    return sum((3 if n.endswith(("velocity", "momentum")) else 1) * (mb.nsd if n.startswith("dust") else mb.nsg) for n in names)


def reduce_fields(mb, names, axes, block0=0, nblocks=None, single=False, expect=0, codes=None):
    """artemis_hip_reduce_fields of blocks [block0, block0 + nblocks) as [nblocks, ncomp + 1, nz', ny', nx']; with expect != 0
    the NaN-filled buffers (out, work) as the call left them"""
    import torch
    from artemis_amd import capi
    nblocks = mb.nb if nblocks is None else nblocks
    codes = [capi.FIELD_VAR[n] for n in names] if codes is None else codes
    sel = (C.c_int * max(len(codes), 1))(*codes)
    args = (C.byref(mb.pack), block0, nblocks, len(codes), sel, int(single), axes)
    nbytes, wbytes = mb.L.artemis_hip_reduce_fields_bytes(*args), mb.L.artemis_hip_reduce_fields_work_bytes(*args)
    esz = 4 if single else 8
    if expect:
        assert nbytes == 0 and wbytes == 0
    out = torch.full((nbytes // esz + 4096,), float("nan"), dtype=torch.float32 if single else torch.float64, device=mb.dev)
    work = torch.full((wbytes // 8 + 4096,), float("nan"), dtype=torch.float64, device=mb.dev)
    rc = mb.L.artemis_hip_reduce_fields(*args, C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), mb._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, mb.L.artemis_hip_last_error().decode())
    flat, wflat = out.cpu().numpy(), work.cpu().numpy()
    if expect:
        return flat, wflat
    assert np.isnan(flat[nbytes // esz:]).all() and np.isnan(wflat[wbytes // 8:]).all()  # the untouched tails stay NaN
    assert not np.isnan(flat[:nbytes // esz]).any()
    shape = (nblocks, ncomp_of(mb, names) + 1) + out_shape(mb.nx, axes)
    assert int(np.prod(shape)) * esz == nbytes
    return flat[:nbytes // esz].reshape(shape)


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name,axes", CASES, ids=["%s-%s" % (n, "".join(names_of(a))) for n, a in CASES])
def test_reduce_fields_equals_the_numpy_emulation(hiplib, reference, name, axes, single):
    mb, g, d = make_pack(name)
    want, vols = reference(name)
    names = GAS + (DUST if mb.nsd else [])
    order = [names[q] for q in np.random.default_rng(5).permutation(len(names))]
    for sel in (names, order[:5]):
        got = reduce_fields(mb, sel, axes, single=single)
        full = np.concatenate([want[v] for v in sel], axis=1)
        for b in range(mb.nb):
            assert same_bits(got[b], reduce_block(full[b], vols[b], axes, single)), (name, axes, b)
    if mb.nb > 1:  # a sub-range that starts behind block 0
        got = reduce_fields(mb, names, axes, block0=1, nblocks=2, single=single)
        full = np.concatenate([want[v] for v in names], axis=1)
        for b in range(2):
            assert same_bits(got[b], reduce_block(full[1 + b], vols[1 + b], axes, single)), (name, axes, b)
    # nothing was written to the pack, and nothing was read from the pressure slot or from cons
    assert np.array_equal(mb.gas_prim.cpu().numpy(), g) and np.array_equal(mb.dust_prim.cpu().numpy(), d)
    assert (mb.gas_u0 == -555.0).all() and (mb.dust_u0 == -555.0).all()


@pytest.mark.parametrize("name", ["x64", "cart3d"])
def test_signed_zeros(hiplib, reference, name):
    """Velocities -0.0 everywhere: N = V * -0.0 = -0.0 in every zone.  The x1 butterfly of one exact chunk (nx1 = 64) adds only
    -0.0 and keeps it; at nx1 = 72 the tail is padded with the literal +0.0 and the sum is +0.0.  The x2 and x3 chains start
    from their first element and keep -0.0."""
    import torch
    mb, g, d = make_pack(name)
    g[:, 1:4] = -0.0
    mb.gas_prim.copy_(torch.from_numpy(g))
    _, vols = reference(name)
    full = interior(mb, g)[0, 1:4]
    for axes in subsets(mb.nx):
        got = reduce_fields(mb, ["gas.prim.velocity"], axes)[0]
        assert same_bits(got, reduce_block(full, vols[0], axes))
        assert (got[:3] == 0.0).all()
        negative = not (axes & 1) or mb.nx[0] == 64
        assert np.signbit(got[:3]).all() if negative else not np.signbit(got[:3]).any(), (name, axes)


def test_refusals_return_einval_and_write_nothing(hiplib):
    from artemis_amd import capi
    mb, _, _ = make_pack("three")       # (24, 6, 4), gas and dust
    flat2d, _, _ = make_pack("cart2d")  # nx3 = 1, no dust
    refused = [
        (mb, GAS[:2], 0, {}, "axes = 0"),                                   # no direction
        (mb, GAS[:2], 8, {}, "axes = 8"),
        (flat2d, GAS[:2], 4, {}, "x3 has one zone"),                        # an inactive direction
        (flat2d, GAS[:2], 7, {}, "x3 has one zone"),
        (mb, [], 1, {}, "no variables"),
        (mb, GAS[:2], 1, dict(codes=[0, 12]), "unknown variable code"),     # whatever pack_fields refuses
        (flat2d, DUST[:1], 1, {}, "without dust"),
        (mb, GAS[:2], 1, dict(block0=2, nblocks=2), "not inside the pack"),
        (mb, GAS[:2], 1, dict(nblocks=-1), "not inside the pack"),
    ]
    for pack, names, axes, kw, text in refused:
        flat, wflat = reduce_fields(pack, names, axes, expect=capi.EINVAL, **kw)
        assert np.isnan(flat).all() and np.isnan(wflat).all(), text
        assert text in pack.L.artemis_hip_last_error().decode(), (text, pack.L.artemis_hip_last_error().decode())


# ---- host driver ------------------------------------------------------------------------------------------------------
NAMES = ["gas.prim.density", "gas.prim.velocity", "gas.cons.density", "gas.cons.total_energy"]
DISK_CYL = SUM_CASES["disk_cyl"]
DISK_CYL_4 = (DISK_CYL[0], [o for o in DISK_CYL[1] if "meshblock" not in o] +
              ["parthenon/meshblock/nx1=8", "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=3"])
RUNS = {  # deck, overrides, coordinates, blocks
    "disk_cyl-1": DISK_CYL + ("cylindrical", 1),
    "disk_cyl-4": DISK_CYL_4 + ("cylindrical", 4),
    "blast-1": (("blast", "blast.in"), [o for o in BLAST32 if "meshblock" not in o] +
                ["parthenon/meshblock/nx1=32", "parthenon/meshblock/nx2=32", "parthenon/meshblock/nx3=32", "parthenon/time/nlim=3"],
                "cartesian", 1),
    "blast-8": (("blast", "blast.in"), BLAST32 + ["parthenon/time/nlim=3"], "cartesian", 8),
}


def block_volumes(s, coordinates):
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    out = []
    for b in range(s.nblocks):
        bd = s.block_bounds(b)
        out.append(oracle_volumes(nx, bd[0::2], bd[1::2], s.is_ if nx[0] > 1 else 2, coordinates))
    return out


@pytest.mark.parametrize("run", list(RUNS))
def test_gather_reduced_equals_the_emulation_of_gather(hiplib, tmp_path, run):
    """gather(reduce=...) equals, block by block, the emulation applied to gather() of the same run; the dump reads back and
    reduced() equals the independent assembly; the run is not disturbed; the fully reduced gas.cons.density is the history's
    mass within 2 gamma_{n-1} S (the same terms rho V, only the order of the additions differs)."""
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    from artemis_amd.fields import read_fields
    deck, ov, coordinates, nblocks = RUNS[run]
    s = Simulation(DECK(*deck), ov)
    s.evolve(3)
    assert s.nblocks == nblocks
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    full, vols = s.gather(NAMES), block_volumes(s, coordinates)
    before = state_of(s)
    blocks = [dict(bounds=s.block_bounds(b)) for b in range(s.nblocks)]
    for axes in (4, 6, 7, 1, 2):
        red = names_of(axes)
        want = np.stack([reduce_block(full[b], vols[b], axes) for b in range(s.nblocks)])
        got = s.gather(NAMES, reduce=red)
        assert same_bits(got, want), (run, red)
        assert same_bits(s.gather(NAMES, single=True, reduce=",".join(red)), want.astype(np.float32)), (run, red)
        with capi.option("fields_stage_mb", 1):
            assert same_bits(s.gather(NAMES, reduce=red), want), (run, red)
        if axes in (6, 7):
            s.write_fields(tmp_path / "r.fld", NAMES, reduce=red)
            fd = read_fields(tmp_path / "r.fld")
            assert fd.version == 3 and fd.reduce == list(red) and fd.level is None and list(fd.variables)[-1] == "volume"
            N, W = assemble(blocks, list(want[:, :-1]), list(want[:, -1:]), axes, nx)
            at = 0
            for v in NAMES:
                n = fd.variables[v]
                assert same_bits(np.stack(fd.get_blocks(v)), want[:, at:at + n])
                assert same_bits(fd.reduced(v, "integral"), N[at:at + n]) and same_bits(fd.reduced(v), N[at:at + n] / W)
                at += n
            assert same_bits(fd.reduced("volume"), W)
    if run == "blast-8":
        # 32 x 3 + 1 components of 16 x 16 are 194 KiB a block, of output and (x2, x3) of work alike: a 1 MiB staging buffer
        # takes the eight blocks as a range of five and one of three
        vel = s.gather(["gas.prim.velocity"])
        for axes in (4, 6):
            want = np.stack([reduce_block(np.tile(vel[b], (32, 1, 1, 1)), vols[b], axes) for b in range(8)])
            with capi.option("fields_stage_mb", 1):
                assert same_bits(s.gather(["gas.prim.velocity"] * 32, reduce=names_of(axes)), want), axes
    after = state_of(s)
    assert before[0] == after[0] and all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    total = fd.reduced("gas.cons.density", "integral")  # (the last dump: every direction reduced)
    assert total.shape == (1, 1, 1, 1)
    mass = s.history()[0]
    bound = 2.0 * gamma(s.total_zones - 1) * abs(mass)  # S of a sum of positive terms is the sum
    print(run, "mass of the reduced dump %.17g, history %.17g, difference %.3e, bound %.3e" % (total[0, 0, 0, 0], mass, abs(total[0, 0, 0, 0] - mass), bound))
    assert abs(total[0, 0, 0, 0] - mass) <= bound
    with pytest.raises(ValueError, match="reduce together with level"):
        s.gather(NAMES, level=0, reduce=("x1",))
    with pytest.raises(ValueError, match="reduce takes x1, x2"):
        s.gather(NAMES, reduce=("x4",))
    s.close()


def test_deck_block_with_reduce_and_the_refusals(hiplib, tmp_path):
    """A `fld` block with reduce = x2,x3 beside a plain one, on schedule: the reduced dumps are version 3 and hold the emulation
    of the plain ones; the plain block's dumps and the run's clock and fields are those of the same run without the reduced
    block; a block that names an inactive direction, or that also sets level, is listed as skipped; load_fields refuses a
    reduced dump and leaves the run alone."""
    from artemis_amd.driver import Simulation
    from artemis_amd.fields import read_fields
    deck, ov = DISK_CYL_4
    v = ", ".join(NAMES)
    blk = lambda n, *extra: ["parthenon/output%d/file_type=fld" % n, "parthenon/output%d/dt=0.002" % n,
                             "parthenon/output%d/variables=%s" % (n, v)] + ["parthenon/output%d/%s" % (n, e) for e in extra]
    plain = blk(1)
    more = blk(2, "reduce=x2,x3") + blk(3, "reduce=x1", "level=0") + blk(4, "reduce=x5") + blk(5, "reduce= x3 , x1", "single_precision_output=true")
    a, b = Simulation(DECK(*deck), ov + plain + more), Simulation(DECK(*deck), ov + plain)
    a.enable_outputs(tmp_path / "a"), b.enable_outputs(tmp_path / "b")
    a.evolve(), b.evolve()
    st = {q["index"]: q for q in a.outputs()["blocks"]}
    assert st[2]["status"] == "active" and st[2]["reduce"] == ["x2", "x3"] and st[5]["reduce"] == ["x1", "x3"]
    assert st[3]["status"] == "skipped: reduce: a block that also sets level is not built"
    assert st[4]["status"] == "skipped: reduce: unknown direction x5 (x1, x2, x3)"
    assert not [f for f in os.listdir(tmp_path / "a") if ".out3." in f or ".out4." in f]
    (ca, fa), (cb, fb) = state_of(a), state_of(b)
    assert ca == cb and all(np.array_equal(x, y) for x, y in zip(fa, fb))
    ones = sorted(os.listdir(tmp_path / "b"))
    assert ones == sorted(f for f in os.listdir(tmp_path / "a") if ".out1." in f) and len(ones) >= 2
    vols = block_volumes(a, "cylindrical")
    nx = (a.ie - a.is_ + 1, a.je - a.js + 1, a.ke - a.ks + 1)
    for f in ones:
        for part in ("meta.json", "rank0.bin"):
            assert open(tmp_path / "a" / f / part, "rb").read() == open(tmp_path / "b" / f / part, "rb").read(), (f, part)
        fd = read_fields(tmp_path / "a" / f)
        assert json.load(open(tmp_path / "a" / f / "meta.json"))["version"] == 1 and fd.reduce is None
        for n, axes, single in ((2, 6, False), (5, 5, True)):
            rd = read_fields(tmp_path / "a" / f.replace(".out1.", ".out%d." % n))
            meta = json.load(open(tmp_path / "a" / f.replace(".out1.", ".out%d." % n) / "meta.json"))
            assert meta["version"] == 3 and meta["reduce"] == list(names_of(axes)) and meta["variables"][-1]["name"] == "volume"
            assert all(q["nx"] == list(out_shape(nx, axes))[::-1] for q in meta["blocks"])
            assert [q["offset"] for q in meta["blocks"]] == [g * 7 * int(np.prod(out_shape(nx, axes))) for g in range(4)]
            full = np.concatenate([fd.get(name) for name in NAMES], axis=1)
            want = np.stack([reduce_block(full[g], vols[g], axes, single) for g in range(4)])
            got = np.concatenate([np.stack(rd.get_blocks(name)) for name in NAMES + ["volume"]], axis=1)
            assert same_bits(got, want), (f, n)
            N, W = assemble(rd.blocks, list(want[:, :-1]), list(want[:, -1:]), axes, nx)
            assert same_bits(rd.reduced("gas.prim.density"), N[:1] / W)
    before = state_of(a)
    with pytest.raises(ValueError, match="was reduced along x2, x3: not a state"):
        a.load_fields(tmp_path / "a" / ones[-1].replace(".out1.", ".out2."))
    after = state_of(a)
    assert before[0] == after[0] and all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    # an inactive direction: the 2-D refined blast of tests/test_outputs.py has one zone along x3
    deck2, ov2 = SUM_CASES["refined"]
    c = Simulation(DECK(*deck2), list(ov2) + blk(1, "reduce=x1,x3") + blk(2, "reduce=x1,x2"))
    st = {q["index"]: q for q in c.outputs()["blocks"]}
    assert st[1]["status"] == "skipped: reduce: x3 has one zone and is not a direction to reduce" and st[2]["status"].startswith("inactive")
    with pytest.raises(RuntimeError, match="x3 has one zone"):
        c.gather(NAMES, reduce=("x3",))
    # a refined mesh: only the fully reduced dump is assembled
    c.write_fields(tmp_path / "c12.fld", NAMES, reduce=("x1", "x2"))
    c.write_fields(tmp_path / "c1.fld", NAMES, reduce=("x1",))
    assert read_fields(tmp_path / "c12.fld").reduced("gas.cons.density", "integral").shape == (1, 1, 1, 1)
    with pytest.raises(ValueError, match="do not share a zone size"):
        read_fields(tmp_path / "c1.fld").reduced("gas.cons.density")
    a.close(), b.close(), c.close()
