"""GPU tests of reduced field outputs on a chosen level: artemis_hip_reduce_fields_level (kernels_reduce.hip,
resample_reduced_kernel behind the unchanged reduce passes) on packs, Simulation.gather / write_fields with reduce=... and
reduce_level=L and a deck's `reduce_level = L` on the host driver.

The definition (include/artemis_hip.h) is emulated in numpy (tests/fields_reduce_level_ref.py on top of
tests/fields_reduce_ref.py): the full-resolution components are what artemis_hip_prim_to_cons leaves in a copy of the pack,
the volumes are the CPU oracle's.  Every comparison of values is bitwise, -0.0 included.  Every zone of a pack is random,
ghost zones included, the floors bind, the pressure slot and cons are poisoned.  The shapes are the smallest at which the
pair trees, the shares, a ragged last tile, blocks of different shift in one launch and the inactive directions can go
wrong."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import amr_cases
import test_multilevel
from fields_reduce_level_ref import allowed_levels, kept_directions, out_shape_level, place_sum, reduce_block_level, resample_reduced
from fields_reduce_ref import names_of, oracle_volumes, reduce_block, same_bits, subsets
from test_fields import BLAST32, DFLOOR, DUST, DUST_DFLOOR, GAS, SIEFLOOR, interior
from test_fields_level import full_components
from test_outputs import gamma, state_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)

ALL = (-3, -2, -1, 0, 1, 2, 3)
# name: (nblocks, nx, lo, hi, ns_gas, ns_dust, coordinates, ng, the shift of every block)
PACKS = {
    "cart3d": (7, (8, 8, 8), (-1, -0.5, 0.25), (2.5, 0.8, 0.95), 1, 1, "cartesian", 2, ALL),     # every shift in one launch
    "cyl3d": (7, (8, 8, 8), (0.5, 0.0, -1.0), (4.0, 6.0, 1.0), 1, 0, "cylindrical", 2, ALL[::-1]),
    "sph3d": (7, (8, 8, 8), (0.3, 0.7, 0.0), (3.8, 2.5, 6.0), 1, 0, "spherical", 2, (0, 3, -3, 1, -1, 2, -2)),
    "cart2d": (7, (8, 8, 1), (-1, -0.5, -0.5), (2.5, 0.8, 0.5), 1, 0, "cartesian", 3, ALL),      # x3 inactive, odd interior start
    "cart1d": (7, (8, 1, 1), (0, -0.5, -0.5), (7, 0.5, 0.5), 2, 0, "cartesian", 2, ALL),         # only x1 active: m = 0
    "long": (1, (40, 8, 8), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 0, "cartesian", 2, (-2,)),      # 160 output zones along x1
    "fine": (1, (8, 8, 8), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 1, "cartesian", 2, (3,)),        # kept extents collapse to 1
    "many": (200, (8, 8, 1), (-1, -0.5, -0.5), (99, 0.8, 0.5), 1, 0, "cartesian", 2, tuple(ALL[b % 7] for b in range(200))),  # two launches
}
CASES = [(name, axes) for name in PACKS for axes in subsets(PACKS[name][1]) if name != "many" or axes == 1]


def block_bounds(name):
    nb, nx, lo, hi = PACKS[name][:4]
    edges = np.linspace(lo[0], hi[0], nb + 1)  # the blocks side by side along x1
    return [[edges[b], lo[1], lo[2]] for b in range(nb)], [[edges[b + 1], hi[1], hi[2]] for b in range(nb)]


def make_pack(name, seed=11):
    """(pack, host copies of its primitive arrays): random primitives in every zone, floors that bind, the pressure slot
    and cons poisoned -- as tests/test_fields_reduce.py builds its packs"""
    import torch
    from artemis_amd.pack import MeshBlockPack
    nb, nx, lo, hi, nsg, nsd, coords, ng = PACKS[name][:8]
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
            nb, nx, lo, hi, nsg, nsd, coords, ng = PACKS[name][:8]
            xmin, xmax = block_bounds(name)
            cache[name] = (full_components(make_pack(name)[0]), [oracle_volumes(nx, xmin[b], xmax[b], ng, coords) for b in range(nb)])
        return cache[name]
    return get


def ncomp_of(mb, names):
    return sum((3 if n.endswith(("velocity", "momentum")) else 1) * (mb.nsd if n.startswith("dust") else mb.nsg) for n in names)


def reduce_fields_level(mb, names, axes, shifts, block0=0, single=False, expect=0, codes=None, nblocks=None):
    """artemis_hip_reduce_fields_level of blocks [block0, block0 + len(shifts)) as a list of [ncomp + 1, nz', ny', nx'] arrays;
    with expect != 0 the NaN-filled buffers (out, work) as the call left them"""
    import torch
    from artemis_amd import capi
    nblocks = len(shifts) if nblocks is None else nblocks
    codes = [capi.FIELD_VAR[n] for n in names] if codes is None else codes
    sel = (C.c_int * max(len(codes), 1))(*codes)
    sh = (C.c_int * max(len(shifts), 1))(*shifts)
    args = (C.byref(mb.pack), block0, nblocks, len(codes), sel, int(single), axes, sh)
    nbytes, wbytes = mb.L.artemis_hip_reduce_fields_level_bytes(*args), mb.L.artemis_hip_reduce_fields_level_work_bytes(*args)
    esz = 4 if single else 8
    if expect:
        assert nbytes == 0 and wbytes == 0
    out = torch.full((nbytes // esz + 4096,), float("nan"), dtype=torch.float32 if single else torch.float64, device=mb.dev)
    work = torch.full((wbytes // 8 + 4096,), float("nan"), dtype=torch.float64, device=mb.dev)
    rc = mb.L.artemis_hip_reduce_fields_level(*args, C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), mb._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, mb.L.artemis_hip_last_error().decode())
    flat, wflat = out.cpu().numpy(), work.cpu().numpy()
    if expect:
        return flat, wflat
    assert np.isnan(flat[nbytes // esz:]).all() and np.isnan(wflat[wbytes // 8:]).all()  # the untouched tails stay NaN
    assert not np.isnan(flat[:nbytes // esz]).any()
    blocks, at = [], 0
    for s in shifts:
        shape = (ncomp_of(mb, names) + 1,) + out_shape_level(mb.nx, axes, s)
        blocks.append(flat[at:at + int(np.prod(shape))].reshape(shape))
        at += int(np.prod(shape))
    assert at * esz == nbytes
    return blocks


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name,axes", CASES, ids=["%s-%s" % (n, "".join(names_of(a))) for n, a in CASES])
def test_reduce_fields_level_equals_the_numpy_emulation(hiplib, reference, name, axes, single):
    from artemis_amd import capi
    mb, g, d = make_pack(name)
    want, vols = reference(name)
    shifts = PACKS[name][8]
    names = GAS + (DUST if mb.nsd else [])
    order = [names[q] for q in np.random.default_rng(5).permutation(len(names))]
    for sel in (names, order[:5]):
        got = reduce_fields_level(mb, sel, axes, shifts, single=single)
        full = np.concatenate([want[v] for v in sel], axis=1)
        expected = [reduce_block_level(full[b], vols[b], axes, shifts[b], single) for b in range(mb.nb)]
        for b in range(mb.nb):
            assert same_bits(got[b], expected[b]), (name, axes, b, shifts[b])
    if mb.nb > 1:
        # a sub-range that starts behind block 0, and launches whose workgroups take many trips of the stride loop
        sub = reduce_fields_level(mb, sel, axes, shifts[2:6], block0=2, single=single)
        assert all(same_bits(x, y) for x, y in zip(sub, expected[2:6])), (name, axes)
        for cap in (1, 3):
            with capi.option("grid_cap", cap):
                cut = reduce_fields_level(mb, sel, axes, shifts, single=single)
            assert all(same_bits(x, y) for x, y in zip(cut, expected)), (name, axes, cap)
        # every shift 0: artemis_hip_reduce_fields bit for bit
        zero = reduce_fields_level(mb, sel, axes, (0,) * mb.nb, single=single)
        assert all(same_bits(zero[b], reduce_block(full[b], vols[b], axes, single)) for b in range(mb.nb)), (name, axes)
    # nothing was written to the pack, and nothing was read from the pressure slot or from cons
    assert np.array_equal(mb.gas_prim.cpu().numpy(), g) and np.array_equal(mb.dust_prim.cpu().numpy(), d)
    assert (mb.gas_u0 == -555.0).all() and (mb.dust_u0 == -555.0).all()


def test_signed_zeros(hiplib, reference):
    """Velocities -0.0 everywhere: N = V * -0.0 = -0.0 in every zone, and the x2 / x3 chains keep it.  A block one level finer
    adds (-0.0) + (-0.0) = -0.0, a block one level coarser multiplies -0.0 by a power of two: a row of -0.0 stays -0.0.  (With x1
    reduced the butterfly of a chunk of 8 is padded with +0.0 and the sums are +0.0, as artemis_hip_reduce_fields defines.)"""
    import torch
    mb, g, d = make_pack("cart3d")
    g[:, 1:4] = -0.0
    mb.gas_prim.copy_(torch.from_numpy(g))
    _, vols = reference("cart3d")
    full = interior(mb, g)[:, 1:4]
    shifts = (-1, 1, -1, 1, 0, 2, -2)
    for axes in subsets(mb.nx):
        got = reduce_fields_level(mb, ["gas.prim.velocity"], axes, shifts)
        for b, s in enumerate(shifts):
            assert same_bits(got[b], reduce_block_level(full[b], vols[b], axes, s)), (axes, b)
            assert (got[b][:3] == 0.0).all()
            assert np.signbit(got[b][:3]).all() if not axes & 1 else not np.signbit(got[b][:3]).any(), (axes, b)


def test_refusals_return_einval_and_write_nothing(hiplib):
    from artemis_amd import capi
    from test_fields_reduce import make_pack as reduce_pack
    mb, _, _ = reduce_pack("three")       # (24, 6, 4), gas and dust, three blocks
    flat2d, _, _ = reduce_pack("cart2d")  # (40, 24, 1), no dust
    refused = [
        (mb, GAS[:2], 1, (0, 4, 0), {}, "block 1 has shift 4, |shift| <= 3 is built"),
        (mb, GAS[:2], 1, (0, 0, -4), {}, "block 2 has shift -4, |shift| <= 3 is built"),
        (mb, GAS[:2], 1, (0, 2, 0), {}, "block 1 has shift 2, and its kept nx2 = 6 is not divisible by 4"),  # x1 reduced: 6 and 4 kept
        (mb, GAS[:2], 2, (3, 0, 0), {}, "block 0 has shift 3, and its kept nx3 = 4 is not divisible by 8"),  # 24 is
        (mb, GAS[:2], 6, (0, 1), dict(block0=1), None),                        # (taken: only the kept extent 24 counts)
        (mb, GAS[:2], 6, (3, 3, 3), {}, None),
        (mb, GAS[:2], 0, (0, 0, 0), {}, "axes = 0"),                           # whatever artemis_hip_reduce_fields refuses
        (mb, GAS[:2], 8, (0, 0, 0), {}, "axes = 8"),
        (flat2d, GAS[:2], 4, (0,), {}, "x3 has one zone"),
        (mb, [], 1, (0, 0, 0), {}, "no variables"),
        (mb, GAS[:2], 1, (0, 0, 0), dict(codes=[0, 12]), "unknown variable code"),
        (flat2d, DUST[:1], 1, (0,), {}, "without dust"),
        (mb, GAS[:2], 1, (0, 0), dict(block0=2), "not inside the pack"),
        (mb, GAS[:2], 1, (0,), dict(nblocks=-1), "not inside the pack"),
    ]
    for pack, names, axes, shifts, kw, text in refused:
        if text is None:
            assert len(reduce_fields_level(pack, names, axes, shifts, **kw)) == len(shifts)
            continue
        flat, wflat = reduce_fields_level(pack, names, axes, shifts, expect=capi.EINVAL, **kw)
        assert np.isnan(flat).all() and np.isnan(wflat).all(), text
        assert text in pack.L.artemis_hip_last_error().decode(), (text, pack.L.artemis_hip_last_error().decode())


# ---- host driver ------------------------------------------------------------------------------------------------------
NAMES = ["gas.prim.density", "gas.prim.velocity", "gas.cons.density", "gas.cons.total_energy"]
NCOMP = 6
AMR = amr_cases.blast_amr(n=64)
RUNS = {  # deck, overrides, coordinates, the levels of the blocks after three cycles
    "visc3d": (test_multilevel.CASES["visc3d"]["deck"], test_multilevel.CASES["visc3d"]["ov"], "cartesian", (0, 1)),
    "sph3d": (test_multilevel.CASES["sph3d"]["deck"], test_multilevel.CASES["sph3d"]["ov"], "spherical", (0, 1)),
    "amr": (AMR["deck"], AMR["overrides"], "cylindrical", (0, 1, 2)),
}


def block_volumes(s, coordinates):
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    out = []
    for b in range(s.nblocks):
        bd = s.block_bounds(b)
        out.append(oracle_volumes(nx, bd[0::2], bd[1::2], s.is_ if nx[0] > 1 else 2, coordinates))
    return out


def same_state(a, b):
    (ca, fa), (cb, fb) = state_of(a), state_of(b)
    return ca == cb and len(fa) == len(fb) and all(np.array_equal(x, y) for x, y in zip(fa, fb))


@pytest.mark.parametrize("run", list(RUNS))
def test_refined_meshes_on_every_level(hiplib, tmp_path, run):
    """Three refined meshes after three cycles, stepped beside a twin that never gathers.
    (a) gather(reduce, reduce_level) is bitwise the emulation of gather(), for every proper subset of the active directions and
        every level the mesh allows, in double and float -- also through a 1 MiB staging buffer that cuts the block ranges.
    (b) every active direction reduced: any reduce_level gives gather(reduce=all) bit for bit.
    (d) under every coarser block the mean N / W is that block's own reduced N / W replicated, bitwise; and in reduced() of the
        version-4 dump of the finest level, every cell met by blocks of the coarsest level alone holds the mean that
        reduced() of the coarsest level's dump holds there.
    (e) visc3d (Cartesian): the sum of reduced("gas.cons.density", "integral") over all cells equals the fully reduced dump
        within 2 gamma_{n-1} S, n the number of terms added.
    (f) clock and all fields are those of the twin."""
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    from artemis_amd.fields import read_fields
    deck, ov, coordinates, levels_want = RUNS[run]
    s, twin = Simulation(DECK(*deck), ov), Simulation(DECK(*deck), ov)
    nx = (s.ie - s.is_ + 1, s.je - s.js + 1, s.ke - s.ks + 1)
    active = tuple(n > 1 for n in nx)
    every = sum(1 << d for d in range(3) if active[d])
    first = 4 if active[2] else 2  # the last active direction reduced: whole columns of root blocks stay unrefined
    for cycle in range(3):  # (f): gathers between the cycles, ranges cut and not
        assert s.evolve(1) == 1 and twin.evolve(1) == 1
        lv = [s.block_level(b) for b in range(s.nblocks)]
        got = s.gather(["gas.prim.velocity"] * 32, reduce=names_of(first), reduce_level=max(lv))
        with capi.option("fields_stage_mb", 1):  # (97 rows of doubles: 48 KiB a block of 8 x 8 cells at shift 0, four times that a level coarser)
            cut = s.gather(["gas.prim.velocity"] * 32, reduce=names_of(first), reduce_level=max(lv))
        assert len(got) == s.nblocks and all(same_bits(x, y) for x, y in zip(got, cut))
    assert same_state(s, twin)
    levels = [s.block_level(b) for b in range(s.nblocks)]
    assert set(levels) == set(levels_want)
    full, vols = s.gather(NAMES), block_volumes(s, coordinates)
    before = state_of(s)
    for axes in subsets(nx):
        own = [reduce_block(full[b], vols[b], axes) for b in range(s.nblocks)]
        red = names_of(axes)
        plain = s.gather(NAMES, reduce=red)
        assert all(same_bits(plain[b], own[b]) for b in range(s.nblocks))
        for L in allowed_levels(levels_want, nx, axes):
            want = [resample_reduced(own[b], levels[b] - L, axes, active) for b in range(s.nblocks)]
            got = s.gather(NAMES, reduce=red, reduce_level=L)
            assert len(got) == s.nblocks and all(same_bits(x, w) for x, w in zip(got, want)), (run, red, L)       # (a)
            got32 = s.gather(NAMES, single=True, reduce=",".join(red), reduce_level=L)
            assert all(same_bits(x, w.astype(np.float32)) for x, w in zip(got32, want)), (run, red, L)
            if axes == every:
                assert all(same_bits(got[b], plain[b]) for b in range(s.nblocks)), (run, L)                        # (b)
            for b in range(s.nblocks):                                                                             # (d)
                if levels[b] < L and axes != every:
                    mean = own[b][:-1] / own[b][-1:]
                    for d in kept_directions(axes, active):
                        mean = np.repeat(mean, 1 << (L - levels[b]), axis=3 - d)
                    assert same_bits(got[b][:-1] / got[b][-1:], mean), (run, red, L, b)
    # the dumps of the coarsest and of the finest level
    lo, hi = min(levels_want), max(levels_want)
    fds = {}
    for L in (lo, hi):
        s.write_fields(tmp_path / ("L%d.fld" % L), NAMES, reduce=names_of(first), reduce_level=L)
        fds[L] = fd = read_fields(tmp_path / ("L%d.fld" % L))
        assert fd.version == 4 and fd.reduce == list(names_of(first)) and fd.reduce_level == L and fd.level is None
        blocks = [dict(bounds=s.block_bounds(b)) for b in range(s.nblocks)]
        want = [reduce_block_level(full[b], vols[b], first, levels[b] - L) for b in range(s.nblocks)]
        N, W, cover = place_sum(blocks, [w[:-1] for w in want], [w[-1:] for w in want], first, nx)
        assert cover.min() >= 1
        at = 0
        for v in NAMES:
            n = fd.variables[v]
            assert same_bits(fd.reduced(v, "integral"), N[at:at + n]) and same_bits(fd.reduced(v), N[at:at + n] / W), (run, L, v)
            at += n
        assert same_bits(fd.reduced("volume"), W)
    # (d) on the assembled arrays: where only blocks of the coarsest level meet a cell, the finest dump repeats its mean
    finest_met = place_sum(blocks, [np.full((1,) + w.shape[1:], float(l != lo)) for w, l in zip(want, levels)],
                           [np.zeros((1,) + w.shape[1:]) for w in want], first, nx)[0][0]
    coarse, fine = fds[lo].reduced("gas.prim.velocity"), fds[hi].reduced("gas.prim.velocity")
    rep = coarse
    for d in kept_directions(first, active):
        rep = np.repeat(rep, 1 << (hi - lo), axis=3 - d)
    pure = finest_met == 0.0
    assert rep.shape == fine.shape and pure.any() and not pure.all()
    assert np.array_equal(rep.view(np.uint64)[:, pure], fine.view(np.uint64)[:, pure])
    if run == "visc3d":  # (e)
        s.write_fields(tmp_path / "all.fld", NAMES, reduce=names_of(every))
        whole = read_fields(tmp_path / "all.fld").reduced("gas.cons.density", "integral")
        assert whole.shape == (1, 1, 1, 1)
        m = len(kept_directions(first, active))
        for L in (lo, hi):
            # The cells of the dump are sums of the terms rho V of the mesh: the share 2^-k of a partial sum is the partial sum
            # of the terms times 2^-k (exact), so each of the 2^k cells under a coarse zone is a summation of that zone's terms,
            # and the total is one summation, in some order, of n terms: every zone's, counted once for each cell it feeds.
            # The fully reduced dump is another summation of the zones' own terms (fewer).  Each is within gamma_{n-1} S of the
            # exact sum; S = the sum of |terms| = the mass, all terms positive.
            n = sum(512 << (m * max(0, L - l)) for l in levels)
            total = float(np.sum(fds[L].reduced("gas.cons.density", "integral")))
            bound = 2.0 * gamma(n - 1) * abs(whole[0, 0, 0, 0])
            print(run, "level %d: sum of the cells %.17g, fully reduced %.17g, difference %.3e, bound %.3e (n = %d)"
                  % (L, total, whole[0, 0, 0, 0], abs(total - whole[0, 0, 0, 0]), bound, n))
            assert abs(total - whole[0, 0, 0, 0]) <= bound
    after = state_of(s)
    assert before[0] == after[0] and all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    assert same_state(s, twin)
    with pytest.raises(ValueError, match="reduce together with level"):
        s.gather(NAMES, level=0, reduce=("x1",))
    with pytest.raises(ValueError, match="reduce_level is only valid beside reduce"):
        s.gather(NAMES, reduce_level=0)
    with pytest.raises(ValueError, match="reduce_level together with level"):
        s.gather(NAMES, level=0, reduce=("x1",), reduce_level=0)
    with pytest.raises(RuntimeError, match=r"shift -4, \|shift\| <= 3 is built"):
        s.gather(NAMES, reduce=("x1",), reduce_level=4)
    s.close(), twin.close()


def test_one_level_mesh_at_its_own_level_is_the_plain_reduce(hiplib):
    """(c) the one-level 32^3 blast in eight 16^3 blocks: reduce_level = 0 returns gather(reduce=...) bit for bit, for every
    subset of the directions, in double and float."""
    from artemis_amd.driver import Simulation
    s = Simulation(DECK("blast", "blast.in"), BLAST32 + ["parthenon/time/nlim=3"])
    s.evolve(3)
    assert s.nblocks == 8
    for axes in range(1, 8):
        for single in (False, True):
            plain = s.gather(NAMES, single=single, reduce=names_of(axes))
            got = s.gather(NAMES, single=single, reduce=names_of(axes), reduce_level=0)
            assert len(got) == 8 and same_bits(np.stack(got), plain), (axes, single)
    s.close()


@pytest.mark.parametrize("run", ["visc3d", "amr"])
def test_deck_block_with_reduce_level(hiplib, tmp_path, run):
    """A `fld` block with reduce = x3 (x2 in 2-D) and reduce_level = 1 beside a plain one: the dumps appear on the plain block's
    schedule, are version 4 and hold the emulation of the plain ones; the run with the block is byte-identical in state to
    the run without, as are the plain dumps; blocks that cannot be served are listed as skipped."""
    from artemis_amd.driver import Simulation
    from artemis_amd.fields import read_fields
    deck, ov, coordinates, _ = RUNS[run]
    ov = [o for o in ov if "nlim" not in o] + ["parthenon/time/nlim=5"]
    v = ", ".join(NAMES)
    axes = 4 if run == "visc3d" else 2
    blk = lambda n, *extra: ["parthenon/output%d/file_type=fld" % n, "parthenon/output%d/dt=1e-9" % n,
                             "parthenon/output%d/variables=%s" % (n, v)] + ["parthenon/output%d/%s" % (n, e) for e in extra]
    red = "reduce=" + ",".join(names_of(axes))
    more = blk(12, red, "reduce_level=1") + blk(13, red, "reduce_level=5") + blk(14, "reduce_level=1") + blk(15, red, "level=0", "reduce_level=1")
    a, b = Simulation(DECK(*deck), ov + blk(11) + more), Simulation(DECK(*deck), ov + blk(11))
    a.enable_outputs(tmp_path / "a"), b.enable_outputs(tmp_path / "b")
    a.evolve(), b.evolve()
    st = {q["index"]: q for q in a.outputs()["blocks"]}
    assert st[12]["status"] == "active" and st[12]["reduce"] == list(names_of(axes)) and st[12]["reduce_level"] == 1
    assert st[13]["status"].startswith("skipped: reduce_level 5: a block on level ") and st[13]["status"].endswith(", |shift| <= 3 is built")
    assert st[14]["status"] == "skipped: reduce_level: only valid beside reduce"
    assert st[15]["status"] == "skipped: reduce: a block that also sets level is not built"
    assert same_state(a, b) and a.ncycle == 5
    files = os.listdir(tmp_path / "a")
    ones = sorted(os.listdir(tmp_path / "b"))
    assert ones == sorted(f for f in files if ".out11." in f) and len(ones) >= 5  # a dump every cycle, and the final one
    assert sorted(f.replace(".out12.", ".out11.") for f in files if ".out12." in f) == ones
    assert not [f for f in files if ".out11." not in f and ".out12." not in f]
    nx = (a.ie - a.is_ + 1, a.je - a.js + 1, a.ke - a.ks + 1)
    for f in ones[-2:]:
        for part in ("meta.json", "rank0.bin"):
            assert open(tmp_path / "a" / f / part, "rb").read() == open(tmp_path / "b" / f / part, "rb").read(), (f, part)
        fd, rd = read_fields(tmp_path / "a" / f), read_fields(tmp_path / "a" / f.replace(".out11.", ".out12."))
        meta = json.load(open(tmp_path / "a" / f.replace(".out11.", ".out12.") / "meta.json"))
        assert meta["version"] == 4 and meta["reduce_level"] == 1 and meta["variables"][-1]["name"] == "volume" and fd.version == 1
        assert (rd.time, rd.cycle) == (fd.time, fd.cycle) and len(rd.blocks) == len(fd.blocks)
        full = np.concatenate([np.stack(fd.get_blocks(name)) for name in NAMES], axis=1)
        for g, q in enumerate(fd.blocks):
            bd = q["bounds"]
            w = reduce_block_level(full[g], oracle_volumes(nx, bd[0::2], bd[1::2], a.is_ if nx[0] > 1 else 2, coordinates), axes, q["level"] - 1)
            got = np.concatenate([rd.get_blocks(name)[g] for name in NAMES + ["volume"]], axis=0)
            assert meta["blocks"][g]["nx"] == list(w.shape[:0:-1]) and same_bits(got, w), (f, g)
        assert not np.isnan(rd.reduced("gas.prim.density")).any()
    before = state_of(a)
    with pytest.raises(ValueError, match="was reduced along .*: not a state"):
        a.load_fields(tmp_path / "a" / ones[-1].replace(".out11.", ".out12."))
    after = state_of(a)
    assert before[0] == after[0] and all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    a.close(), b.close()
