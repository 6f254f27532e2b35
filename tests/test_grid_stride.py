"""The second and later trips of every grid-stride loop.  The field packs, the reductions, the history sums and the
timestep kernels cap their grid (1024 .. 4096 workgroups) and cover the remaining tiles by grid stride; on the small
packs of this suite every workgroup has one tile and the stride loop runs once.  GRID_CAP lowers the cap: at 1 a single
workgroup walks every tile of every block, at 3 the tiles are dealt 0, 3, 6, ... / 1, 4, 7, ... / 2, 5, 8, ...

Everything but the history sums must give the same bits as with one tile per workgroup, so each result is held against
the reference its own test module uses (the numpy emulations of tests/fields_level_ref.py and tests/fields_reduce_ref.py,
artemis_hip_prim_to_cons, the CPU oracle's EstimateTimestepMesh).  The history sums depend on the number of partial rows
by design: they are held to the exactly rounded sum of the same terms within the bound of tests/test_outputs.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import test_fields_level as lvl
import test_fields_reduce as red
import test_scatter as sc
from fields_level_ref import oracle_volumes, resample, same_bits
from fields_reduce_ref import reduce_block, subsets
from test_fields import DUST, GAS, pack_fields
from test_outputs import gamma
from test_parity_diffusion import pair
from test_parity_ops import make_pair, push

pytestmark = pytest.mark.gpu

CAPS = (1, 3)
NAN = float("nan")
THREE = "three"  # 3 blocks of 24 x 6 x 4, gas and one dust species: 24 tiles of 64 x 4 zones
NAMES = GAS + DUST


@functools.lru_cache(maxsize=None)
def three_reference():
    """(full-resolution components, volumes per block) of the pack `three`: formed once, never modified"""
    nb, nx, lo, hi, nsg, nsd, coords, ng = lvl.PACKS[THREE]
    xmin, xmax = lvl.block_bounds(THREE)
    want = lvl.full_components(lvl.make_pack(THREE)[0])
    vols = [oracle_volumes(nx, xmin[b], xmax[b], ng, coords) for b in range(nb)]
    for a in list(want.values()) + vols:
        a.setflags(write=False)
    return want, vols


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("cap", CAPS)
def test_pack_fields_and_levels(hiplib, cap, single):
    """artemis_hip_pack_fields == PrimToCons's values; artemis_hip_pack_fields_level with a restricted, an unchanged and a
    replicated block == the numpy tree."""
    from artemis_amd import capi
    mb, g, d = lvl.make_pack(THREE)
    want, vols = three_reference()
    full = np.concatenate([want[v] for v in NAMES], axis=1)
    with capi.option("grid_cap", cap):
        got = pack_fields(mb, NAMES, single=single)
        levels = lvl.pack_fields_level(mb, NAMES, (1, 0, -1), single=single)
        finer = lvl.pack_fields_level(mb, NAMES, (-1, -2), block0=1, single=single)
    assert same_bits(got, full.astype(np.float32) if single else full)
    for b, s in enumerate((1, 0, -1)):
        assert same_bits(levels[b], resample(full[b], vols[b], s, single)), (b, s)
    for b, s in enumerate((-1, -2)):
        assert same_bits(finer[b], resample(full[1 + b], vols[1 + b], s, single)), (b, s)
    assert np.array_equal(mb.gas_prim.cpu().numpy(), g) and np.array_equal(mb.dust_prim.cpu().numpy(), d)


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("cap", CAPS)
def test_reduce_fields_every_subset_of_axes(hiplib, cap, single):
    from artemis_amd import capi
    mb, _, _ = red.make_pack(THREE)
    want, vols = three_reference()
    full = np.concatenate([want[v] for v in NAMES], axis=1)
    for axes in subsets(mb.nx):
        with capi.option("grid_cap", cap):
            got = red.reduce_fields(mb, NAMES, axes, single=single)
        for b in range(mb.nb):
            assert same_bits(got[b], reduce_block(full[b], vols[b], axes, single)), (axes, b)


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("cap", CAPS)
def test_unpack_fields(hiplib, cap, single):
    """The primitive form: the interiors become the floored inputs, everything else stays (tests/test_scatter.py)."""
    from artemis_amd import capi
    mb, g, d = sc.make_pack("three_blocks")  # 3 blocks of 20 x 6 x 5: 30 tiles
    names = (sc.GAS_PRIM + sc.DUST_PRIM)[::-1]
    vals = sc.inputs(mb, names)
    arr = sc.joined(vals, names)
    if single:
        arr = arr.astype(np.float32)
        vals = {n: v.astype(np.float32).astype(np.float64) for n, v in vals.items()}
    with capi.option("grid_cap", cap):
        sc.unpack_fields(mb, names, arr)
    n, m = mb.nsg, mb.nsd
    want_g, want_d = g.copy(), d.copy()
    sc.put_interior(mb, want_g, list(range(0, n)), np.maximum(vals["gas.prim.density"], sc.DFLOOR))
    sc.put_interior(mb, want_g, list(range(n, 4 * n)), vals["gas.prim.velocity"])
    sc.put_interior(mb, want_g, list(range(5 * n, 6 * n)), np.maximum(vals["gas.prim.sie"], sc.SIEFLOOR))
    sc.put_interior(mb, want_d, list(range(0, m)), np.maximum(vals["dust.prim.density"], sc.DUST_DFLOOR))
    sc.put_interior(mb, want_d, list(range(m, 4 * m)), vals["dust.prim.velocity"])
    gp, dp, gu, du = sc.state(mb)
    assert np.array_equal(gp, want_g) and np.array_equal(dp, want_d)
    assert (gu == -555.0).all() and (du == -555.0).all()


# ---- timestep limits ----------------------------------------------------------------------------------------------------
def last_zone(o):
    return (o.ke, o.je, o.ie)


@pytest.mark.parametrize("placed", [False, True], ids=["random", "minimum-in-the-last-tile"])
def test_estimate_dt_and_timestep_all_hydro(hiplib, placed):
    """Three blocks of 33 x 7 x 5 (30 tiles of 64 x 4 zones; 15 flat tiles of 256 zones), gas and two dust species.
    `placed`: the fastest gas zone and the fastest dust zone are the last interior zone of the last block, which only a
    later trip of any workgroup reaches."""
    from artemis_amd import capi
    oracles, mb = make_pair((33, 7, 5), ns_gas=1, ns_dust=2, riem="hlle", seed=7, nb=3, cfl=0.3)
    before = [min(o.EstimateTimestepMesh(f) for o in oracles) for f in (0, 1)]
    if placed:
        o = oracles[-1]
        k, j, i = last_zone(o)
        o.gprim[1, k, j, i] = 1.0e4
        o.dprim[2 + 3 * 1 + 1, k, j, i] = -2.0e4  # (x2 velocity of the second species)
        o.PrimToCons()
        push(oracles, mb)
    want = [min(o.EstimateTimestepMesh(f) for o in oracles) for f in (0, 1)]
    if placed:
        assert want[0] < 0.5 * before[0] and want[1] < 0.5 * before[1]
        assert want[0] == oracles[-1].EstimateTimestepMesh(0) and want[1] == oracles[-1].EstimateTimestepMesh(1)
    for cap in CAPS:
        with capi.option("grid_cap", cap):
            assert mb.EstimateTimestepMesh(0, cfl=0.3) == want[0], cap
            assert mb.EstimateTimestepMesh(1, cfl=0.3) == want[1], cap
            assert mb.TimestepAll(0.3, 0.3, None) == min(want), cap


@pytest.mark.parametrize("placed", ["random", "hydro", "diffusion"])
def test_timestep_all_and_diffusion_dt(hiplib, placed):
    """One block of 24 x 12 x 10 (30 tiles; 12 flat tiles) with constant viscosity and conduction; the oracle's limit is
    the smallest of the hydrodynamic, the viscous and the conductive one.  random: the diffusive limit binds somewhere.
    hydro: the last interior zone is fast (v1 = 1e3) and carries the hydrodynamic limit, which then binds.  diffusion: the
    last interior zone is thin (density x 1e-3, velocity untouched): its conductive diffusivity cond / (rho cv) is a
    thousand times its neighbours', the diffusive limit binds there and the hydrodynamic one does not move.  In both placed
    states ONLY the last zone differs from the random state and every limit is a minimum over single zones, so a limit
    that fell is carried by that zone -- the last zone of the last tile, which only a later trip of a workgroup reaches."""
    from artemis_amd import capi
    from artemis_amd.pack import diffusion_params
    o, mb = pair((24, 12, 10), ns_gas=1, seed=51)
    oh, _ = pair((24, 12, 10), ns_gas=1, seed=51)  # the same state without diffusion: the hydrodynamic limit by itself
    o.set_viscosity("constant", nu=0.03, eta_bulk=0.4, averaging="arithmetic")
    o.set_conductivity("conductivity", averaging="arithmetic", cond=0.07)
    D = diffusion_params(1.4, viscosity=dict(type="constant", nu=0.03, eta_bulk=0.4, averaging="arithmetic"),
                         conductivity=dict(type="conductivity", averaging="arithmetic", cond=0.07))
    before, hyd_before = o.EstimateTimestepMesh(0), oh.EstimateTimestepMesh(0)
    assert before < hyd_before  # (the random state: diffusion binds)
    if placed != "random":
        k, j, i = last_zone(o)
        for q in (o, oh):
            if placed == "hydro":
                q.gprim[1, k, j, i] = 1.0e3
            else:
                q.gprim[0, k, j, i] *= 1.0e-3
            q.PrimToCons()
        push([o], mb)
    want, want_hyd = o.EstimateTimestepMesh(0), oh.EstimateTimestepMesh(0)
    if placed == "hydro":  # the fast zone carries the hydrodynamic limit, and that limit binds
        assert want == want_hyd and want_hyd < 0.01 * hyd_before
    if placed == "diffusion":  # the thin zone carries the diffusive limit, which binds; the hydrodynamic one has not moved
        assert want < 0.01 * before and want_hyd == hyd_before and want < 0.01 * want_hyd
    for cap in CAPS:
        with capi.option("grid_cap", cap):
            hyd, dif = mb.EstimateTimestepMesh(0, cfl=0.3), mb.DiffusionTimestep(D, 0.3)
            both = mb.TimestepAll(0.3, 0.3, D)
        assert hyd == want_hyd, (cap, hyd, want_hyd)
        assert min(hyd, dif) == want and both == want, (cap, hyd, dif, both, want)
        if placed == "hydro":
            assert hyd < dif and dif == before, (cap, hyd, dif)  # (the diffusive limit is the random state's)
        else:
            assert dif < hyd and dif == want, (cap, hyd, dif)


# ---- history sums -------------------------------------------------------------------------------------------------------
def history_sums(mb, rows):
    """artemis_hip_history_sums into NaN-filled buffers; `rows`: the partial rows the scratch must have room for"""
    nq = 6 * mb.nsg + 4 * mb.nsd
    nbytes = mb.L.artemis_hip_history_scratch_bytes(C.byref(mb.pack))
    assert nbytes == rows * nq * 8, (nbytes, rows, nq)
    scratch = torch.full((rows * nq + 64,), NAN, dtype=torch.float64, device=mb.dev)
    sums = torch.full((nq + 8,), NAN, dtype=torch.float64, device=mb.dev)
    mb._call(mb.L.artemis_hip_history_sums, C.c_void_p(sums.data_ptr()), C.c_void_p(scratch.data_ptr()))
    torch.cuda.synchronize()
    s, w = sums.cpu().numpy(), scratch.cpu().numpy()
    assert not np.isnan(s[:nq]).any() and np.isnan(s[nq:]).all()
    assert not np.isnan(w[:rows * nq]).any() and np.isnan(w[rows * nq:]).all()  # every row written, none past the last
    return s[:nq]


def history_terms():
    """The per-zone terms of the history layout for the pack `three` (one gas, one dust species): PrimToCons's values
    times the oracle's volumes, [10][zones of every block]"""
    want, vols = three_reference()
    v = np.stack(vols)[:, None]
    comps = np.concatenate([want["gas.cons.density"], want["gas.cons.momentum"], want["gas.cons.total_energy"],
                            want["gas.cons.internal_energy"], want["dust.cons.density"], want["dust.cons.momentum"]], axis=1)
    return (comps * v).transpose(1, 0, 2, 3, 4).reshape(10, -1)


# artemis_hip_history_sums of the pack `three` with GRID_CAP unset, as the commit before GRID_CAP existed computed them
# (float.hex of the ten sums, recorded from that commit's library on an MI355X): the default grid has not moved
DEFAULT_SUMS_BEFORE_THE_KNOB = [
    "0x1.ba58e2eecac1bp+1", "0x1.2272c3fcc49f5p-5", "-0x1.6c299ffdba81ap-6", "-0x1.41c20043d7fa8p-8", "0x1.08b5929c39e1ap+3",
    "0x1.16509b62bf45dp+2", "0x1.b257e81fb912cp+1", "-0x1.862d4a9c00cb8p-5", "-0x1.040f4072369adp-4", "0x1.ed1bf886590c8p-4"]


@pytest.mark.parametrize("cap", (0,) + CAPS)
def test_history_sums(hiplib, cap):
    from artemis_amd import capi
    mb, _, _ = lvl.make_pack(THREE)
    terms = history_terms()
    n = terms.shape[1]
    assert n == 3 * 24 * 6 * 4
    tiles = 3 * 1 * 2 * 4  # 64 x 4 tiles a plane, planes, blocks
    with capi.option("grid_cap", cap):
        got = history_sums(mb, min(cap, tiles) if cap else tiles)
        again = history_sums(mb, min(cap, tiles) if cap else tiles)
    assert got.tobytes() == again.tobytes()
    exact = np.array([math.fsum(t) for t in terms])
    S = np.array([math.fsum(np.abs(t)) for t in terms])
    err, bound = np.abs(got - exact), gamma(n - 1) * S
    print("cap", cap, "max err / bound", np.max(err / bound), "sums", [float(x).hex() for x in got])
    assert np.all(err <= bound), (cap, err, bound)
    if cap == 0:
        assert [float(x).hex() for x in got] == DEFAULT_SUMS_BEFORE_THE_KNOB
