"""GPU tests of artemis_hip_unpack_fields (kernels_fields.hip), the inverse of artemis_hip_pack_fields: a buffer in the
layout that kernel writes becomes the primitives of the interior zones.  Only repository code runs here.

Every comparison is bitwise unless it says otherwise.  The references are the inputs themselves with the floors applied
(primitive form), numpy's IEEE evaluation of P / ((gamma-1) rho) (pressure form), and what artemis_hip_set_aux followed by
artemis_hip_cons_to_prim leave in a copy of the pack whose conserved arrays hold the same inputs (conserved form).  The packs
are those of tests/test_fields.py plus one whose rows of 67 zones end inside the second 64-lane tile; ghost zones, the
pressure slot and the conserved arrays are poisoned beforehand and must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

from test_fields import DFLOOR, DUST_DFLOOR, PACKS as FIELD_PACKS, SIEFLOOR, interior, pack_fields

pytestmark = pytest.mark.gpu

# name: (nblocks, nx, lo, hi, ns_gas, ns_dust, coordinates, ng)
PACKS = dict(FIELD_PACKS, wide67=(2, (67, 5, 3), (-1, -0.5, 0.25), (1, 0.8, 0.95), 1, 1, "cartesian", 2))
GAMMA = 1.4
GAS_PRIM = ["gas.prim.density", "gas.prim.velocity", "gas.prim.sie"]
GAS_PRES = ["gas.prim.density", "gas.prim.velocity", "gas.prim.pressure"]
GAS_CONS = ["gas.cons.density", "gas.cons.momentum", "gas.cons.total_energy"]
DUST_PRIM = ["dust.prim.density", "dust.prim.velocity"]
DUST_CONS = ["dust.cons.density", "dust.cons.momentum"]


def make_pack(name, de_switch=0.0, seed=11):
    """(pack, host copies of its primitive arrays).  Every zone holds random primitives, the pressure slot -777 and the
    conserved arrays -555: whatever the kernel must leave alone is recognisable."""
    import torch
    from artemis_amd.pack import MeshBlockPack
    nb, nx, lo, hi, nsg, nsd, coords, ng = PACKS[name]
    edges = np.linspace(lo[0], hi[0], nb + 1)  # the blocks side by side along x1
    xmin = [[edges[b], lo[1], lo[2]] for b in range(nb)]
    xmax = [[edges[b + 1], hi[1], hi[2]] for b in range(nb)]
    mb = MeshBlockPack(nb, nx, xmin, xmax, ng=ng, ns_gas=nsg, ns_dust=nsd, gamma=GAMMA, dfloor=DFLOOR, siefloor=SIEFLOOR,
                       de_switch=de_switch, dust_dfloor=DUST_DFLOOR, coordinates=coords, with_fluxes=False)
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


def ncomp_of(mb, names):
    return sum((3 if n.endswith(("velocity", "momentum")) else 1) * (mb.nsd if n.startswith("dust") else mb.nsg) for n in names)


def inputs(mb, names, nblocks=None, seed=5):
    """{name: [nblocks, its components, nx3, nx2, nx1]}: densities, sie and pressures so that about a seventh of the zones
    sit below each floor, velocities and momenta of both signs, energies on both sides of the kinetic energy"""
    rng = np.random.default_rng(seed)
    nblocks = mb.nb if nblocks is None else nblocks
    out = {}
    for n in names:
        shape = (nblocks, ncomp_of(mb, [n]), mb.nx[2], mb.nx[1], mb.nx[0])
        if n.endswith(("velocity", "momentum")):
            out[n] = rng.uniform(-1.5, 1.5, size=shape)
        elif n.endswith("pressure"):
            out[n] = rng.uniform(0.1, 1.2, size=shape)  # (sie = P / (0.4 rho) < 0.75 in about a sixth of the zones)
        elif n.endswith("total_energy"):
            out[n] = rng.uniform(0.3, 3.0, size=shape)
        elif n.endswith("internal_energy"):
            out[n] = rng.uniform(0.3, 1.5, size=shape)
        else:
            out[n] = rng.uniform(0.5, 2.0, size=shape)
    return out


def unpack_fields(mb, names, arr, block0=0, nblocks=None, expect=0):
    """artemis_hip_unpack_fields of blocks [block0, block0 + nblocks) from the numpy array `arr` (its dtype decides `single`)"""
    import torch
    from artemis_amd import capi
    nblocks = arr.shape[0] if nblocks is None else nblocks
    sel = (C.c_int * max(len(names), 1))(*[n if isinstance(n, int) else capi.FIELD_VAR[n] for n in names])
    dev = torch.from_numpy(np.ascontiguousarray(arr)).to(mb.dev)
    rc = mb.L.artemis_hip_unpack_fields(C.byref(mb.pack), block0, nblocks, len(names), sel, int(arr.dtype == np.float32),
                                        C.c_void_p(dev.data_ptr()), mb._stream())
    torch.cuda.synchronize()
    msg = mb.L.artemis_hip_last_error().decode()
    assert rc == expect, (rc, msg)
    return msg


def joined(vals, names):
    return np.ascontiguousarray(np.concatenate([vals[n] for n in names], axis=1))


def state(mb):
    return [t.cpu().numpy() for t in (mb.gas_prim, mb.dust_prim, mb.gas_u0, mb.dust_u0)]


def put_interior(mb, full, comps, values):
    """`values` [nb, len(comps), nx3, nx2, nx1] into components `comps` of the interior of the whole array `full`"""
    full[:, comps, mb.ks:mb.ke + 1, mb.js:mb.je + 1, mb.is_:mb.ie + 1] = values


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("name", list(PACKS))
def test_primitive_form_is_the_floored_input(hiplib, name, single):
    mb, g, d = make_pack(name)
    names = GAS_PRIM + (DUST_PRIM if mb.nsd else [])
    names = names[::-1]  # (the components follow the order of the codes, whatever it is)
    vals = inputs(mb, names)
    arr = joined(vals, names)
    if single:
        arr = arr.astype(np.float32)
        vals = {n: v.astype(np.float32).astype(np.float64) for n, v in vals.items()}  # widened exactly
    unpack_fields(mb, names, arr)
    n, m = mb.nsg, mb.nsd
    want_g, want_d = g.copy(), d.copy()
    rho, sie = np.maximum(vals["gas.prim.density"], DFLOOR), np.maximum(vals["gas.prim.sie"], SIEFLOOR)
    assert (rho == DFLOOR).mean() > 0.08 and (sie == SIEFLOOR).mean() > 0.08
    put_interior(mb, want_g, list(range(0, n)), rho)
    put_interior(mb, want_g, list(range(n, 4 * n)), vals["gas.prim.velocity"])
    put_interior(mb, want_g, list(range(5 * n, 6 * n)), sie)
    if m:
        drho = np.maximum(vals["dust.prim.density"], DUST_DFLOOR)
        assert (drho == DUST_DFLOOR).mean() > 0.05
        put_interior(mb, want_d, list(range(0, m)), drho)
        put_interior(mb, want_d, list(range(m, 4 * m)), vals["dust.prim.velocity"])
    gp, dp, gu, du = state(mb)
    # interiors as asked; ghost zones and the pressure slot as they were; no conserved array touched
    assert np.array_equal(gp, want_g) and np.array_equal(dp, want_d)
    assert (gp[:, 4 * n:5 * n] == -777.0).all() and (gu == -555.0).all() and (du == -555.0).all()


@pytest.mark.parametrize("name", list(PACKS))
def test_unpack_of_pack_is_the_identity_on_a_floored_pack(hiplib, name):
    import torch
    mb, _, _ = make_pack(name)
    mb.PrimToCons()  # floors every zone
    torch.cuda.synchronize()
    before = state(mb)
    names = GAS_PRIM + (DUST_PRIM if mb.nsd else [])
    packed = pack_fields(mb, names)
    mb.gas_prim[:, :, mb.ks:mb.ke + 1, mb.js:mb.je + 1, mb.is_:mb.ie + 1] = 123.0  # (so that the values really come back)
    mb.gas_prim[:, 4 * mb.nsg:5 * mb.nsg] = torch.from_numpy(before[0][:, 4 * mb.nsg:5 * mb.nsg]).to(mb.dev)
    unpack_fields(mb, names, packed)
    for x, y in zip(state(mb), before):
        assert np.array_equal(x, y)


def cons_reference(name, de_switch, vals, with_eint):
    """Interior primitives that SetAuxillaryFields + ConsToPrim leave in a copy of the pack whose conserved arrays hold `vals`"""
    import torch
    ref, _, _ = make_pack(name, de_switch)
    n, m = ref.nsg, ref.nsd
    gu, du = ref.gas_u0.cpu().numpy(), ref.dust_u0.cpu().numpy()
    put_interior(ref, gu, list(range(0, n)), vals["gas.cons.density"])
    put_interior(ref, gu, list(range(n, 4 * n)), vals["gas.cons.momentum"])
    put_interior(ref, gu, list(range(4 * n, 5 * n)), vals["gas.cons.total_energy"])
    put_interior(ref, gu, list(range(5 * n, 6 * n)), vals["gas.cons.internal_energy"] if with_eint else 0.0)
    if m:
        put_interior(ref, du, list(range(0, m)), vals["dust.cons.density"])
        put_interior(ref, du, list(range(m, 4 * m)), vals["dust.cons.momentum"])
    ref.gas_u0.copy_(torch.from_numpy(gu)), ref.dust_u0.copy_(torch.from_numpy(du))
    ref.SetAuxillaryFields()
    ref.ConsToPrim()
    torch.cuda.synchronize()
    return interior(ref, ref.gas_prim.cpu().numpy()), interior(ref, ref.dust_prim.cpu().numpy())


def energy_branches(name, vals, de_switch):
    """Fraction of the zones in which SetAuxillaryFields takes E - ke (the rest takes the internal-energy variable).  The
    scale factors are taken at the cell centres, which is as good as exact for counting zones."""
    nb, nx, lo, hi, nsg, nsd, coords, ng = PACKS[name]
    D, M, E = vals["gas.cons.density"], vals["gas.cons.momentum"], vals["gas.cons.total_energy"]
    edges = np.linspace(lo[0], hi[0], nb + 1)
    x1 = np.stack([edges[b] + (np.arange(nx[0]) + 0.5) * (edges[b + 1] - edges[b]) / nx[0] for b in range(nb)])
    x1 = x1.reshape(nb, 1, 1, 1, nx[0])
    x2 = (lo[1] + (np.arange(nx[1]) + 0.5) * (hi[1] - lo[1]) / nx[1]).reshape(1, 1, 1, nx[1], 1)
    h = {"cartesian": [1.0, 1.0, 1.0], "cylindrical": [1.0, x1, 1.0], "spherical": [1.0, x1, x1 * np.sin(x2)]}[coords]
    ke = sum((M[:, q::3] / h[q]) ** 2 for q in range(3))  # (component 3 n + q of species n)
    ke = 0.5 * ke / np.maximum(D, DFLOOR)
    return float(((E - ke) > de_switch * E).mean())


@pytest.mark.parametrize("with_eint", [True, False], ids=["eint", "no_eint"])
@pytest.mark.parametrize("de_switch", [0.0, 0.3])
@pytest.mark.parametrize("name", list(PACKS))
def test_conserved_form_equals_set_aux_and_cons_to_prim(hiplib, name, de_switch, with_eint):
    mb, g, d = make_pack(name, de_switch)
    names = GAS_CONS + (["gas.cons.internal_energy"] if with_eint else []) + (DUST_CONS if mb.nsd else [])
    vals = inputs(mb, GAS_CONS + ["gas.cons.internal_energy"] + (DUST_CONS if mb.nsd else []))
    took_e = energy_branches(name, vals, de_switch)
    assert 0.1 < took_e < 0.9, took_e  # both branches of the energy switch occur in the input
    assert (vals["gas.cons.density"] < DFLOOR).mean() > 0.08
    unpack_fields(mb, names, joined(vals, names))
    want_g, want_d = cons_reference(name, de_switch, vals, with_eint)
    gp, dp, gu, du = state(mb)
    n = mb.nsg
    keep = [c for c in range(6 * n) if not 4 * n <= c < 5 * n]
    assert np.array_equal(interior(mb, gp)[:, keep], want_g[:, keep])
    assert (interior(mb, gp)[:, 5 * n:] == SIEFLOOR).mean() > 0.02  # the sie floor binds somewhere
    assert np.array_equal(interior(mb, dp), want_d)
    # the rest of the pack is as it was
    put_interior(mb, g, keep, interior(mb, gp)[:, keep])
    put_interior(mb, d, list(range(4 * mb.nsd)), interior(mb, dp))
    assert np.array_equal(gp, g) and np.array_equal(dp, d) and (gu == -555.0).all() and (du == -555.0).all()


@pytest.mark.parametrize("name", ["cart3d", "cart1d", "sph3d", "wide67"])
def test_pressure_form(hiplib, name):
    """sie = P / ((gamma-1) rho_floored), the product first, one IEEE division, then the floor: numpy's evaluation, bitwise.
    pack_fields then forms fl(fl((gamma-1) rho) sie): with q = fl((gamma-1) rho) the stored sie is (P / q)(1 + e1) and the
    returned pressure q sie (1 + e2), |e1|, |e2| <= 2^-53, so it is within 2^-52 + 2^-106 < 2^-51 of P -- derived, not measured.
    That holds where the sie floor does not bind; where it binds the returned pressure is that of the floor, exactly."""
    mb, g, d = make_pack(name)
    vals = inputs(mb, GAS_PRES)
    unpack_fields(mb, GAS_PRES, joined(vals, GAS_PRES))
    rho = np.maximum(vals["gas.prim.density"], DFLOOR)
    raw = vals["gas.prim.pressure"] / ((GAMMA - 1.0) * rho)
    sie = np.maximum(raw, SIEFLOOR)
    n = mb.nsg
    gp = mb.gas_prim.cpu().numpy()
    assert np.array_equal(interior(mb, gp)[:, 5 * n:], sie) and np.array_equal(interior(mb, gp)[:, :n], rho)
    assert (gp[:, 4 * n:5 * n] == -777.0).all()  # the pressure slot is not written
    back = pack_fields(mb, ["gas.prim.pressure"])
    free = raw > SIEFLOOR
    assert 0.05 < 1.0 - free.mean() < 0.5
    rel = np.abs(back[free] - vals["gas.prim.pressure"][free]) / vals["gas.prim.pressure"][free]
    print("pressure round trip: max relative error %.3g (bound %.3g)" % (rel.max(), 2.0 ** -51))
    assert rel.max() <= 2.0 ** -51
    assert np.array_equal(back[~free], ((GAMMA - 1.0) * rho * SIEFLOOR)[~free])


def test_block_ranges_and_partial_selections(hiplib):
    mb, g, d = make_pack("three_blocks")
    names = GAS_PRIM + DUST_PRIM
    vals = inputs(mb, names, nblocks=2)
    unpack_fields(mb, names, joined(vals, names), block0=1, nblocks=2)
    gp, dp, gu, du = state(mb)
    assert np.array_equal(gp[0], g[0]) and np.array_equal(dp[0], d[0])  # block 0 is untouched
    assert np.array_equal(interior(mb, gp)[1:, 0:1], np.maximum(vals["gas.prim.density"], DFLOOR))
    assert np.array_equal(interior(mb, dp)[1:, 1:4], vals["dust.prim.velocity"])
    assert np.array_equal(interior(mb, gp)[1:, 1:4], vals["gas.prim.velocity"])
    unpack_fields(mb, names, joined(vals, names)[:0], block0=3, nblocks=0)  # an empty range at the end is no error
    # one fluid named: the other one's arrays stay as they are, interiors included
    mb, g, d = make_pack("three_blocks")
    vals = inputs(mb, DUST_CONS)
    unpack_fields(mb, DUST_CONS, joined(vals, DUST_CONS))
    gp, dp, _, _ = state(mb)
    assert np.array_equal(gp, g) and not np.array_equal(dp, d)
    assert np.array_equal(interior(mb, dp)[:, 0:1], np.maximum(vals["dust.cons.density"], DUST_DFLOOR))
    mb, g, d = make_pack("three_blocks")
    vals = inputs(mb, GAS_PRIM)
    unpack_fields(mb, GAS_PRIM, joined(vals, GAS_PRIM))
    gp, dp, _, _ = state(mb)
    assert np.array_equal(dp, d) and not np.array_equal(gp, g)
    unpack_fields(mb, [], np.zeros((3, 0, 5, 6, 20)))  # nothing named: nothing done
    assert np.array_equal(mb.gas_prim.cpu().numpy(), gp)


def test_bad_arguments_are_refused_and_name_the_cause(hiplib):
    from artemis_amd import capi
    from artemis_amd.pack import MeshBlockPack
    three, g, d = make_pack("three_blocks")
    gas_only, g1, d1 = make_pack("sph3d")
    buf = np.zeros((3, 16, 5, 6, 20))
    small = np.zeros((1, 16, 6, 8, 16))
    bad = [(GAS_PRIM[:2] + ["gas.cons.total_energy"], "mix the primitive and the conserved form"),
           (["gas.prim.density", "gas.prim.velocity"], "gas.prim.sie or gas.prim.pressure is missing"),
           (["gas.prim.velocity", "gas.prim.sie"], "gas.prim.density is missing"),
           (GAS_PRIM + ["gas.prim.pressure"], "both given"),
           (["gas.cons.density", "gas.cons.total_energy"], "gas.cons.momentum is missing"),
           (["gas.cons.internal_energy"], "gas.cons.density is missing"),
           (GAS_PRIM + ["dust.prim.density"], "dust.prim.velocity is missing"),
           (GAS_PRIM + ["dust.prim.density", "dust.cons.momentum"], "dust variables mix"),
           (GAS_PRIM + ["gas.prim.density"], "gas.prim.density is given twice"),
           (GAS_PRIM + [12], "unknown variable code 12"), ([-1], "unknown variable code -1"), (GAS_PRIM + [1000], "unknown variable code 1000")]
    for names, text in bad:
        assert text in unpack_fields(three, names, buf, expect=capi.EINVAL), names
    for names in (GAS_PRIM + DUST_PRIM, DUST_CONS):
        assert "on a pack without dust" in unpack_fields(gas_only, names, small, expect=capi.EINVAL)
    nb, nx, lo, hi, _, _, coords, ng = PACKS["cart3d"]
    dust_only = MeshBlockPack(1, nx, [list(lo)], [list(hi)], ng=ng, ns_gas=0, ns_dust=1, gamma=GAMMA, with_fluxes=False)
    dust_only.dust_prim.fill_(3.0)
    assert "on a pack without gas" in unpack_fields(dust_only, GAS_PRIM, small, expect=capi.EINVAL)
    assert (dust_only.dust_prim == 3.0).all()
    for b0, n in ((0, 4), (2, 2), (3, 1), (-1, 1), (0, -1), (4, 0)):
        assert "not inside the pack" in unpack_fields(three, GAS_PRIM, buf, b0, n, expect=capi.EINVAL)
    # none of it wrote anything
    gp, dp, gu, du = state(three)
    assert np.array_equal(gp, g) and np.array_equal(dp, d) and (gu == -555.0).all() and (du == -555.0).all()
    assert np.array_equal(gas_only.gas_prim.cpu().numpy(), g1)
