"""GPU parity of the lean form of the Cartesian stage.

With the redo list on and gas/de_switch = 0 the stage runs stage_fused_kernel_lean: the tile march without the second
energy equation (no slope, face value or upwinded flux of `sie`, no face velocity, no update of cons::internal_energy).
SetAuxillaryFields reads that equation's result only in zones where the total-energy update leaves !(ue > de_switch * E);
the lean kernel does not store such a zone but appends it to the redo list, and stage_redo_kernel recomputes it with
the full expression set.  The claim: the bits of the CPU oracle in every zone, whichever share of the zones is
deferred -- none, some, all -- and the bits of the full kernel (option NO_LEAN_ENERGY).  The option LEAN_ENERGY selects
the lean kernel for a positive switch as well, which is how the tests below fill the list; artemis_hip_redo_totals
counts what the redo kernel processed, so that no case is vacuous.

Blocks: test_parity_flat_waves.py's (ragged tiles; tile (1, 1) has all four perimeter lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.oracle import Oracle
from test_parity_fused import fused_step
from test_parity_ops import random_state, same

pytestmark = pytest.mark.gpu

SHAPES = {"3d": (72, 20, 36), "2d": (72, 20, 1)}
BCS = {"hllc": "outflow", "hlle": "periodic", "llf": "reflecting"}
LO, HI = (-1.0, -0.7, 0.1), (1.0, 0.9, 1.3)
STEPS, STAGES = 2, 2  # rk2


@pytest.fixture(autouse=True)
def _lean_switches_restored():
    """The two switches of this file are process-wide; put back what a test found."""
    from artemis_amd import capi
    L = capi.load()
    before = {n: L.artemis_hip_get_option(n) for n in (b"LEAN_ENERGY", b"NO_LEAN_ENERGY")}
    yield
    for n, v in before.items():
        L.artemis_hip_set_option(n, v)


def build(dim, riem, de_switch, state):
    """An oracle and a pack of their own (both take de_switch), holding the same start-of-run state."""
    from artemis_amd.pack import MeshBlockPack
    nx, bc = SHAPES[dim], (BCS[riem],) * 6
    kw = dict(ng=2, reconstruct="plm", riemann=riem, gamma=1.4, dfloor=1e-10, siefloor=1e-10, de_switch=de_switch)
    o = Oracle(nx, LO, HI, cfl=0.3, bc=bc, integrator="rk2", **kw)
    if state == "blast":
        o.pgen_blast(radius=0.3, internal_energy=1.0, p0=1e-5, d0=1.0, x0=(0.0, 0.1, 0.7), samples=0)
    else:
        random_state(o, np.random.default_rng(17), mach=1.0, contrast=30.0)
        if state == "cold":
            o.gprim[5] *= 1.0e-9
        o.ApplyBoundaryConditions()
        o.PrimToCons()
    mb = MeshBlockPack(1, nx, [LO], [HI], with_fluxes=False, **kw)
    start = o.gprim.copy()
    return o, mb, bc, start


def oracle_steps(o):
    """[(dt, prim, cons)] of STEPS rk2 steps."""
    out = []
    for _ in range(STEPS):
        dt = o.new_dt()
        o.dt = dt
        o.step()
        assert np.isfinite(o.gprim).all(), "the oracle itself left the finite range"
        out.append((dt, o.gprim.copy(), o.gu0.copy()))
    return out


def gpu_steps(mb, bc, start, dts):
    """The same steps on the device from `start`: ([(prim, cons)] per step, (bulk, shell) deferred zones)."""
    from artemis_amd import capi
    mb.gas_prim[0].copy_(torch.from_numpy(start.copy()))
    bufs = [(mb.gas_prim, mb.pack.gas.prim), mb.new_prim_buffer("B"), mb.new_prim_buffer("C")]
    capi.redo_totals(reset=True)
    out = []
    for dt in dts:
        fused_step(mb, bufs, "rk2", dt, [bc])
        mb.PrimToCons()  # materialise P in the ghosts and the conserved state for comparison
        out.append((mb.gas_prim[0].cpu().numpy().copy(), mb.gas_u0[0].cpu().numpy().copy()))
    return out, capi.redo_totals()


def check(got, ref, what):
    for step, ((gp, gc), (_, rp, rc)) in enumerate(zip(got, ref)):
        same(torch.from_numpy(gp), rp, f"{what}: prim after step {step}")
        same(torch.from_numpy(gc), rc, f"{what}: cons after step {step}")


def zones(dim):
    nx = SHAPES[dim]
    return nx[0] * nx[1] * nx[2]


@pytest.mark.parametrize("state", ["random", "blast"])
@pytest.mark.parametrize("dim", sorted(SHAPES))
@pytest.mark.parametrize("riem", sorted(BCS))
def test_default_path_matches_oracle_and_full_kernel(hiplib, option, riem, dim, state):
    """gas/de_switch = 0: the lean kernel is what runs.  The oracle's bits; and once more with NO_LEAN_ENERGY: the same
    arrays, nothing deferred."""
    o, mb, bc, start = build(dim, riem, 0.0, state)
    ref = oracle_steps(o)
    dts = [r[0] for r in ref]
    lean, n_lean = gpu_steps(mb, bc, start, dts)
    print("deferred zones (bulk, shell) on the lean path:", n_lean)
    check(lean, ref, "lean")
    option("no_lean_energy")
    full, n_full = gpu_steps(mb, bc, start, dts)
    for step, ((lp, lc), (fp, fc)) in enumerate(zip(lean, full)):
        assert np.array_equal(lp, fp) and np.array_equal(lc, fc), f"lean and full kernels differ after step {step}"
    assert n_full == (0, 0), n_full


def test_default_path_device_timestep(hiplib):
    """The last stage also reduces the CFL timestep on the device: the oracle's dt, deferred zones or not."""
    o, mb, bc, start = build("3d", "hllc", 0.0, "random")
    mb.gas_prim[0].copy_(torch.from_numpy(start.copy()))
    bufs = [(mb.gas_prim, mb.pack.gas.prim), mb.new_prim_buffer("B"), mb.new_prim_buffer("C")]
    dt_dev = torch.empty(1, dtype=torch.float64, device="cuda")
    for step in range(STEPS):
        dt = o.new_dt()
        o.dt = dt
        o.step()
        dt_dev.fill_(torch.finfo(torch.float64).max)
        fused_step(mb, bufs, "rk2", dt, [bc], dt_dev=C.c_void_p(dt_dev.data_ptr()), cfl=0.3)
        mb.PrimToCons()
        same(mb.gas_prim[0], o.gprim, f"prim after step {step}")
        same(mb.gas_u0[0], o.gu0, f"cons after step {step}")
        assert dt_dev.item() == o.new_dt(), "fused EstimateTimestepMesh"


@pytest.mark.parametrize("dim,riem", [("3d", "hllc"), ("2d", "hllc"), ("3d", "hlle"), ("3d", "llf")])
def test_mixed_waves(hiplib, option, dim, riem):
    """de_switch = 0.4 on the forced lean path: a share of the zones of every wave is deferred, the rest is stored."""
    o, mb, bc, start = build(dim, riem, 0.4, "random")
    I = np.s_[o.ks:o.ke + 1, o.js:o.je + 1, o.is_:o.ie + 1]
    e = start[5][I]
    share = np.mean(e / (e + 0.5 * (start[1][I] ** 2 + start[2][I] ** 2 + start[3][I] ** 2)) <= 0.4)
    print("share of interior zones with e / (e + v^2 / 2) <= 0.4 in the initial state: %.3f" % share)
    assert 0.2 < share < 0.8, share  # (the input is what the test needs)
    ref = oracle_steps(o)
    option("lean_energy")
    got, (bulk, shell) = gpu_steps(mb, bc, start, [r[0] for r in ref])
    print("deferred zones:", bulk, shell, "of", zones(dim) * STAGES * STEPS)
    check(got, ref, "mixed")
    assert 0 < bulk + shell < zones(dim) * STAGES * STEPS


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_every_zone_deferred(hiplib, option, dim):
    """de_switch = 2: ue > 2 E fails wherever E > 0, so the redo kernel computes every zone of every stage -- the list
    at full length, the grid-stride loop."""
    o, mb, bc, start = build(dim, "hllc", 2.0, "random")
    ref = oracle_steps(o)
    option("lean_energy")
    got, (bulk, shell) = gpu_steps(mb, bc, start, [r[0] for r in ref])
    check(got, ref, "every zone deferred")
    assert bulk + shell == zones(dim) * STAGES * STEPS, (bulk, shell)


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_cold_gas(hiplib, dim):
    """Internal energies of 1e-9 under velocities of order one (de_switch = 0, the default path): wherever the
    total-energy update leaves no positive internal energy the zone takes the equation from the redo kernel."""
    o, mb, bc, start = build(dim, "hllc", 0.0, "cold")
    ref = oracle_steps(o)
    got, n = gpu_steps(mb, bc, start, [r[0] for r in ref])
    print("cold gas: deferred zones (bulk, shell):", n, "of", zones(dim) * STAGES * STEPS)
    check(got, ref, "cold gas")


# ---- the boundary shell of an overlapped run (host driver) ---------------------------------------------------------
def _shell_run(option, de_switch, lean):
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    import os
    deck = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "inputs", "blast", "blast.in")
    ov = ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=32", "parthenon/mesh/nx3=32", "parthenon/mesh/x3min=-1.0",
          "parthenon/mesh/x3max=1.0", "parthenon/meshblock/nx1=64", "parthenon/meshblock/nx2=32",
          "parthenon/meshblock/nx3=16", "gas/riemann=hllc", "problem/symmetry=spherical", "problem/radius=0.3",
          "problem/samples=0", "parthenon/time/nlim=3", "gas/de_switch=%r" % de_switch]
    option("force_overlap", 1)
    option("lean_energy", 1 if lean else 0)
    option("no_lean_energy", 0 if lean else 1)
    sim = Simulation(deck, ov)
    assert sim.nblocks == 2 and sim.uses_tuned_kernel
    sim.set_overlap(1)
    capi.redo_totals(reset=True)
    sim.evolve()
    assert sim.ncycle == 3 and sim.overlap == 1
    prim = [sim.field("gas.prim", b).copy() for b in range(sim.nblocks)]
    dt = sim.dt
    totals = capi.redo_totals()
    sim.close()
    return prim, dt, totals


@pytest.mark.parametrize("de_switch", [0.4, 0.97])
def test_shell_lists(hiplib, option, de_switch):
    """The blast deck in two blocks along x3, shell launch first and bulk launch behind it (overlap mode 1), lean
    against full: the same primitives in every block and the same dt.  With gas/de_switch = 0.4 nothing is deferred in
    three cycles -- the CPU oracle's thermal share e / (e + v^2 / 2) of this deck stays above 0.93 -- so the run that
    has to show deferred shell zones takes 0.97, which the blast's edge (it crosses the plane between the blocks) falls
    below from the second cycle on."""
    lean, dt_lean, (bulk, shell) = _shell_run(option, de_switch, True)
    full, dt_full, n_full = _shell_run(option, de_switch, False)
    print("de_switch %g: deferred zones bulk %d, shell %d (full kernel: %s)" % (de_switch, bulk, shell, n_full))
    assert dt_lean == dt_full
    for b, (p, q) in enumerate(zip(lean, full)):
        assert np.array_equal(p, q), "block %d" % b
    if de_switch > 0.9:
        assert shell > 0
