"""GPU tests of Simulation.scatter / load_fields (artemis_sim_scatter_fields): the state of a run set from arrays through
artemis_hip_unpack_fields and completed like a problem generator's.  Only repository code runs here; every comparison is
bitwise.  The same cases on the driver's host loop, and on several ranks, are tests/test_scatter_cpu.py; the kernel alone is
tests/test_scatter.py."""
import os

import numpy as np
import pytest

import amr_cases
from test_fields import BLAST32, SHIPPED
from test_outputs_cpu import blast

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = lambda *p: os.path.join(ROOT, "inputs", *p)

PRIM = ["gas.prim.density", "gas.prim.velocity", "gas.prim.sie"]
CONS = ["gas.cons.density", "gas.cons.momentum", "gas.cons.total_energy", "gas.cons.internal_energy"]
DUST = ["dust.prim.density", "dust.prim.velocity"]

BLAST2D = (("blast", "blast.in"), blast()["overrides"], "problem/radius=0.2", True)
BLAST3D = (("blast", "blast.in"),
           ["parthenon/mesh/nx1=16", "parthenon/mesh/nx2=16", "parthenon/mesh/nx3=16", "parthenon/mesh/x3min=-1.0",
            "parthenon/mesh/x3max=1.0", "parthenon/meshblock/nx1=16", "parthenon/meshblock/nx2=16", "parthenon/meshblock/nx3=8",
            "gas/riemann=hllc", "problem/symmetry=spherical", "problem/radius=0.3", "problem/samples=0", "parthenon/time/nlim=40"],
           "problem/radius=0.2", True)
ADVECTION = (("advection", "advection.in"),
             ["parthenon/mesh/nx1=16", "parthenon/mesh/nx2=8", "parthenon/mesh/nx3=8", "parthenon/meshblock/nx1=8",
              "parthenon/meshblock/nx2=8", "parthenon/meshblock/nx3=8"], "problem/amp=2.0e-3", False)


def sim(case, *extra):
    from artemis_amd.driver import Simulation
    return Simulation(DECK(*case[0]), list(case[1]) + list(extra))


def interiors(s):
    out = [np.stack([s.interior(s.field("gas.prim", b)) for b in range(s.nblocks)])]
    if s.ns_dust:
        out.append(np.stack([s.interior(s.field("dust.prim", b)) for b in range(s.nblocks)]))
    return out


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(interiors(a), interiors(b)))


def in_step(a, b, cycles, clock=True):
    """a and b take `cycles` cycles one at a time: the same kernel, dt and (clock) time, the same interiors after each"""
    for _ in range(cycles):
        assert a.evolve(1) == 1 and b.evolve(1) == 1
        assert a.dt == b.dt and a.stage_kernel == b.stage_kernel and (a.time == b.time or not clock)
        assert same_state(a, b), a.ncycle


@pytest.mark.parametrize("case", [BLAST2D, BLAST3D, ADVECTION], ids=["blast2d", "blast3d_tuned", "advection_dust"])
def test_scatter_reproduces_a_problem_generator(hiplib, case):
    """Run A at cycle 0; run B, the same deck with another problem parameter, given A's primitives: A's dt, then A's cycles.
    The 3-D blast runs the tuned kernel, and after the five single cycles both take six more in one call, the last of them
    as replays of a captured graph."""
    a, b = sim(case), sim(case, case[2])
    names = PRIM + (DUST if a.ns_dust else [])
    a.evolve(0), b.evolve(0)
    assert not same_state(a, b) and a.uses_tuned_kernel == case[3] == b.uses_tuned_kernel
    b.scatter(names, a.gather(names))
    assert same_state(a, b) and b.dt == a.dt and (b.time, b.ncycle) == (0.0, 0)
    in_step(a, b, 5)
    if case is BLAST3D:
        assert a.nblocks == 2 and a.evolve(6) == 6 and b.evolve(6) == 6
        assert (a.time, a.dt, a.stage_kernel) == (b.time, b.dt, b.stage_kernel) and same_state(a, b)
    a.close(), b.close()


@pytest.mark.parametrize("case", [BLAST2D, BLAST3D], ids=["blast2d", "blast3d_tuned"])
def test_scatter_in_the_middle_of_a_run(hiplib, case):
    """C scatters, after three cycles, the state it already holds (B's, an identical run): the ghost fill and the flags
    about ghost zones start from a ping-pong buffer other than 0.  C's interiors then equal B's, and its next three cycles
    are those of a fresh run D given the same arrays and time.  C's clock is NOT that of a run A that takes six cycles
    without a scatter: the dt after a scatter is a fresh estimate, without the "at most doubles" rule that still holds A's
    dt back at cycle 3 of a blast; that is by construction and not asserted."""
    b, c, d = sim(case), sim(case), sim(case)
    assert b.evolve(3) == 3 and c.evolve(3) == 3
    g = b.gather(PRIM)
    c.scatter(PRIM, g, time=b.time)
    assert same_state(b, c) and c.time == b.time and c.ncycle == 3
    d.scatter(PRIM, g, time=b.time)
    assert (d.time, d.dt, d.ncycle) == (c.time, c.dt, 0) and same_state(c, d)
    in_step(c, d, 3)
    b.close(), c.close(), d.close()


def test_the_conserved_route_is_consistent(hiplib):
    """B takes A's conserved variables, C the primitives B then shows: the same state, and the same three cycles.  (B is
    not A bit for bit: E - rho v^2 / 2 formed from the momenta rounds differently from the sie A holds.)"""
    a, b, c = sim(BLAST3D), sim(BLAST3D, "problem/radius=0.2"), sim(BLAST3D, "problem/radius=0.25")
    a.evolve(2)
    b.scatter(CONS, a.gather(CONS))
    assert np.array_equal(interiors(a)[0][:, 0], interiors(b)[0][:, 0])  # (the density is)
    c.scatter(PRIM, b.gather(PRIM))
    assert same_state(b, c) and b.dt == c.dt
    in_step(b, c, 3)
    a.close(), b.close(), c.close()


def test_refined_mesh_round_trip_through_a_dump(hiplib, tmp_path):
    """blast_amr.in at its test size (cylindrical, three levels): write_fields, load_fields into a fresh run of the same deck,
    then three identical cycles, dt included; a run whose mesh has other leaves refuses, naming a block."""
    from artemis_amd.driver import Simulation
    case = amr_cases.blast_amr()
    a, b = Simulation(DECK(*case["deck"]), case["overrides"]), Simulation(DECK(*case["deck"]), case["overrides"])
    x = Simulation(DECK(*case["deck"]), case["overrides"] + ["parthenon/mesh/numlevel=2"])
    assert len({a.block_level(q) for q in range(a.nblocks)}) >= 2
    a.write_fields(tmp_path / "amr.fld", PRIM)
    with pytest.raises(ValueError, match=r"holds no block on level \d with the bounds \["):
        x.load_fields(tmp_path / "amr.fld")
    assert b.load_fields(tmp_path / "amr.fld") == PRIM
    assert same_state(a, b) and b.time == a.time == 0.0
    for _ in range(3):
        assert a.evolve(1) == 1 and b.evolve(1) == 1
        assert (a.time, a.dt, a.stage_kernel, a.nblocks) == (b.time, b.dt, b.stage_kernel, b.nblocks) and same_state(a, b)
    a.close(), b.close(), x.close()


def test_gather_after_scatter_is_undisturbed(hiplib):
    """32^3 blast in eight 16^3 blocks on the tuned kernel.  B takes A's state through a 1 MiB staging buffer (blocks of 160
    KiB: two block ranges), C in one piece and in float32 widened by the caller; then gather and field() agree on B, pressure
    included, and a B that gathers takes the steps of a C that does not."""
    from artemis_amd import capi
    from artemis_amd.driver import Simulation
    ov = BLAST32 + ["parthenon/time/nlim=8"]
    a, b, c = (Simulation(DECK("blast", "blast.in"), ov + extra) for extra in ([], ["problem/radius=0.2"], ["problem/radius=0.2"]))
    a.evolve(2)
    g = a.gather(PRIM)
    assert g.shape == (8, 5, 16, 16, 16) and g.nbytes > (1 << 20)
    with capi.option("fields_stage_mb", 1):
        b.scatter(PRIM, g)
    c.scatter(PRIM, g)
    assert same_state(a, b) and same_state(b, c) and b.dt == c.dt

    def gathered_equals_field(s):
        want = np.stack([s.interior(s.field("gas.prim", q)) for q in range(s.nblocks)])
        got = s.gather(SHIPPED)
        return np.array_equal(got, want[:, 0:5]) and want[:, 4].min() > 0.0

    b.evolve(3), c.evolve(3)
    shipped = b.gather(SHIPPED)  # (before anything has materialised B's conserved state)
    b.evolve(), c.evolve()
    assert (b.time, b.dt, b.ncycle, b.stage_kernel) == (c.time, c.dt, 8, "stage_fused_kernel") == (c.time, c.dt, c.ncycle, c.stage_kernel)
    assert same_state(b, c) and gathered_equals_field(b) and shipped.shape == (8, 5, 16, 16, 16)
    # float32 input is widened exactly: the run that takes it equals one given the widened doubles
    g32 = g.astype(np.float32)
    b.scatter(PRIM, g32, time=0.5), c.scatter(PRIM, g32.astype(np.float64), time=0.5)
    assert same_state(b, c) and (b.time, b.dt) == (0.5, c.dt) and gathered_equals_field(b)
    with pytest.raises(RuntimeError, match="mix the primitive and the conserved form"):
        b.scatter(["gas.prim.density", "gas.prim.velocity", "gas.cons.total_energy"], g)
    with pytest.raises(ValueError, match="the array is"):
        b.scatter(PRIM, g[:, :4].copy())
    a.close(), b.close(), c.close()
