"""GPU parity of the two-level flat-wave guards of the tile march.

Every sweep direction of the Cartesian march forms the limiter's verdicts of its slopes first and takes ONE wave-uniform
decision over their conjunction: a wave whose slopes along the direction are all zero -- gas without a gradient along
the sweep -- writes q - 0.0 and q + 0.0 as its face values without a branch or a quotient per slope; any other wave
runs the slopes as before.  The decision is taken in four places: the own x1 and x2 slopes, the two perimeter duties
(partial waves: the decision looks at the duty lanes only), the x3 sweep, and the priming slope of a chunk.  The claim
is the same bits as the CPU oracle in every zone, ghost zones included, after both stages of rk2, whichever side a wave
takes.

The mesh is the smallest on which every one of those decisions can still go wrong: one block of 64 x 16 x 6 zones with
two ghost layers -- two tiles (32 x 8) in x1 and in x2, one chunk with its priming trip, and waves of two rows."""
import os

import numpy as np
import pytest
import torch

from test_parity_fused import fused_step, setup
from test_parity_ops import same

pytestmark = pytest.mark.gpu

TX, TY = 32, 8  # the march's tile
NX = (64, 16, 6)
BCS = {"hllc": "outflow", "hlle": "periodic", "llf": "reflecting"}
AXIS = {1: 3, 2: 2, 3: 1}  # array axis of gprim[var, k, j, i] along sweep direction 1, 2, 3


def _mild(w, rng, shape=None):
    """Random primitives of moderate contrast: no flat variable, no plateau."""
    shp = shape or w[0].shape  # (an axis of length one in `shape` broadcasts; the pressure, w[4], is derived)
    w[0][...] = rng.uniform(0.5, 2.0, shp)
    w[5][...] = rng.uniform(0.5, 2.0, shp)
    for v in (1, 2, 3):
        w[v][...] = rng.normal(0.0, 1.0, shp)


def _flat(w, where):
    """Gas at rest with one density and one energy in the zones `where` (a mask over the block, ghosts included)."""
    w[0][where] = 1.25
    w[5][where] = 0.75
    for v in (1, 2, 3):
        w[v][where] = 0.0


def _one_direction_flat(d):
    """No gradient along direction d (its velocity component included, which is not zero), random across it: the
    direction's decision skips on every wave while the other two directions divide."""
    def make(o, rng):
        shp = list(o.gprim[0].shape)
        shp[AXIS[d] - 1] = 1
        _mild(o.gprim, rng, tuple(shp))
    return make


def _all_flat_but(var):
    """Five variables uniform, `var` random: every conjunction fails on one term only."""
    def make(o, rng):
        w = o.gprim
        _flat(w, np.ones(w[0].shape, bool))
        w[1][...], w[2][...], w[3][...] = 0.3, -0.2, 0.1
        if var in (0, 5):
            w[var] = rng.uniform(0.5, 2.0, w[0].shape)
        else:
            w[var] = rng.normal(0.0, 1.0, w[0].shape)
    return make


def _cut_in_row(i):
    """Flat gas in the columns below interior column i, random gas from there on: the waves of the first tile column
    hold lanes of both kinds, one column either side of the middle of a row included."""
    def make(o, rng):
        _mild(o.gprim, rng)
        m = np.zeros(o.gprim[0].shape, bool)
        m[:, :, :o.is_ + i] = True
        _flat(o.gprim, m)
    return make


def _cut_between_rows(j):
    """Flat gas in the rows below interior row j, random gas above: j = 1 and 3 cut between the two rows of a wave."""
    def make(o, rng):
        _mild(o.gprim, rng)
        m = np.zeros(o.gprim[0].shape, bool)
        m[:, :o.js + j, :] = True
        _flat(o.gprim, m)
    return make


def _perimeter_lines(o):
    """Columns i0 - 1 of the second tile column and i0 + 32 of the first, rows j0 - 1 and j0 + 8 likewise."""
    return (o.is_ + TX - 1, o.is_ + TX), (o.js + TY - 1, o.js + TY)


def _perimeter_rough(o, rng):
    """Flat tile interiors, random values in the perimeter lines only: duty lanes divide, most own waves do not."""
    _mild(o.gprim, rng)
    cols, rows = _perimeter_lines(o)
    m = np.ones(o.gprim[0].shape, bool)
    m[:, :, list(cols)] = False
    m[:, list(rows), :] = False
    _flat(o.gprim, m)


def _perimeter_flat(o, rng):
    """The reverse: random gas in which each perimeter line repeats the line before it, so that the duty lanes' slopes
    along their sweep vanish (with the outflow ghosts: on every duty lane of the first tile) while the own waves divide."""
    _mild(o.gprim, rng)
    cols, rows = _perimeter_lines(o)
    w = o.gprim
    for c in cols:
        w[:, :, :, c] = w[:, :, :, c - 1]
    for r in rows:
        w[:, :, r, :] = w[:, :, r - 1, :]


def _negative_zero(o, rng):
    """Flat gas whose velocities are -0.0 (v1 everywhere, v2 in the upper half of the rows; v3 uniform and not zero, so
    that the zeros are carried through products): a zero slope gives the upper face value -0.0 + 0.0 = +0.0 and the lower
    one -0.0 - 0.0 = -0.0, and so must the flat side."""
    w = o.gprim
    _flat(w, np.ones(w[0].shape, bool))
    w[1][...] = -0.0
    w[2][:, o.js + TY:, :] = -0.0
    w[3][...] = 0.4
    assert np.signbit(w[1]).all()


def _random(o, rng):
    _mild(o.gprim, rng)


def _same_bits(a_gpu, b_np, what):
    """`same` compares values, and -0.0 == +0.0: the sign of a zero is part of the claim here."""
    a = np.ascontiguousarray(a_gpu.cpu().numpy())
    b = np.ascontiguousarray(b_np)
    bad = np.argwhere(a.view(np.int64) != b.view(np.int64))
    assert len(bad) == 0, f"{what}: {len(bad)} values differ in their bits (a zero's sign), first at {bad[0]}"


STATES = {"flat_x1": _one_direction_flat(1), "flat_x2": _one_direction_flat(2), "flat_x3": _one_direction_flat(3),
          "negative_zero": _negative_zero, "perimeter_flat": _perimeter_flat, "perimeter_rough": _perimeter_rough,
          "random": _random}
STATES.update({"all_flat_but_%s" % n: _all_flat_but(v) for n, v in (("d", 0), ("v1", 1), ("v2", 2), ("v3", 3), ("e", 5))})
STATES.update({"cut_in_row_at_%d" % i: _cut_in_row(i) for i in (15, 16, 17)})
STATES.update({"cut_between_rows_at_%d" % j: _cut_between_rows(j) for j in (1, 3)})
FIRST = "flat_x1"
CASES = [("hllc", s) for s in sorted(STATES)] + [("hlle", FIRST), ("llf", FIRST)]


@pytest.mark.parametrize("riem,state", CASES)
def test_two_level_guards_match_oracle(hiplib, riem, state):
    """One rk2 step (both stages through the march) from each constructed state: primitives and conserved state equal
    the oracle's in every zone."""
    bc = (BCS[riem],) * 6
    o, mb, bufs = setup(NX, 2, "plm", riem, bc, seed=17)
    STATES[state](o, np.random.default_rng(31))
    o.ApplyBoundaryConditions()
    o.PrimToCons()
    mb.gas_prim[0].copy_(torch.from_numpy(o.gprim.copy()))
    dt = o.new_dt()
    o.dt = dt
    o.step()
    fused_step(mb, bufs, "rk2", dt, [bc])
    mb.PrimToCons()  # materialise P in the ghosts and the conserved state for comparison
    assert np.isfinite(o.gprim).all(), "the oracle itself left the finite range"
    same(mb.gas_prim[0], o.gprim, "prim after the step")
    same(mb.gas_u0[0], o.gu0, "cons after the step")
    _same_bits(mb.gas_prim[0], o.gprim, "prim after the step")
    _same_bits(mb.gas_u0[0], o.gu0, "cons after the step")


@pytest.mark.parametrize("mode", [1, 2])
def test_two_blocks_shell_first_match_oracle(hiplib, option, mode):
    """Two blocks of 64 x 16 x 6 side by side in x1, stages launched shell first (mode 1: a shell and a bulk launch,
    mode 2: one launch whose shell workgroups run first and signal): three cycles of the blast deck -- gas at rest around
    the blast -- equal the oracle's run of the whole 128 x 16 x 6 mesh."""
    from artemis_amd.driver import Simulation
    from oracle.oracle import Oracle
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    deck = os.path.join(root, "inputs", "blast", "blast.in")
    nx = (2 * NX[0], NX[1], NX[2])
    ov = ["parthenon/mesh/nx1=%d" % nx[0], "parthenon/mesh/nx2=%d" % nx[1], "parthenon/mesh/nx3=%d" % nx[2],
          "parthenon/mesh/x3min=-1.0", "parthenon/mesh/x3max=1.0", "parthenon/meshblock/nx1=%d" % NX[0],
          "parthenon/meshblock/nx2=%d" % NX[1], "parthenon/meshblock/nx3=%d" % NX[2], "gas/riemann=hllc",
          "problem/symmetry=spherical", "problem/radius=0.3", "problem/samples=0", "parthenon/time/nlim=3"]
    o = Oracle(nx, (-1, -1, -1), (1, 1, 1), ng=2, reconstruct="plm", riemann="hllc", gamma=1.4, dfloor=1e-10,
               siefloor=1e-10, cfl=0.3, bc=("outflow",) * 6, integrator="rk2")
    o.pgen_blast(radius=0.3, internal_energy=1.0, p0=1e-5, d0=1.0, samples=0)
    o.evolve(0.1, 3)
    option("force_overlap", 1)  # shell-first launches although every link is local
    s = Simulation(deck, ov)
    try:
        assert s.nblocks == 2 and s.uses_tuned_kernel
        s.set_overlap(mode)
        s.evolve()
        assert s.ncycle == 3 and s.overlap == mode
        assert s.dt == o.dt
        keep = [0, 1, 2, 3, 5]  # the FillGhost variables (the fused stages keep the pressure on interior zones only)
        whole = o.gprim[keep][:, o.ks:o.ke + 1, o.js:o.je + 1, o.is_:o.ie + 1]
        for b in range(2):
            i0 = int(round((s.block_bounds(b)[0] + 1.0) / 2.0 * nx[0]))
            assert i0 in (0, NX[0])
            got = s.interior(s.field("gas.prim", b))[keep]
            assert np.array_equal(got, whole[..., i0:i0 + NX[0]]), (mode, b)
    finally:
        s.close()
