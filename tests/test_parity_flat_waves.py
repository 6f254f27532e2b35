"""GPU parity of the tile march's flat-wave guards.

The Cartesian march skips, wave by wave, work whose result the whole wave discards: the quotient of the van-Leer slope
where the limiter zeroes it on every lane (device_math.hpp plm_dqm_fast_skip), and HLLC's shock corrections where the
interface pressure exceeds neither state's on any lane (hllc_gas_fast_skip).  Both sides of a guard keep the expression
trees, so the claim is: the same bits as the CPU oracle in every zone, ghost zones included, whatever side a wave takes.
The states below are built to put waves on every side.  A tile is 32 x 8 zones and a wave two rows of 32; the perimeter
duties (the slopes of columns i0 - 1, i0 + 32 and rows j0 - 1, j0 + 8) run on partial waves with guards of their own.
Densities and energies of the constructed states stay within a factor of a few of one; the blast deck's ambient energy
of 2.5e-5 is still five decades above the floors of 1e-10."""
import numpy as np
import pytest
import torch

from test_parity_fused import fused_step, setup
from test_parity_ops import same

pytestmark = pytest.mark.gpu

TX, TY = 32, 8  # the march's tile


def _flat(w, where):
    """Gas at rest with one density and one energy in the zones `where` (a mask over the block, ghosts included)."""
    w[0][where] = 1.25
    w[5][where] = 0.75
    for v in (1, 2, 3):
        w[v][where] = 0.0


def _mild(o, rng):
    """Random primitives of moderate contrast in every zone: no flat variable, no plateau."""
    shp = o.gprim[0].shape
    w = o.gprim
    w[0] = rng.uniform(0.5, 2.0, shp)
    w[5] = rng.uniform(0.5, 2.0, shp)
    for v in (1, 2, 3):
        w[v] = rng.normal(0.0, 1.0, shp)


def _rest(o, rng):
    _flat(o.gprim, np.ones(o.gprim[0].shape, bool))


def _flat_variables(o, rng):
    """Random, but v3 = 0 and one density everywhere: two of the six slopes of every sweep are flat on every lane."""
    _mild(o, rng)
    o.gprim[3][...] = 0.0
    o.gprim[0][...] = 1.5


def _split_mid_row(o, rng):
    """Flat gas left of a line through the middle of the first tile's rows, random gas right of it: every wave of that
    tile column holds lanes of both kinds."""
    _mild(o, rng)
    m = np.zeros(o.gprim[0].shape, bool)
    m[:, :, :o.is_ + TX // 2] = True
    _flat(o.gprim, m)


def _split_between_rows(o, rng):
    """Flat gas below a line between tile rows 2 and 3 -- the two rows of one wave -- random gas above it."""
    _mild(o, rng)
    m = np.zeros(o.gprim[0].shape, bool)
    m[:, :o.js + 3, :] = True
    _flat(o.gprim, m)


def _perimeter_lines(o):
    """The perimeter columns / rows of tile (1, 1): i0 - 1, i0 + 32, j0 - 1, j0 + 8 (all inside the block)."""
    cols = [c for c in (o.is_ + TX - 1, o.is_ + 2 * TX) if c <= o.ie]
    rows = [r for r in (o.js + TY - 1, o.js + 2 * TY) if r <= o.je]
    assert cols and rows
    return cols, rows


def _perimeter_rough(o, rng):
    """Flat gas in the tile interiors, random values only in the perimeter columns and rows of tile (1, 1): its duty
    lanes divide while its own waves do not (and its neighbours hold the rough lines inside their tiles)."""
    _mild(o, rng)
    cols, rows = _perimeter_lines(o)
    m = np.ones(o.gprim[0].shape, bool)
    m[:, :, cols] = False
    m[:, rows, :] = False
    _flat(o.gprim, m)


def _perimeter_flat(o, rng):
    """The reverse: random gas, with each perimeter column / row of tile (1, 1) a copy of the line before it, so that
    the duty lanes' slopes along the sweep vanish while the tile's own waves divide."""
    _mild(o, rng)
    cols, rows = _perimeter_lines(o)
    w = o.gprim
    for c in cols:
        w[:, :, :, c] = w[:, :, :, c - 1]
    for r in rows:  # (at a crossing the zone then equals its neighbour of either direction)
        w[:, :, r, :] = w[:, :, r - 1, :]


def _pressure_jumps(o, rng):
    """HLLC's guard on every side.  In the first tile row (3-D; the first tile column in 2-D) the state is piecewise
    constant along the march (along x2 in 2-D) in pairs of planes, random across them, and the velocity along that axis
    drops by 1 from pair to pair.  A face inside a pair has equal states: pmid == p on every lane, both corrections
    skipped by the whole wave.  A face between pairs is compressed: with densities and energies within 10 % of one,
    (vl - vr) * rc_avg >= 0.45 exceeds any pressure difference (<= 0.16), so pmid exceeds both pressures on every lane
    -- and in 3-D the 64 faces of a wave's x3 sweep lie in one plane.  Elsewhere the gas is random: mixed waves, as in
    the sweeps across the pairs."""
    _mild(o, rng)
    w = o.gprim
    if o.ndim == 3:
        a, vel = w[:, :, :o.js + TY, :], 3           # (views: axis 1 runs along the pairs)
    else:
        a, vel = np.swapaxes(w[:, :, :, :o.is_ + TX], 1, 2), 2
    a[0] = 0.9 + 0.2 * (a[0] - 0.5) / 1.5
    a[5] = 0.9 + 0.2 * (a[5] - 0.5) / 1.5
    n = a.shape[1]
    for m in range(0, n - 1, 2):
        a[:, m + 1] = a[:, m]
    for m in range(n):
        a[vel, m] = 1.0 * (n // 4 - m // 2)


STATES = {"rest": _rest, "flat_variables": _flat_variables, "split_mid_row": _split_mid_row,
          "split_between_rows": _split_between_rows, "perimeter_rough": _perimeter_rough,
          "perimeter_flat": _perimeter_flat, "pressure_jumps": _pressure_jumps}
BCS = {"hllc": "outflow", "hlle": "periodic", "llf": "reflecting"}
SHAPES = {"3d": (72, 20, 36), "2d": (72, 20, 1)}  # ragged tiles in x1 and x2; tile (1, 1) has all four perimeter lines


def _run(o, mb, bufs, bc, steps):
    for step in range(steps):
        dt = o.new_dt()
        o.dt = dt
        o.step()
        fused_step(mb, bufs, "rk2", dt, [bc])
        mb.PrimToCons()  # materialise P in the ghosts and the conserved state for comparison
        assert np.isfinite(o.gprim).all(), "the oracle itself left the finite range"
        same(mb.gas_prim[0], o.gprim, f"prim after step {step}")
        same(mb.gas_u0[0], o.gu0, f"cons after step {step}")


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("dim", sorted(SHAPES))
@pytest.mark.parametrize("riem", sorted(BCS))
def test_flat_wave_guards_match_oracle(hiplib, riem, dim, state):
    """Two rk2 steps from each constructed state: primitives and conserved state equal the oracle's in every zone."""
    bc = (BCS[riem],) * 6
    o, mb, bufs = setup(SHAPES[dim], 2, "plm", riem, bc, seed=17)
    STATES[state](o, np.random.default_rng(29))
    o.ApplyBoundaryConditions()
    o.PrimToCons()
    mb.gas_prim[0].copy_(torch.from_numpy(o.gprim.copy()))
    _run(o, mb, bufs, bc, 2)


@pytest.mark.parametrize("dim", sorted(SHAPES))
@pytest.mark.parametrize("riem", sorted(BCS))
def test_flat_wave_guards_blast(hiplib, riem, dim):
    """The blast deck has all of it at once -- ambient gas at rest, the shock, the rarefaction behind it: four steps."""
    bc = ("outflow",) * 6
    o, mb, bufs = setup(SHAPES[dim], 2, "plm", riem, bc, seed=0, blast=True)
    _run(o, mb, bufs, bc, 4)
