"""The CPU oracle against the reference's own headers, bit for bit.

oracle/_ref/libartemis_ref.so (oracle/ref/ref_leaves.cpp, built by `make -C oracle` where the reference's source tree
is present) compiles the reference's unmodified artemis.hpp, geometry/geometry.hpp, utils/fluxes/reconstruction/
reconstruction.hpp and utils/fluxes/riemann/riemann.hpp with the oracle's compiler, flags and libm.  Every test here
feeds both sides the same doubles and compares BIT PATTERNS (so -0.0 and NaN payloads count): tables of the scalar
reconstructions and of single Riemann faces with the edges constructed to reach every branch, geometry::Coords on
every cell of a block, and whole flux sweeps through Reconstruction<>::apply and RiemannSolver<>::solve.  Branch
coverage is asserted from the reference's outputs (and the inputs), never from the oracle's.
"""
import functools

import numpy as np
import pytest

from oracle import reference as ref
from oracle.oracle import COORDS, Oracle
from test_parity_ops import face_slices, random_state

GAS, DUST = 0, 1
GM1 = (1.0e-6, 0.4, 2.0 / 3.0)
PAIRS = [(GAS, "hllc"), (GAS, "hlle"), (GAS, "llf"), (DUST, "hlle"), (DUST, "llf")]


@pytest.fixture(autouse=True)
def _library():
    ref.need()  # skips only where there is neither a library, nor a reference tree, nor a GPU; fails if it is missing


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(want, got, what):
    w, g = bits(want), bits(got)
    assert w.shape == g.shape, what
    if not np.array_equal(w, g):
        bad = np.argwhere(w != g)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {w.size} values differ in bits, first at {first}: "
                             f"reference {np.asarray(want)[first]!r}, oracle {np.asarray(got)[first]!r}")


# ---------------------------------------------------------------------------------------------------------------------
# scalar reconstructions
def random_stencils(rng, n, width):
    """n stencils of `width` values over 10 decades of scale: a third unrelated values of both signs, a third a
    monotone run with random steps (the limiter's smooth side), a third a small ripple on a large offset (cancellation
    in the differences)."""
    scale = 10.0 ** rng.uniform(-5.0, 5.0, n)
    a = rng.normal(0.0, 1.0, (width, n))
    b = np.cumsum(rng.uniform(0.0, 1.0, (width, n)) ** 3, axis=0) * rng.choice([-1.0, 1.0], n)
    c = 1.0 + 1.0e-9 * rng.normal(0.0, 1.0, (width, n))
    kind = rng.integers(0, 3, n)
    return np.where(kind == 0, a, np.where(kind == 1, b, c)) * scale


SUB = 5e-324  # the smallest subnormal
PLM_EDGES = np.array([
    (1.0, 1.0, 1.0), (-3.5, -3.5, -3.5), (0.0, 0.0, 0.0),          # all equal
    (1.0, 1.0, 2.0), (1.0, 2.0, 2.0), (-1.0, -1.0, 5.0),           # dq2 == 0 from either side
    (1.0, 2.0, 1.0), (3.0, -1.0, 3.0), (1e-3, 1e3, 1e-3),          # dql == -dqr: dq2 / 0
    (1.0, 2.0, 1.5), (-1.0, 1.0, -2.0), (2.0, 1.0, 3.0),           # a sign change of the slope
    (-1.0, 0.5, 2.0), (2.0, -0.5, -1.0),                           # monotone through zero
    (1.0, 1e12, 2e12), (1.0, 2.0, 1e12), (1e-12, 1.0, 2.0), (1e-12, 2e-12, 1.0),  # monotone, contrast 1e+-12
    (1.0, 1.0 + 1e-12, 1.0 + 3e-12), (2e12, 1e12, 1.0), (1.0, 1.0 - 2 ** -53, 1.0 - 2 ** -52),
    (SUB, 2 * SUB, 3 * SUB), (0.0, SUB, 2 * SUB), (1e-310, 2e-310, 4e-310), (-SUB, 0.0, SUB),  # subnormal
    (1e-200, 2e-200, 3e-200),                                      # dq2 underflows to 0 though the slopes agree
    (-0.0, -0.0, -0.0), (-0.0, 0.0, 0.0), (0.0, -0.0, 1.0), (-1.0, -0.0, 0.0), (0.0, 0.0, -0.0), (-0.0, 0.0, -0.0),
    (-1e308, 0.0, 1e308), (1e308, -1e308, 1e308), (1e200, 2e200, 4e200),  # dq2 overflows
], dtype=np.float64).T


@functools.lru_cache(maxsize=None)
def plm_table():
    rng = np.random.default_rng(2024)
    return np.concatenate([random_stencils(rng, 100000, 3), PLM_EDGES], axis=1)


def test_plm_table():
    """ArtemisUtils::PLM (plm.hpp:32-47).  Reached, by the reference's outputs: zeroed slopes and kept slopes."""
    qm, q, qp = plm_table()
    rl, rr = ref.plm(qm, q, qp)
    flat = (rl == q) & (rr == q)
    assert flat[-PLM_EDGES.shape[1]:].sum() >= 20 and flat[:100000].any() and (~flat[:100000]).any()
    assert (~flat[-PLM_EDGES.shape[1]:]).any()
    ol, orr = ref.oracle_plm(qm, q, qp)
    same_bits(rl, ol, "PLM ql(i+1)")
    same_bits(rr, orr, "PLM qr(i)")


PPM_EDGES = np.array([
    (1.0, 1.0, 1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0), (-0.0, -0.0, -0.0, -0.0, -0.0),   # all equal
    (0.0, 1.0, 2.0, 1.0, 0.0), (3.0, 1.0, 0.0, 1.0, 3.0), (0.0, 0.0, 1.0, 0.0, 0.0),       # an extremum at q_i
    (1.0, 2.0, 2.0, 3.0, 4.0), (1.0, 2.0, 3.0, 3.0, 4.0),                                   # qd == 0, qc == 0
    (1.0, 2.0, 3.0, 4.0, 5.0), (5.0, 4.0, 3.0, 2.0, 1.0), (-2.0, -1.0, 0.0, 1.0, 2.0),     # a straight line: untouched
    (0.0, 1.0, 4.0, 9.0, 16.0), (16.0, 9.0, 4.0, 1.0, 0.0),                                 # a parabola
    (0.0, 0.0, 0.1, 1.0, 1.0), (1.0, 1.0, 0.9, 0.0, 0.0),       # |qc| >= 2|qd|: the right value is steepened
    (1.0, 1.0, 0.1, 0.0, 0.0), (0.0, 0.0, 0.9, 1.0, 1.0),       # |qd| >= 2|qc|: the left value is steepened
    (20.0, 0.0, 1.0, 2.0, 3.0), (3.0, 2.0, 1.0, 0.0, 20.0), (-20.0, 0.0, 1.0, 2.0, 30.0),  # CS eqn 13 clamps
    (1.0, 1e12, 2e12, 3e12, 4e12), (1e-12, 1.0, 2.0, 3.0, 1e12), (4e12, 3e12, 2e12, 1e12, 1.0),
    (SUB, 2 * SUB, 3 * SUB, 4 * SUB, 5 * SUB), (1e-310, 2e-310, 3e-310, 5e-310, 6e-310), (-SUB, -0.0, 0.0, SUB, SUB),
    (-0.0, 0.0, -0.0, 0.0, -0.0), (-1.0, -0.0, 0.0, -0.0, 1.0), (0.0, -0.0, 0.0, 1.0, 2.0),
    (-1e308, -1e307, 0.0, 1e307, 1e308), (1e308, 1e308, 1e308, 1e308, 1e308), (1e200, 2e200, 3e200, 4e200, 6e200),
], dtype=np.float64).T


@functools.lru_cache(maxsize=None)
def ppm_table():
    rng = np.random.default_rng(2025)
    return np.concatenate([random_stencils(rng, 100000, 5), PPM_EDGES], axis=1)


def test_ppm4_table():
    """ArtemisUtils::PPM4 (ppm.hpp:33-66).  Every branch is reached, judged by the reference's outputs alone: a
    flattened cell returns q on both sides (:50-52); a steepened side is exactly q - 2 (other side - q) (:54-59);
    the rest leave both interpolated values, some of them clamped to a neighbour (:42-45)."""
    qmm, qm, q, qp, qpp = ppm_table()
    rl, rr = ref.ppm4(qmm, qm, q, qp, qpp)  # rl = ql(i+1) = qrv, rr = qr(i) = qlv
    fin = np.isfinite(rl) & np.isfinite(rr)
    flat = fin & (rl == q) & (rr == q)
    with np.errstate(all="ignore"):
        steep_r = fin & ~flat & (rl == q - 2.0 * (rr - q))
        steep_l = fin & ~flat & (rr == q - 2.0 * (rl - q))
    plain = fin & ~flat & ~steep_r & ~steep_l
    clamp_l = plain & (rr == qm)
    clamp_r = plain & (rl == qp)
    for name, hit in (("flattened", flat), ("right steepened", steep_r), ("left steepened", steep_l),
                      ("untouched", plain), ("left clamp", clamp_l), ("right clamp", clamp_r)):
        assert hit.any(), f"no stencil of the table reaches the branch: {name}"
    edges = slice(-PPM_EDGES.shape[1], None)
    assert flat[edges].sum() >= 8 and steep_r[edges].any() and steep_l[edges].any() and plain[edges].any()
    ol, orr = ref.oracle_ppm4(qmm, qm, q, qp, qpp)
    same_bits(rl, ol, "PPM4 ql(i+1)")
    same_bits(rr, orr, "PPM4 qr(i)")


def plm_g_rows():
    """Positions PLM_G receives (plm.hpp:93-101, :127-135) along x1 and x2 rows of a spherical and a cylindrical mesh
    whose first cell's inner face lies at r = 0.1 dx, all from the reference's own Coords: (xm, xc, xp, xf0, xf1, dx)."""
    rows = []
    n1, n2 = 34, 18
    dx1 = 1.0 / 32
    for system, x2lo, dx2 in ((COORDS["spherical3D"], 0.3, 2.5 / n2), (COORDS["cylindrical"], 0.0, 2 * np.pi / n2)):
        geom = np.array([0.1 * dx1, dx1, x2lo, dx2, 0.0, 0.25])
        i = np.arange(n1)
        c = ref.coords(system, geom, 0, 3, i)                  # an x1 row
        xv, w = c[:, ref.COORD_NAMES.index("x1v")], c[:, ref.COORD_NAMES.index("WidthX1")]
        xf = geom[0] + np.arange(n1 + 1) * geom[1]              # Coordinates_t::Xf
        rows.append(np.stack([xv[:-2], xv[1:-1], xv[2:], xf[1:-2], xf[2:-1], w[1:-1]]))
        j = np.arange(n2)
        for i0 in (0, 7):                                       # x2 rows: next to the axis and further out
            c = ref.coords(system, geom, 0, j, i0)
            xv, w = c[:, ref.COORD_NAMES.index("x2v")], c[:, ref.COORD_NAMES.index("WidthX2")]
            xf = geom[2] + np.arange(n2 + 1) * geom[3]
            rows.append(np.stack([xv[:-2], xv[1:-1], xv[2:], xf[1:-2], xf[2:-1], w[1:-1]]))
    return np.concatenate(rows, axis=1)


def test_plm_g_table():
    """ArtemisUtils::PLM_G (plm.hpp:54-73) with the centroids, faces and widths of the reference's Coords."""
    pos = plm_g_rows()
    assert 0.1 / 32 < pos[0].min() < 1.1 / 32 and np.all(np.diff(pos[:3], axis=0) > 0)  # (the cell next to r = 0.1 dx)
    rng = np.random.default_rng(2026)
    q = plm_table()
    # every edge stencil at every position, then the random stencils at random positions
    ne, npos = PLM_EDGES.shape[1], pos.shape[1]
    qe = np.repeat(PLM_EDGES, npos, axis=1)
    pe = np.tile(pos, (1, ne))
    pick = rng.integers(0, npos, 100000)
    qs = np.concatenate([q[:, :100000], qe], axis=1)
    ps = np.concatenate([pos[:, pick], pe], axis=1)
    rl, rr = ref.plm_g(*qs, *ps)
    flat = (rl == qs[1]) & (rr == qs[1])
    assert flat.any() and (~flat).any()
    ol, orr = ref.oracle_plm_g(*qs, *ps)
    same_bits(rl, ol, "PLM_G ql(i+1)")
    same_bits(rr, orr, "PLM_G qr(i)")


# ---------------------------------------------------------------------------------------------------------------------
# single Riemann faces
def state(rho, vx, p, vy=0.3, vz=-0.2, sie=1.5):
    return (rho, vx, vy, vz, p, sie)


def constructed_pairs(gm1):
    """Named groups of (left, right) gas states [rho, vx, vy, vz, P, sie] that reach each branch of the solvers."""
    gamma = gm1 + 1.0
    c = np.sqrt(gamma * 1.0 / 1.0)  # sound speed of rho = p = 1
    g = {}
    g["rest"] = [(state(r, 0.0, p, 0.0, 0.0), state(r, 0.0, p, 0.0, 0.0)) for r, p in ((1.0, 1.0), (1e-8, 3.0), (7.0, 1e8))]
    g["rest"] += [(state(1.0, 0.0, 1.0), state(1.0, 0.0, 1.0)), (state(2.0, -0.0, 1.0), state(2.0, -0.0, 1.0)),
                  (state(2.0, 0.0, 1.0), state(2.0, -0.0, 1.0)), (state(2.0, -0.0, 1.0), state(2.0, 0.0, 1.0))]
    g["mirror"] = [(state(r, u, p), state(r, -u, p)) for r, p in ((1.0, 1.0), (3.0, 0.1), (1e-4, 20.0))
                   for u in (0.5, -0.5, 0.01 * c, -0.01 * c, 3.0 * c)]
    g["rarefaction"] = [(state(1.0, -20.0 * c, 1.0), state(1.0, 20.0 * c, 1.0)),
                        (state(4.0, -20.0 * c, 4.0), state(4.0, 20.0 * c, 4.0))]
    g["supersonic_right"] = [(state(1.0, 5.0 * c, 1.0), state(1.0, 5.0 * c, 1.0)),
                             (state(1.0, 5.0 * c, 1.0), state(0.5, 7.0 * c, 0.8)),
                             (state(2.0, 30.0 * c, 1.0), state(1.0, 25.0 * c, 2.0))]
    g["supersonic_left"] = [(state(r[0], -r[1], r[4]), state(l[0], -l[1], l[4])) for l, r in g["supersonic_right"]]
    # qd (the PVRS middle pressure, hllc.hpp:107) against the side pressures (:110-113)
    g["qd_above_both"] = [(state(1.0, 2.0, 1.0), state(1.0, -2.0, 1.0)), (state(1.0, 1.0, 1.0), state(2.0, -1.5, 1.2))]
    g["qd_below_both"] = [(state(1.0, -0.5, 1.0), state(1.0, 0.5, 1.0)), (state(1.0, -0.2, 1.0), state(2.0, 0.4, 1.2))]
    g["qd_above_right_only"] = [(state(1.0, 0.0, 1000.0), state(1.0, 0.0, 1.0)), (state(3.0, 0.1, 50.0), state(1.0, 0.1, 0.5))]
    g["qd_above_left_only"] = [(state(1.0, 0.0, 1.0), state(1.0, 0.0, 1000.0)), (state(1.0, -0.1, 0.5), state(3.0, -0.1, 50.0))]
    g["contrast"] = [(state(a, u, b), state(1.0, -u, 1.0)) for a in (1e8, 1e-8) for b in (1e8, 1e-8) for u in (0.0, 0.7)]
    g["contrast"] += [(state(1.0, u, 1.0), state(a, u, b)) for a in (1e8, 1e-8) for b in (1e8, 1e-8) for u in (0.0, -0.7)]
    tiny = (1e-310, -1e-310, -0.0, 0.0, SUB, 1e-250)
    g["vanishing"] = [(state(1.0, a, 1.0, b, -a), state(1.3, b, 0.9, a, -0.0)) for a in tiny for b in tiny]
    return g


def riemann_table(fluid, gm1):
    rng = np.random.default_rng(77)
    n = 20000
    w = np.empty((2, n, 6))
    for s in range(2):
        w[s, :, 0] = 10.0 ** rng.uniform(-3, 3, n)
        w[s, :, 4] = 10.0 ** rng.uniform(-3, 3, n)
        w[s, :, 1:4] = rng.normal(0.0, 1.0, (n, 3)) * (10.0 ** rng.uniform(-2, 1.5, (n, 1)))
        w[s, :, 5] = 10.0 ** rng.uniform(-3, 3, n)
    w[1, : n // 4, 0] = w[0, : n // 4, 0] * (1.0 + 1e-3 * rng.normal(size=n // 4))  # weak jumps too
    w[1, : n // 4, 4] = w[0, : n // 4, 4] * (1.0 + 1e-3 * rng.normal(size=n // 4))
    groups, lo = {}, n
    left, right = [w[0]], [w[1]]
    for name, pairs in constructed_pairs(gm1).items():
        left.append(np.array([p[0] for p in pairs])), right.append(np.array([p[1] for p in pairs]))
        groups[name] = slice(lo, lo + len(pairs))
        lo += len(pairs)
    wl, wr = np.concatenate(left), np.concatenate(right)
    if fluid == DUST:
        wl, wr = wl[:, :4].copy(), wr[:, :4].copy()
    return wl, wr, groups


@pytest.mark.parametrize("gm1", GM1)
@pytest.mark.parametrize("fluid,solver", PAIRS)
def test_riemann_table(fluid, solver, gm1):
    """RiemannSolver<solver, fluid>::solve (hllc.hpp, hlle.hpp, llf.hpp) through the class, one face at a time."""
    wl, wr, grp = riemann_table(fluid, gm1)
    r = ref.riemann(fluid, solver, gm1, wl, wr)
    frho, pf, vf = r[:, 0], r[:, 6], r[:, 7]
    gamma = gm1 + 1.0
    # --- which branches the table reached, from the reference's outputs ---
    if fluid == GAS:
        # equal states at rest: frho == 0 exactly, the upwind select (frho >= 0) falls on the left state
        assert np.all(frho[grp["rest"]] == 0.0) and np.all(vf[grp["rest"]] == 0.0) and np.all(r[grp["rest"], 5] == 0.0)
        assert np.allclose(pf[grp["rest"]], wl[grp["rest"], 4], rtol=1e-14, atol=0)
    if solver == "hllc":
        # frho carries the sign of the contact speed am (hllc.hpp:157-171): both branches, and am == 0 on mirror states
        assert (frho[:20000] > 0).sum() > 1000 and (frho[:20000] < 0).sum() > 1000
        assert np.all(frho[grp["mirror"]] == 0.0) and np.all(wl[grp["mirror"], 1] != 0.0)
        # cp clamped to 0 (:138): with am == 0 the face pressure is cp itself
        assert np.all(pf[grp["rarefaction"]] == 0.0)
        # the table holds the PVRS middle pressure qd (:105-107) on either side of each state's pressure (:110-113);
        # a statement about the inputs, with margins far above rounding
        qd = 0.5 * (wl[:, 4] + wr[:, 4] + (wl[:, 1] - wr[:, 1]) * 0.25 * (wl[:, 0] + wr[:, 0])
                    * (np.sqrt(gamma * wl[:, 4] / wl[:, 0]) + np.sqrt(gamma * wr[:, 4] / wr[:, 0])))
        for name, above_l, above_r in (("qd_above_both", True, True), ("qd_below_both", False, False),
                                       ("qd_above_right_only", False, True), ("qd_above_left_only", True, False)):
            g = grp[name]
            assert np.all((qd[g] > 1.01 * wl[g, 4]) if above_l else (qd[g] < 0.99 * wl[g, 4])), name
            assert np.all((qd[g] > 1.01 * wr[g, 4]) if above_r else (qd[g] < 0.99 * wr[g, 4])), name
    if solver in ("hllc", "hlle"):
        # supersonic to the right: bm = -1e-20 (hllc.hpp:122, hlle.hpp:172), the flux is the left state's; and mirrored
        R, L = grp["supersonic_right"], grp["supersonic_left"]
        assert np.allclose(frho[R], wl[R, 0] * wl[R, 1], rtol=1e-12, atol=0) and np.all(frho[R] > 0)
        assert np.allclose(frho[L], wr[L, 0] * wr[L, 1], rtol=1e-12, atol=0) and np.all(frho[L] < 0)
        if fluid == GAS:
            assert np.allclose(pf[R], wl[R, 4], rtol=1e-12, atol=0) and np.allclose(pf[L], wr[L, 4], rtol=1e-12, atol=0)
            c = np.sqrt(gamma * wl[:, 4] / wl[:, 0])
            assert np.all(wl[R, 1] > c[R])
    assert np.isfinite(r[:20000]).all()
    o = ref.oracle_riemann(fluid, solver, gm1, wl, wr)
    names = ("frho", "fmx", "fmy", "fmz", "fe", "feg", "face pressure", "face velocity")
    for c, name in enumerate(names):
        same_bits(r[:, c], o[:, c], f"{solver} {'dust' if fluid else 'gas'} gm1={gm1}: {name}")


# ---------------------------------------------------------------------------------------------------------------------
# geometry
GEOMETRY = [  # coordinates, nx, lower corner, upper corner
    ("cylindrical", (16, 8, 8), (0.2, 0.0, -1.0), (1.8, 2 * np.pi, 1.0)),
    ("spherical", (16, 1, 1), (0.2, 0.3, 0.0), (1.8, 2.8, 2 * np.pi)),
    ("spherical", (16, 8, 1), (0.2, 0.3, 0.0), (1.8, 2.8, 2 * np.pi)),
    ("spherical", (16, 8, 8), (0.2, 0.3, 0.0), (1.8, 2.8, 2 * np.pi)),
    ("axisymmetric", (16, 8, 8), (0.2, -1.0, 0.0), (1.8, 1.0, 1.0)),
    ("cartesian", (16, 8, 8), (-1.0, -0.5, 0.25), (1.0, 0.8, 0.95)),
]


@pytest.mark.parametrize("coordinates,nx,lo,hi", GEOMETRY, ids=lambda v: v if isinstance(v, str) else None)
def test_coords_every_cell(coordinates, nx, lo, hi):
    """geometry::Coords<GEOM> (geometry.hpp, spherical.hpp, cylindrical.hpp, axisymmetric.hpp) on every interior and
    ghost cell: volume, areas, centroids, scale factors, connection coefficients, widths, face-centre scale factors."""
    o = Oracle(nx, lo, hi, ng=2, coordinates=coordinates)
    k, j, i = np.meshgrid(np.arange(o.nk), np.arange(o.nj), np.arange(o.ni), indexing="ij")
    want = ref.coords(o.cfg.coords, ref.geom_of(o), k, j, i)
    got = ref.oracle_coords(o, k, j, i)
    assert want.shape == (o.N, ref.NCOORD) and np.isfinite(want).all()
    for c, name in enumerate(ref.COORD_NAMES):
        same_bits(want[:, c], got[:, c], f"{coordinates} {nx}: {name}")


# ---------------------------------------------------------------------------------------------------------------------
# whole sweeps
def check_sweep(o, fluid):
    o.CalculateFluxes(fluid, False)
    s = ref.sweep_of(o, fluid)
    who = f"{'dust' if fluid else 'gas'}"
    for d in range(o.ndim):
        sl = face_slices(o, d)
        want = s.scaled_flux(d)[sl]
        assert np.isfinite(want).all(), "the reference sweep left faces of the range unwritten"
        same_bits(want, (o.dflux(d) if fluid else o.gflux(d))[sl], f"{who} flux x{d + 1}")
        if fluid == GAS:
            same_bits(s.pflux[d][sl], o.gpflux(d)[sl], f"face pressure x{d + 1}")
            same_bits(s.vface[d][sl], o.gvface(d)[sl], f"face velocity x{d + 1}")


def cart_oracle(nx, ng, **kw):
    o = Oracle(nx, (-1.0, -0.5, 0.25), (1.0, 0.8, 0.95), ng=ng, gamma=1.4, **kw)
    random_state(o, np.random.default_rng(5), shock=True)
    return o


@pytest.mark.parametrize("riem", ["hllc", "hlle", "llf"])
@pytest.mark.parametrize("recon,ng", [("pcm", 2), ("plm", 2), ("ppm", 4)])
@pytest.mark.parametrize("nx", [(12, 6, 5), (9, 5, 1)])
def test_sweep_cartesian(nx, recon, ng, riem):
    """Reconstruction<>::apply (direction permutation, the i+1 indexing of the left states) and RiemannSolver<>::solve
    over scratch rows with the bounds of fluid_fluxes.hpp:105-206, against Oracle.CalculateFluxes."""
    o = cart_oracle(nx, ng, reconstruct=recon, riemann=riem)
    check_sweep(o, GAS)
    # the flat patch of random_state reaches dq2 == 0 and frho == 0 inside a sweep
    assert (o.gflux(0)[0][face_slices(o, 0)[1:]] == 0.0).any()


def mirror_state(o, d):
    """Make the gas primitives of `o` mirror images about the central face of direction d (even nx): every variable
    reflected, the normal velocity negated.  PCM, PLM and PPM4 keep the symmetry exactly, so the two states of the
    central faces are mirror images with random normal and tangential velocities: HLLC's contact speed am is 0 there
    (hllc.hpp:135,157), which no random state reaches."""
    p = o.gprim
    ax = 3 - d  # [var, k, j, i]
    n = p.shape[ax] // 2
    lower = [slice(None)] * 4
    upper = [slice(None)] * 4
    lower[ax], upper[ax] = slice(0, n), slice(n, 2 * n)
    p[tuple(upper)] = np.flip(p[tuple(lower)], axis=ax)
    ns = o.cfg.ns_gas
    for s in range(ns):
        upper[0] = ns + 3 * s + d
        p[tuple(upper)] *= -1.0
    o.PrimToCons()


@pytest.mark.parametrize("recon,ng", [("pcm", 2), ("plm", 2), ("ppm", 4)])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_sweep_mirror_plane(d, recon, ng):
    """HLLC with am == 0 inside a sweep: a block that is its own mirror image about the central face of direction d."""
    o = Oracle((12, 6, 4), (-1.0, -0.5, 0.25), (1.0, 0.8, 0.95), ng=ng, gamma=1.4, reconstruct=recon, riemann="hllc")
    random_state(o, np.random.default_rng(8), shock=False)
    mirror_state(o, d)
    s = ref.sweep_of(o, GAS)
    faces = list(face_slices(o, d)[1:])
    n = o.gprim.shape[3 - d] // 2  # the mirror plane is the lower face of cell n
    faces[2 - d] = slice(n, n + 1)
    frho, vf = s.flux[d][0][tuple(faces)], s.vface[d][0][tuple(faces)]
    assert frho.size and np.all(frho == 0.0) and np.all(vf == 0.0)
    check_sweep(o, GAS)


@pytest.mark.parametrize("recon,ng,riem", [("plm", 2, "hllc"), ("ppm", 4, "hlle"), ("pcm", 2, "llf")])
def test_sweep_two_gas_species(recon, ng, riem):
    check_sweep(cart_oracle((12, 6, 5), ng, ns_gas=2, reconstruct=recon, riemann=riem), GAS)


@pytest.mark.parametrize("driem", ["hlle", "llf"])
@pytest.mark.parametrize("drecon,ng", [("plm", 2), ("ppm", 4)])
def test_sweep_two_dust_species(drecon, ng, driem):
    check_sweep(cart_oracle((12, 6, 5), ng, ns_dust=2, dust_reconstruct=drecon, dust_riemann=driem), DUST)


CURVILINEAR = [
    ("cylindrical", (8, 6, 4), (0.8, 0.0, -1.0), (2.0, 2 * np.pi, 1.0)),
    ("spherical", (8, 1, 1), (0.8, 1.1, 0.0), (2.0, 2.1, 2 * np.pi)),
    ("spherical", (8, 6, 1), (0.8, 1.1, 0.0), (2.0, 2.1, 2 * np.pi)),
    ("spherical", (8, 6, 4), (0.8, 1.1, 0.0), (2.0, 2.1, 2 * np.pi)),
    ("axisymmetric", (8, 6, 4), (0.8, -1.0, 0.0), (2.0, 1.0, 1.0)),
]


@pytest.mark.parametrize("recon,ng,riem", [("plm", 2, "hlle"), ("plm", 2, "hllc"), ("ppm", 4, "llf")])
@pytest.mark.parametrize("coordinates,nx,lo,hi", CURVILINEAR, ids=lambda v: v if isinstance(v, str) else None)
def test_sweep_curvilinear(coordinates, nx, lo, hi, recon, ng, riem):
    """PLM_G fed by the reference's own Coords inside Reconstruction<plm, DIR, GEOM>::apply, and ScaleMomentumFlux's
    factors from the reference's Coords (one IEEE multiply in numpy), gas and dust."""
    o = Oracle(nx, lo, hi, ng=ng, ns_gas=1, ns_dust=1, reconstruct=recon, riemann=riem, dust_reconstruct=recon,
               dust_riemann="llf" if riem == "llf" else "hlle", gamma=1.4, coordinates=coordinates)
    random_state(o, np.random.default_rng(6), shock=True)
    check_sweep(o, GAS)
    check_sweep(o, DUST)
