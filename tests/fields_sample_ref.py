"""The definition of a point sample (include/artemis_hip_sample.h), emulated in numpy: containment is a plain scan over the
blocks, the zone comes from searchsorted over the faces Xf(t) = xf0 + t * dx, and the values are picked out of a gather
array.  Also the point families the sample tests share: zone centres, face coordinates, block corners, points outside the mesh
and points that are not finite."""
import numpy as np

from fields_level_ref import same_bits  # noqa: F401  (the tests import it from here)


def faces(lo, hi, n, g):
    """Xf(t), t = g .. g + n, of a block direction as the driver's geom table gives them: one multiplication, one addition"""
    dx = (hi - lo) / n
    xf0 = lo - g * dx
    return xf0 + np.arange(g, g + n + 1, dtype=np.float64) * dx


def locate(points, bounds, nx, ng, closed_hi):
    """loc [npoints, 4] int32 {block, k, j, i} of points [npoints, 3]; bounds [nb][6] = (lo1, hi1, lo2, hi2, lo3, hi3) as
    Simulation.block_bounds returns them; nx: interior zones of a block; all -1 where the point is not found"""
    points = np.asarray(points, dtype=np.float64)
    bounds = np.asarray(bounds, dtype=np.float64).reshape(-1, 6)
    active = [d for d in range(3) if nx[d] > 1]
    loc = np.full((len(points), 4), -1, dtype=np.int32)
    finite = np.ones(len(points), dtype=bool)
    for d in active:
        finite &= np.isfinite(points[:, d])
    with np.errstate(invalid="ignore"):
        for b, bd in enumerate(bounds):  # the lowest block that contains the point
            inside = finite & (loc[:, 0] < 0)
            for d in active:
                lo, hi, x = bd[2 * d], bd[2 * d + 1], points[:, d]
                inside &= (lo <= x) & ((x < hi) | ((x == hi) & (hi == closed_hi[d])))
            if not inside.any():
                continue
            loc[inside, 0] = b
            loc[inside, 1:] = 0
            for d in active:
                xf = faces(bd[2 * d], bd[2 * d + 1], nx[d], ng)
                loc[inside, 3 - d] = np.clip(np.searchsorted(xf, points[inside, d], side="right") - 1, 0, nx[d] - 1)
    return loc


def pick(gathered, loc, single=False):
    """[ncomp, npoints] of gathered [nb, ncomp, nz, ny, nx] at loc, NaN where loc says not found; narrowed like gather"""
    gathered = np.asarray(gathered)
    out = np.full((gathered.shape[1], len(loc)), np.nan)
    ok = loc[:, 0] >= 0
    out[:, ok] = gathered[loc[ok, 0], :, loc[ok, 1], loc[ok, 2], loc[ok, 3]].T
    return out.astype(np.float32) if single else out


def in_domain(points, lo, hi, nx):
    """finite along every active direction and inside the closed box [lo, hi] of the mesh"""
    ok = np.ones(len(points), dtype=bool)
    with np.errstate(invalid="ignore"):
        for d in range(3):
            if nx[d] > 1:
                ok &= np.isfinite(points[:, d]) & (points[:, d] >= lo[d]) & (points[:, d] <= hi[d])
    return ok


def centres(bd, nx, ng):
    """per direction the zone centres of a block (the middle of [lo, hi] along a direction of one zone)"""
    out = []
    for d in range(3):
        xf = faces(bd[2 * d], bd[2 * d + 1], nx[d], ng if nx[d] > 1 else 0)
        out.append(0.5 * (xf[:-1] + xf[1:]))
    return out


def cross(x1, x2, x3):
    a3, a2, a1 = np.meshgrid(x3, x2, x1, indexing="ij")
    return np.stack([a1.ravel(), a2.ravel(), a3.ravel()], axis=1)


def centre_points(bounds, nx, ng):
    """every zone centre of every block, in gather's order [block][k][j][i]"""
    return np.concatenate([cross(*centres(bd, nx, ng)) for bd in np.asarray(bounds).reshape(-1, 6)])


def face_points(bounds, nx, ng):
    """every face coordinate Xf(t) of every block along each active direction, crossed with the centres along the others: the
    lower-inclusive rule, the faces blocks share, and the closed upper edge of the mesh"""
    out = []
    for bd in np.asarray(bounds).reshape(-1, 6):
        c = centres(bd, nx, ng)
        for d in range(3):
            if nx[d] > 1:
                axes = list(c)
                axes[d] = faces(bd[2 * d], bd[2 * d + 1], nx[d], ng)
                out.append(cross(*axes))
    return np.concatenate(out)


def corner_points(bounds):
    out = []
    for bd in np.asarray(bounds).reshape(-1, 6):
        out.append(cross(bd[0:2], bd[2:4], bd[4:6]))
    return np.concatenate(out)


def outside_points(lo, hi, nx, bounds, ng):
    """one zone width outside every face of the mesh, and a NaN and an inf along every active direction: none is found"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    bd = np.asarray(bounds).reshape(-1, 6)[0]
    mid = 0.5 * (lo + hi)
    out = []
    for d in range(3):
        if nx[d] > 1:
            dx = (bd[2 * d + 1] - bd[2 * d]) / nx[d]
            for v in (lo[d] - dx, hi[d] + dx, np.nan, np.inf, -np.inf):
                p = mid.copy()
                p[d] = v
                out.append(p)
    return np.array(out)


def uniform_points(lo, hi, count, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), size=(count, 3))


def families(bounds, nx, ng, lo, hi, seed=7, count=4096):
    """name -> points of the five families on a mesh (or pack) of these blocks inside the box [lo, hi]"""
    c = centre_points(bounds, nx, ng)
    return {"centres": np.ascontiguousarray(c[np.random.default_rng(seed).permutation(len(c))]), "faces": face_points(bounds, nx, ng),
            "corners": corner_points(bounds), "outside": outside_points(lo, hi, nx, bounds, ng), "uniform": uniform_points(lo, hi, count, seed + 1)}
