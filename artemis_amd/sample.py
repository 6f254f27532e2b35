"""Points for Simulation.sample_plan / Simulation.sample (numpy only): the zone centres of a box, and the mesh coordinates of
Cartesian positions on a curvilinear mesh.  A sample takes the value of the zone that holds a point, so a lattice laid over
whole zones reads as an array of the mesh itself: a slice is a box one cell thick, a zoom a box at the finest zone size."""
import numpy as np

TWO_PI = 2.0 * np.pi


def lattice(lo, hi, shape):
    """Centres of the shape = (n1, n2, n3) cells of the box [lo, hi] (three numbers each, x1 x2 x3) as [n3 * n2 * n1, 3]
    float64, x1 fastest: values(...).reshape(ncomp, n3, n2, n1) is the box as gather would lay it out.  An extent of one
    cell puts the points at the middle of [lo, hi] along it -- the midplane of a block is lattice((x1min, x2min, z), (x1max,
    x2max, z), (nx1, nx2, 1)); along a direction the mesh does not have, any numbers do."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    shape = tuple(int(n) for n in shape)
    if lo.shape != (3,) or hi.shape != (3,) or len(shape) != 3 or min(shape) < 1:
        raise ValueError("lattice takes lo and hi of three numbers and a shape of three positive counts")
    axes = [lo[d] + (np.arange(shape[d]) + 0.5) * ((hi[d] - lo[d]) / shape[d]) for d in range(3)]
    x3, x2, x1 = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x1.ravel(), x2.ravel(), x3.ravel()], axis=1))


def from_cartesian(coordinates, xyz, lo=None, hi=None):
    """Mesh coordinates [n, 3] of the Cartesian positions xyz [n, 3] (x, y, z) on a mesh of the named system, with the axes of
    the reference's ConvertCoordsToCart:
        "cartesian"                     (x, y, z)
        "cylindrical"                   (R, phi, z)      x = R cos phi,           y = R sin phi
        "spherical"                     (r, theta, phi)  x = r sin theta cos phi, y = r sin theta sin phi, z = r cos theta
        "axisymmetric"                  (R, z, phi)
    lo, hi: the mesh's lower and upper corner (three numbers each, or None; only lo's azimuth is used, hi is taken so that a
    mesh's two corners can be passed as they are); the azimuth is brought into [lo, lo + 2 pi) of its direction (phi from
    atan2 lies in (-pi, pi]; a disk deck runs 0 .. 2 pi), so the pixel grid of a disk image samples as it is.  A position the mesh does not cover -- inside the inner radius, beyond the outer one -- comes back as a point
    that sample() does not find."""
    xyz = np.asarray(xyz, dtype=np.float64)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("from_cartesian takes positions [n, 3]")
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if coordinates == "cartesian":
        return np.ascontiguousarray(xyz)
    phi = np.arctan2(y, x)
    az = {"cylindrical": 1, "spherical": 2, "axisymmetric": 2}.get(coordinates)
    if az is None:
        raise ValueError("from_cartesian knows cartesian, cylindrical, spherical and axisymmetric, not %r" % (coordinates,))
    start = 0.0 if lo is None else float(np.asarray(lo, dtype=np.float64)[az])
    phi = start + np.mod(phi - start, TWO_PI)
    phi = np.where(phi >= start + TWO_PI, start, phi)  # (a remainder rounded up to the whole turn belongs to the start)
    R = np.hypot(x, y)
    if coordinates == "cylindrical":
        out = [R, phi, z]
    elif coordinates == "axisymmetric":
        out = [R, z, phi]
    else:
        r = np.sqrt(x * x + y * y + z * z)
        out = [r, np.arctan2(R, z), phi]
    return np.ascontiguousarray(np.stack(out, axis=1))
