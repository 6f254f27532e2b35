"""The definition of the derived field outputs -- velocity divergence and vorticity (include/artemis_hip.h, "derived
variables") -- emulated in numpy for tests/test_fields_derived.py and tests/test_fields_derived_cpu.py.  Not a test module.

Built from a block's GHOSTED primitives.  Face areas and volumes come from the CPU oracle (face_areas(d): the lower face at
the cell, so the upper face is the lower face of the next cell; d = 0 the volume), the scale factors h and the centres xi
from the DCoords formulas written out below on the faces xf0 + idx * dx, and the trigonometry of the spherical systems from
the tables artemis_hip_metric_fill returns (host code), never from numpy's sin: the reference depends on no libm of its own.
numpy evaluates float64 arrays element by element with IEEE operations, so these are the bits the device must give."""
import ctypes as C

import numpy as np

MT_COSF, MT_SINF, MT_X2V = 0, 1, 2  # rows of the metric table (csrc/geometry_core.hpp)
GAS_DIV, GAS_VORT, DUST_DIV, DUST_VORT = "gas.derived.divergence", "gas.derived.vorticity", "dust.derived.divergence", "dust.derived.vorticity"


class BlockGeometry:
    """areas, volume, h and xi of every zone of one block, ghost zones included, as [nk, nj, ni] arrays"""

    def __init__(self, nx, xmin, xmax, ng, coordinates):
        from artemis_amd import capi
        from oracle.oracle import Oracle
        nx = tuple(int(n) for n in nx)
        self.nx, self.ng = nx, ng
        self.active = tuple(n > 1 for n in nx)
        ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
        g = [ng if a else 0 for a in self.active]
        g[0] = ng
        self.lo = g
        n = [nx[d] + 2 * g[d] for d in range(3)]  # ni, nj, nk
        self.shape = (n[2], n[1], n[0])
        o = Oracle(nx, tuple(xmin), tuple(xmax), ng=ng, coordinates=coordinates)
        assert (o.nk, o.nj, o.ni) == self.shape
        self.vol = o.face_areas(0)
        self.area = [o.face_areas(d + 1) if self.active[d] else None for d in range(3)]
        sys = capi.coord_select(coordinates, ndim)
        sph23 = sys in (capi.SPHERICAL2D, capi.SPHERICAL3D)
        sph = sph23 or sys == capi.SPHERICAL1D
        geom = np.zeros(6)
        for d in range(3):
            dx = (float(xmax[d]) - float(xmin[d])) / nx[d]
            geom[2 * d], geom[2 * d + 1] = float(xmin[d]) - g[d] * dx, dx
        f = [geom[2 * d] + np.arange(n[d] + 1) * geom[2 * d + 1] for d in range(3)]  # faces
        x0, x1 = f[0][:-1], f[0][1:]
        if sph:
            dr2 = x0 * x0 + x1 * x1
            x1v = 0.75 * (x0 + x1) * dr2 / (dr2 + x0 * x1)
        elif sys in (capi.CYLINDRICAL, capi.AXISYMMETRIC):
            x1v = 2.0 / 3.0 * (x0 * x0 + x0 * x1 + x1 * x1) / (x0 + x1)
        else:
            x1v = 0.5 * (x0 + x1)
        x2v, x3v = 0.5 * (f[1][:-1] + f[1][1:]), 0.5 * (f[2][:-1] + f[2][1:])
        one = np.ones(self.shape)
        h2 = x1v[None, None, :] * one if (sph23 or sys == capi.CYLINDRICAL) else one
        h3 = one
        if sph23:
            L = capi.load()
            p = capi.Pack()
            p.nblocks, p.nghost, p.coords = 1, ng, sys
            p.nx1, p.nx2, p.nx3 = nx
            m = np.zeros(L.artemis_hip_metric_count(C.byref(p)))
            capi.check(L.artemis_hip_metric_fill(C.byref(p), geom.ctypes.data, m.ctypes.data))
            st = n[1] + 1
            cf, sf = m[MT_COSF * st:MT_COSF * st + st], m[MT_SINF * st:MT_SINF * st + st]
            x2v = m[MT_X2V * st:MT_X2V * st + n[1]].copy()
            dsc = sf[1:] * cf[1:] - sf[:-1] * cf[:-1]
            dx2 = f[1][1:] - f[1][:-1]
            h3 = x1v[None, None, :] * 0.5 * (dx2 - dsc)[None, :, None] / np.abs(cf[:-1] - cf[1:])[None, :, None] * one
        elif sys == capi.AXISYMMETRIC:
            h3 = x1v[None, None, :] * one
        self.h = [one, h2, h3]
        self.xi = [x1v[None, None, :] * one, x2v[None, :, None] * one, x3v[:, None, None] * one]

    def window(self, a, d=0, s=0):
        """the interior zones of a [.., nk, nj, ni] array, moved by s zones along direction d"""
        sl = [slice(self.lo[q] + (s if q == d else 0), self.lo[q] + self.nx[q] + (s if q == d else 0)) for q in range(3)]
        return a[..., sl[2], sl[1], sl[0]]

    def volumes(self):
        return np.ascontiguousarray(self.window(self.vol))


def derived(vel, G):
    """vel: the three stored velocity components of one species, [3, nk, nj, ni] with ghost zones.  Returns (div, w) on the
    interior zones: [nz, ny, nx] and [3, nz, ny, nx]."""
    w0 = G.window
    zero = np.zeros(w0(vel[0]).shape)  # the literal +0.0 of an inactive direction
    T = [zero, zero, zero]
    D = [[zero] * 3 for _ in range(3)]  # D[a][d] = D_a[g_d]
    for a in range(3):
        if not G.active[a]:
            continue
        v0, vm, vp = w0(vel[a]), w0(vel[a], a, -1), w0(vel[a], a, +1)
        T[a] = w0(G.area[a], a, +1) * (0.5 * (v0 + vp)) - w0(G.area[a]) * (0.5 * (vm + v0))
        dxi = w0(G.xi[a], a, +1) - w0(G.xi[a], a, -1)
        for d in range(3):
            if d != a:
                D[a][d] = (w0(G.h[d], a, +1) * w0(vel[d], a, +1) - w0(G.h[d], a, -1) * w0(vel[d], a, -1)) / dxi
    h2, h3 = w0(G.h[1]), w0(G.h[2])
    div = ((T[0] + T[1]) + T[2]) / w0(G.vol)
    w = np.stack([(D[1][2] - D[2][1]) / (h2 * h3), (D[2][0] - D[0][2]) / h3, (D[0][1] - D[1][0]) / h2])
    return div, w


def block_components(names, gas, dust, nsg, nsd, G):
    """[ncomp, nz, ny, nx]: the components of the derived `names` of one block, in gather's order (a vector 3 n + d), from
    its ghosted primitives gas [6 nsg, nk, nj, ni] and dust [4 nsd, nk, nj, ni] (None where the fluid is absent)"""
    cache, rows = {}, []

    def of(prim, ns, n):
        key = (id(prim), n)
        if key not in cache:
            cache[key] = derived(prim[ns + 3 * n:ns + 3 * n + 3], G)
        return cache[key]
    for name in names:
        prim, ns = (dust, nsd) if name.startswith("dust.") else (gas, nsg)
        for n in range(ns):
            div, w = of(prim, ns, n)
            rows += [div] if name.endswith("divergence") else [w[0], w[1], w[2]]
    return np.stack(rows)
