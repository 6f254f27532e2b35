"""ctypes binding for the reference leaf library (oracle/ref/ref_leaves.cpp -> oracle/_ref/libartemis_ref.so): the
reference's own, unmodified reconstruction, Riemann and geometry headers behind a C ABI, built by `make -C oracle`
where the reference's source tree is present.  The library is never committed; it travels with the tree.

TEST INFRASTRUCTURE ONLY, like oracle/oracle.py.  Enumerations and array layouts are the oracle's.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .oracle import COORDS, RC, RS, coord_select  # noqa: F401  (re-exported for the tests)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "_ref", "libartemis_ref.so")
NCOORD = 31  # doubles per cell of ref_coords / oracle_coords
COORD_NAMES = (["Volume", "AreaX1", "AreaX2", "AreaX3", "x1v", "x2v", "x3v", "hx1v", "hx2v", "hx3v"]
               + [f"dh{c}dx{d}" for d in (1, 2, 3) for c in (1, 2, 3)] + ["WidthX1", "WidthX2", "WidthX3"]
               + [f"hx{c}@X{d}face" for d in (1, 2, 3) for c in (1, 2, 3)])

_P = C.POINTER(C.c_double)
_PI = C.POINTER(C.c_int)
_PP = C.POINTER(_P)
_lib = None
_tried = False
_obound = False


def reference_dir():
    """The reference tree's location: oracle/Makefile's REFERENCE (one place to say it)."""
    try:
        return subprocess.check_output(["make", "-s", "--no-print-directory", "-C", _HERE, "reference-dir"],
                                       text=True).strip()
    except Exception:
        return ""


def lib():
    global _lib, _tried
    if not _tried:
        _tried = True
        if not os.path.exists(_LIB) and required():
            subprocess.call(["make", "-C", _HERE, "-s"])
        if os.path.exists(_LIB):
            L = C.CDLL(_LIB)
            L.ref_plm.argtypes = [C.c_long] + [_P] * 5
            L.ref_plm_g.argtypes = [C.c_long] + [_P] * 11
            L.ref_ppm4.argtypes = [C.c_long] + [_P] * 7
            L.ref_riemann.argtypes = [C.c_int, C.c_int, C.c_double, C.c_long, _P, _P, _P]
            L.ref_coords.argtypes = [C.c_int, _P, _PI, _PI, _PI, C.c_long, _P]
            L.ref_sweep.argtypes = [C.c_int] * 4 + [C.c_double, C.c_int, _PI, C.c_int, _P, _P, _PP, _PP, _PP, _PP]
            _lib = L
    return _lib


def available():
    """The library loads."""
    return lib() is not None


def required():
    """The library must be there: this machine has the reference tree (so `make -C oracle` builds it), or it has a
    GPU (so the tree came with what `make -C oracle` built where the reference is)."""
    d = reference_dir()
    if d and os.path.exists(os.path.join(d, "src", "artemis.hpp")):
        return True
    try:
        import torch
        return bool(torch.cuda.is_available())
    except Exception:
        return False


def need():
    """For a test's first line: skip where the library neither exists nor can be expected, fail where it is missing."""
    import pytest
    if available():
        return
    if not required():
        pytest.skip("no reference leaf library, no reference tree to build it from and no GPU")
    pytest.fail("oracle/_ref/libartemis_ref.so is missing: run `make -C oracle` on a machine that has the "
                "reference's source tree (oracle/Makefile's REFERENCE) and bring oracle/_ref/ along with the tree")


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_P)


def _table(fn, ins):
    ins = [_d(a) for a in np.broadcast_arrays(*ins)]
    n = ins[0].size
    ql, qr = np.empty(n), np.empty(n)
    fn(n, *[_p(a) for a in ins], _p(ql), _p(qr))
    return ql, qr


# ---- scalar reconstructions: (ql_ip1, qr_i) arrays -------------------------------------------------------------
def plm(qm, q, qp): return _table(lib().ref_plm, (qm, q, qp))
def ppm4(qmm, qm, q, qp, qpp): return _table(lib().ref_ppm4, (qmm, qm, q, qp, qpp))
def plm_g(qm, q, qp, xm, xc, xp, xf0, xf1, dx): return _table(lib().ref_plm_g, (qm, q, qp, xm, xc, xp, xf0, xf1, dx))


def _olib():
    from . import oracle
    L = oracle.lib()
    global _obound
    if not _obound:
        L.oracle_plm_n.argtypes = [C.c_long] + [_P] * 5
        L.oracle_plm_g.argtypes = [C.c_long] + [_P] * 11
        L.oracle_ppm4_n.argtypes = [C.c_long] + [_P] * 7
        L.oracle_riemann_n.argtypes = [C.c_int, C.c_int, C.c_double, C.c_long, _P, _P, _P]
        L.oracle_geom.argtypes = [C.c_void_p, _P]
        L.oracle_coords.argtypes = [C.c_void_p, _PI, _PI, _PI, C.c_long, _P]
        _obound = True
    return L


# the oracle's leaves over the same tables
def oracle_plm(qm, q, qp): return _table(_olib().oracle_plm_n, (qm, q, qp))
def oracle_ppm4(qmm, qm, q, qp, qpp): return _table(_olib().oracle_ppm4_n, (qmm, qm, q, qp, qpp))


def oracle_plm_g(qm, q, qp, xm, xc, xp, xf0, xf1, dx):
    return _table(_olib().oracle_plm_g, (qm, q, qp, xm, xc, xp, xf0, xf1, dx))


def _solver(s):
    return RS[s] if isinstance(s, str) else s


def riemann(fluid, solver, gm1, wl, wr):
    """RiemannSolver<solver, fluid>::solve on n faces: wl, wr [n, 6] (dust [n, 4]) -> [n, 8]
    (frho, fmx, fmy, fmz, fe, feg, face pressure, face velocity)."""
    wl, wr = _d(wl), _d(wr)
    assert wl.shape == wr.shape and wl.shape[1] == (4 if fluid else 6)
    out = np.empty((wl.shape[0], 8))
    assert lib().ref_riemann(fluid, _solver(solver), gm1, wl.shape[0], _p(wl), _p(wr), _p(out)) == 0
    return out


def oracle_riemann(fluid, solver, gm1, wl, wr):
    wl, wr = _d(wl), _d(wr)
    out = np.empty((wl.shape[0], 8))
    _olib().oracle_riemann_n(fluid, _solver(solver), gm1, wl.shape[0], _p(wl), _p(wr), _p(out))
    return out


# ---- geometry ---------------------------------------------------------------------------------------------------
def geom_of(o):
    """{x1 of face 0, dx1, ...} of an Oracle block: the arguments of Coordinates_t::Xf."""
    g = np.empty(6)
    _olib().oracle_geom(o.h, _p(g))
    return g


def _kji(k, j, i):
    k, j, i = [np.ascontiguousarray(a, dtype=np.int32).ravel() for a in np.broadcast_arrays(k, j, i)]
    return k, j, i


def coords(system, geom, k, j, i):
    """Coords<system> at cells (k, j, i): [n, NCOORD], columns COORD_NAMES."""
    k, j, i = _kji(k, j, i)
    out = np.empty((k.size, NCOORD))
    g = _d(geom)
    assert lib().ref_coords(system, _p(g), k.ctypes.data_as(_PI), j.ctypes.data_as(_PI), i.ctypes.data_as(_PI),
                            k.size, _p(out)) == 0
    return out


def oracle_coords(o, k, j, i):
    k, j, i = _kji(k, j, i)
    out = np.empty((k.size, NCOORD))
    _olib().oracle_coords(o.h, k.ctypes.data_as(_PI), j.ctypes.data_as(_PI), i.ctypes.data_as(_PI), k.size, _p(out))
    return out


# ---- whole sweeps -----------------------------------------------------------------------------------------------
class Sweep:
    """Result of sweep(): flux[d] [nvar, nk, nj, ni], pflux[d] / vface[d] [nsp, nk, nj, ni] (gas), hface[d]
    [3, nk, nj, ni]; unwritten cells hold NaN.  scaled_flux(d) applies ScaleMomentumFlux (fluid_fluxes.hpp:64-66):
    one IEEE multiply of each momentum flux by the reference's own scale factor at the face centre."""

    def scaled_flux(self, d):
        f = self.flux[d].copy()
        if self.system != COORDS["cartesian"]:
            for n in range(self.nsp):
                for c in range(3):
                    f[self.nsp + 3 * n + c] *= self.hface[d][c]
        return f


def sweep(system, fluid, recon, solver, gm1, nsp, nx, ng, geom, prim):
    """Reconstruction<recon, DIR, system>::apply + RiemannSolver<solver, fluid>::solve in every active direction of
    one block (nx interior zones, ng ghosts), with the index bounds of fluid_fluxes.hpp:105-206."""
    prim = _d(prim)
    nvar, nk, nj, ni = prim.shape
    assert nvar == (4 if fluid else 6) * nsp
    r = Sweep()
    r.system, r.nsp = system, nsp
    nan = lambda nv: [np.full((nv, nk, nj, ni), np.nan) for _ in range(3)]
    r.flux, r.hface = nan(nvar), nan(3)
    r.pflux, r.vface = (nan(nsp), nan(nsp)) if fluid == 0 else (None, None)
    arr3 = lambda a: (_P * 3)(*[_p(x) for x in a]) if a is not None else (_P * 3)()
    g = _d(geom)
    rc = lib().ref_sweep(system, fluid, RC[recon] if isinstance(recon, str) else recon, _solver(solver), gm1, nsp,
                         (C.c_int * 3)(*nx), ng, _p(g), _p(prim), arr3(r.flux), arr3(r.pflux), arr3(r.vface),
                         arr3(r.hface))
    assert rc == 0, "ref_sweep: no such (system, fluid, reconstruction, solver)"
    return r


def sweep_of(o, fluid=0, pcm=False):
    """sweep() with the configuration, geometry and primitives of an Oracle block."""
    c = o.cfg
    gas = fluid == 0
    recon = 0 if pcm else (c.recon_gas if gas else c.recon_dust)
    return sweep(c.coords, fluid, recon, c.riemann_gas if gas else c.riemann_dust, c.gamma - 1.0,
                 c.ns_gas if gas else c.ns_dust, (c.nx1, c.nx2, c.nx3), c.ng, geom_of(o),
                 o.gprim if gas else o.dprim)
