// C-ABI harness around the reference's own, unmodified leaf headers: the scalar reconstructions, the
// Reconstruction<> and RiemannSolver<> classes and geometry::Coords<>.  Test infrastructure only (tests/
// test_reference_leaves.py, tests/test_parity_reference.py through oracle/reference.py); built by oracle/Makefile into
// oracle/_ref/ where the reference tree is present, and never committed in compiled form.
//
// Everything the reference computes is reached through its headers; this file only provides the packs its templates
// are duck-typed against, the loops of the caller (utils/fluxes/fluid_fluxes.hpp, which does not parse against the
// stand-ins) and the marshalling.  Arrays use the oracle's layout: [var][k][j][i] with ghost zones, face `f` of a
// sweep stored at the cell whose lower face it is.
#include "artemis.hpp"
#include "geometry/geometry.hpp"
#include "utils/fluxes/reconstruction/reconstruction.hpp"
#include "utils/fluxes/riemann/riemann.hpp"

#include <cstring>
#include <vector>

namespace {

using parthenon::Coordinates_t;
using parthenon::ScratchPad2D;
using parthenon::team_mbr_t;
using TE = parthenon::TopologicalElement;

// One block with ghost zones, shaped as oracle_create shapes it.
struct Block {
  int ni, nj, nk, is, ie, js, je, ks, ke, ndim;
  size_t N;
  Coordinates_t co;
  Block(const int nx[3], int ng, const double geom[6]) {
    ndim = (nx[2] > 1) ? 3 : ((nx[1] > 1) ? 2 : 1);
    const int g1 = ng, g2 = (nx[1] > 1) ? ng : 0, g3 = (nx[2] > 1) ? ng : 0;
    ni = nx[0] + 2 * g1, nj = nx[1] + 2 * g2, nk = nx[2] + 2 * g3;
    is = g1, ie = g1 + nx[0] - 1, js = g2, je = g2 + nx[1] - 1, ks = g3, ke = g3 + nx[2] - 1;
    N = static_cast<size_t>(ni) * nj * nk;
    for (int d = 0; d < 3; ++d) co.x0[d] = geom[2 * d], co.dx[d] = geom[2 * d + 1];
  }
  size_t idx(int k, int j, int i) const { return (static_cast<size_t>(k) * nj + j) * ni + i; }
};

// The packs the reference's templates see.  Variable order inside a pack is the reference's: density of every
// species, then the velocity triples, then (gas) pressure and specific internal energy.
struct PrimPack { // vprim: read by Reconstruction<>::apply; its flux of the pressure slot is the face pressure
  const Block *blk;
  const Real *prim;
  Real *pflux[3];
  int nvar, nsp;
  const Real &operator()(int, int n, int k, int j, int i) const { return prim[n * blk->N + blk->idx(k, j, i)]; }
  int GetLowerBound(int) const { return 0; }
  int GetUpperBound(int) const { return nvar - 1; }
  int GetMaxNumberOfVars() const { return nvar; }
  const Coordinates_t &GetCoordinates(int) const { return blk->co; }
  Real &flux(int, int dir, int v, int k, int j, int i) const {
    return pflux[dir - 1][(v - 4 * nsp) * blk->N + blk->idx(k, j, i)];
  }
};
struct FluxPack { // vflux: the conserved variables' fluxes
  const Block *blk;
  Real *f[3];
  int nvar;
  int GetMaxNumberOfVars() const { return nvar; }
  const Coordinates_t &GetCoordinates(int) const { return blk->co; }
  Real &flux(int, int dir, int v, int k, int j, int i) const { return f[dir - 1][v * blk->N + blk->idx(k, j, i)]; }
};
struct FacePack { // vface: gas::face::velocity on F1..F3
  const Block *blk;
  Real *v[3];
  Real &operator()(int, TE el, int n, int k, int j, int i) const {
    return v[static_cast<int>(el) - static_cast<int>(TE::F1)][n * blk->N + blk->idx(k, j, i)];
  }
};

// ---------------------------------------------------------------------------------------------------------------
// ref_riemann: one face through the solver class
struct OneFacePrim {
  Real *pf;
  int nvar;
  int GetMaxNumberOfVars() const { return nvar; }
  Real &flux(int, int, int, int, int, int) const { return *pf; }
};
struct OneFaceFlux {
  Real *out;
  Real &flux(int, int, int v, int, int, int) const { return out[v]; }
};
struct OneFaceVel {
  Real *vf;
  Real &operator()(int, TE, int, int, int, int) const { return *vf; }
};

template <RSolver RS, Fluid FL>
void riemann_table(const double gm1, const long n, const double *wl, const double *wr, double *out) {
  constexpr int nv = (FL == Fluid::gas) ? 6 : 4;
  ArtemisUtils::EOS eos{singularity::IdealGas(gm1, 1.0)};
  ArtemisUtils::RiemannSolver<RS, FL> riemann;
  team_mbr_t mbr;
  for (long f = 0; f < n; ++f) {
    Real l[6], r[6], o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::memcpy(l, wl + f * nv, nv * sizeof(Real));
    std::memcpy(r, wr + f * nv, nv * sizeof(Real));
    ScratchPad2D<Real> sl(l, nv, 1), sr(r, nv, 1);
    // one species: IDN 0, velocities 1..3, IPR = IEN 4, ISE = IEG 5 -- already the 8-double layout's first six
    riemann.solve(eos, mbr, 0, 0, 0, 0, 0, X1DIR, sl, sr, OneFacePrim{&o[6], nv}, OneFaceFlux{o}, OneFaceVel{&o[7]});
    std::memcpy(out + f * 8, o, sizeof(o));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// ref_coords: what the hot path reads of Coords<GEOM>, 31 doubles a cell
constexpr int NCOORD = 31;
template <Coordinates GEOM>
void coords_cell(const Coordinates_t &pco, int k, int j, int i, double *o) {
  using geometry::CellFace;
  geometry::Coords<GEOM> c(pco, k, j, i);
  o[0] = c.Volume();
  o[1] = c.template GetFaceArea<X1DIR>(), o[2] = c.template GetFaceArea<X2DIR>();
  o[3] = c.template GetFaceArea<X3DIR>();
  o[4] = c.x1v(), o[5] = c.x2v(), o[6] = c.x3v();
  o[7] = c.hx1v(), o[8] = c.hx2v(), o[9] = c.hx3v();
  o[10] = c.dh1dx1(), o[11] = c.dh2dx1(), o[12] = c.dh3dx1();
  o[13] = c.dh1dx2(), o[14] = c.dh2dx2(), o[15] = c.dh3dx2();
  o[16] = c.dh1dx3(), o[17] = c.dh2dx3(), o[18] = c.dh3dx3();
  o[19] = c.GetCellWidthX1(), o[20] = c.GetCellWidthX2(), o[21] = c.GetCellWidthX3();
  const std::array<Real, 3> xf[3] = {c.FaceCenX1(CellFace::lower), c.FaceCenX2(CellFace::lower),
                                     c.FaceCenX3(CellFace::lower)};
  for (int d = 0; d < 3; ++d) {
    o[22 + 3 * d + 0] = c.hx1(xf[d][0], xf[d][1], xf[d][2]);
    o[22 + 3 * d + 1] = c.hx2(xf[d][0], xf[d][1], xf[d][2]);
    o[22 + 3 * d + 2] = c.hx3(xf[d][0], xf[d][1], xf[d][2]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// ref_sweep: Reconstruction<>::apply and RiemannSolver<>::solve over scratch rows
template <Coordinates GEOM, Fluid FL, RSolver RS, ReconstructionMethod RC>
void sweep(const Block &B, const double gm1, const int nsp, const double *prim, double *const flux[3],
           double *const pflux[3], double *const vface[3], double *const hface[3]) {
  const int nvars = ((FL == Fluid::gas) ? 6 : 4) * nsp;
  const int ncells1 = B.ni;
  ArtemisUtils::EOS eos{singularity::IdealGas(gm1, 1.0)};
  const PrimPack vprim{&B, prim, {pflux[0], pflux[1], pflux[2]}, nvars, nsp};
  const FluxPack vflux{&B, {flux[0], flux[1], flux[2]}, nvars};
  const FacePack vface_{&B, {vface[0], vface[1], vface[2]}};
  team_mbr_t mbr;
  const int b = 0;
  std::vector<Real> s1(static_cast<size_t>(nvars) * ncells1), s2(s1.size()), s3(s1.size());
  const bool multi_d = (B.ndim > 1), three_d = (B.ndim > 2);

  // The loops below are those of fluid_fluxes.hpp:105-206 (CalculateFluxesImpl), serial: the same index bounds, the
  // same three scratch rows exchanged on the parity of j (k).  ScaleMomentumFlux (:125,:164,:206) is left to the
  // caller; hface holds the factors it would multiply by.
  // X1-Flux (:105-126)
  {
    const int il = B.is, iu = B.ie + 1;
    for (int k = B.ks; k <= B.ke; ++k)
      for (int j = B.js; j <= B.je; ++j) {
        ScratchPad2D<Real> wl(s1.data(), nvars, ncells1), wr(s2.data(), nvars, ncells1);
        ArtemisUtils::Reconstruction<RC, X1DIR, GEOM> recon;
        recon.apply(mbr, b, k, j, il - 1, iu, vprim, wl, wr);
        ArtemisUtils::RiemannSolver<RS, FL> riemann;
        riemann.solve(eos, mbr, b, k, j, il, iu, X1DIR, wl, wr, vprim, vflux, vface_);
      }
  }
  // X2-Flux (:129-168)
  if (multi_d) {
    const int jl = B.js - 1, ju = B.je + 1, il = B.is, iu = B.ie;
    for (int k = B.ks; k <= B.ke; ++k) {
      ScratchPad2D<Real> scr1(s1.data(), nvars, ncells1), scr2(s2.data(), nvars, ncells1),
          scr3(s3.data(), nvars, ncells1);
      for (int j = jl; j <= ju; ++j) {
        auto wl = scr1;
        auto wl_jp1 = scr2;
        auto wr = scr3;
        if ((j % 2) == 0) {
          wl = scr2;
          wl_jp1 = scr1;
        }
        ArtemisUtils::Reconstruction<RC, X2DIR, GEOM> recon;
        recon.apply(mbr, b, k, j, il, iu, vprim, wl_jp1, wr);
        if (j > jl) {
          ArtemisUtils::RiemannSolver<RS, FL> riemann;
          riemann.solve(eos, mbr, b, k, j, il, iu, X2DIR, wl, wr, vprim, vflux, vface_);
        }
      }
    }
  }
  // X3-Flux (:171-210)
  if (three_d) {
    const int kl = B.ks - 1, ku = B.ke + 1, il = B.is, iu = B.ie;
    for (int j = B.js; j <= B.je; ++j) {
      ScratchPad2D<Real> scr1(s1.data(), nvars, ncells1), scr2(s2.data(), nvars, ncells1),
          scr3(s3.data(), nvars, ncells1);
      for (int k = kl; k <= ku; ++k) {
        auto wl = scr1;
        auto wl_kp1 = scr2;
        auto wr = scr3;
        if ((k % 2) == 0) {
          wl = scr2;
          wl_kp1 = scr1;
        }
        ArtemisUtils::Reconstruction<RC, X3DIR, GEOM> recon;
        recon.apply(mbr, b, k, j, il, iu, vprim, wl_kp1, wr);
        if (k > kl) {
          ArtemisUtils::RiemannSolver<RS, FL> riemann;
          riemann.solve(eos, mbr, b, k, j, il, iu, X3DIR, wl, wr, vprim, vflux, vface_);
        }
      }
    }
  }
  // scale factors at the lower face centres of every cell, [3][k][j][i] per direction
  for (int k = 0; k < B.nk; ++k)
    for (int j = 0; j < B.nj; ++j)
      for (int i = 0; i < B.ni; ++i) {
        double o[NCOORD];
        coords_cell<GEOM>(B.co, k, j, i, o);
        for (int d = 0; d < 3; ++d)
          for (int c = 0; c < 3; ++c) hface[d][c * B.N + B.idx(k, j, i)] = o[22 + 3 * d + c];
      }
}

template <Coordinates GEOM, Fluid FL, RSolver RS, class... A>
int sweep_recon(int recon, A &&...a) {
  switch (recon) {
  case 0: sweep<GEOM, FL, RS, ReconstructionMethod::pcm>(a...); return 0;
  case 1: sweep<GEOM, FL, RS, ReconstructionMethod::plm>(a...); return 0;
  case 2: sweep<GEOM, FL, RS, ReconstructionMethod::ppm>(a...); return 0;
  }
  return 1;
}
template <Coordinates GEOM, class... A>
int sweep_solver(int fluid, int solver, int recon, A &&...a) {
  if (fluid == 0) {
    switch (solver) {
    case 0: return sweep_recon<GEOM, Fluid::gas, RSolver::hllc>(recon, a...);
    case 1: return sweep_recon<GEOM, Fluid::gas, RSolver::hlle>(recon, a...);
    case 2: return sweep_recon<GEOM, Fluid::gas, RSolver::llf>(recon, a...);
    }
  } else if (fluid == 1) {
    switch (solver) { // (the HLLC solver needs an energy equation: hllc.hpp:62)
    case 1: return sweep_recon<GEOM, Fluid::dust, RSolver::hlle>(recon, a...);
    case 2: return sweep_recon<GEOM, Fluid::dust, RSolver::llf>(recon, a...);
    }
  }
  return 1;
}

} // namespace

extern "C" {

// Enumerations are the reference's (artemis.hpp:78-92), which are also the oracle's.
// Scalar reconstructions over tables of n stencils.
void ref_plm(long n, const double *qm, const double *q, const double *qp, double *ql_ip1, double *qr_i) {
  for (long s = 0; s < n; ++s) ArtemisUtils::PLM(qm[s], q[s], qp[s], ql_ip1[s], qr_i[s]);
}
void ref_plm_g(long n, const double *qm, const double *q, const double *qp, const double *xm, const double *xc,
               const double *xp, const double *xf0, const double *xf1, const double *dx, double *ql_ip1,
               double *qr_i) {
  for (long s = 0; s < n; ++s) {
    const Real xf[2] = {xf0[s], xf1[s]};
    ArtemisUtils::PLM_G(qm[s], q[s], qp[s], ql_ip1[s], qr_i[s], xm[s], xc[s], xp[s], xf, dx[s]);
  }
}
void ref_ppm4(long n, const double *qmm, const double *qm, const double *q, const double *qp, const double *qpp,
              double *ql_ip1, double *qr_i) {
  for (long s = 0; s < n; ++s) ArtemisUtils::PPM4(qmm[s], qm[s], q[s], qp[s], qpp[s], ql_ip1[s], qr_i[s]);
}

// wl/wr: n rows of [rho, vx, vy, vz, P, sie] (dust: the first four); out: n rows of
// [frho, fmx, fmy, fmz, fe, feg, face pressure, face velocity] (dust: the first four, the rest 0).
int ref_riemann(int fluid, int solver, double gm1, long n, const double *wl, const double *wr, double *out) {
  if (fluid == 0 && solver == 0) riemann_table<RSolver::hllc, Fluid::gas>(gm1, n, wl, wr, out);
  else if (fluid == 0 && solver == 1) riemann_table<RSolver::hlle, Fluid::gas>(gm1, n, wl, wr, out);
  else if (fluid == 0 && solver == 2) riemann_table<RSolver::llf, Fluid::gas>(gm1, n, wl, wr, out);
  else if (fluid == 1 && solver == 1) riemann_table<RSolver::hlle, Fluid::dust>(gm1, n, wl, wr, out);
  else if (fluid == 1 && solver == 2) riemann_table<RSolver::llf, Fluid::dust>(gm1, n, wl, wr, out);
  else return 1;
  return 0;
}

// geom = {x1 of face 0, dx1, x2 of face 0, dx2, x3 of face 0, dx3}; out: n rows of NCOORD doubles:
// Volume, lower AreaX1..3, x1v..x3v, hx1v..hx3v, dh{1,2,3}dx1, dh{1,2,3}dx2, dh{1,2,3}dx3, cell widths X1..X3,
// hx1..3 at the lower X1, X2 and X3 face centres.
int ref_coords(int system, const double *geom, const int *k, const int *j, const int *i, long n, double *out) {
  Coordinates_t co;
  for (int d = 0; d < 3; ++d) co.x0[d] = geom[2 * d], co.dx[d] = geom[2 * d + 1];
  for (long c = 0; c < n; ++c) {
    double *o = out + c * NCOORD;
    switch (static_cast<Coordinates>(system)) {
    case Coordinates::cartesian: coords_cell<Coordinates::cartesian>(co, k[c], j[c], i[c], o); break;
    case Coordinates::cylindrical: coords_cell<Coordinates::cylindrical>(co, k[c], j[c], i[c], o); break;
    case Coordinates::spherical1D: coords_cell<Coordinates::spherical1D>(co, k[c], j[c], i[c], o); break;
    case Coordinates::spherical2D: coords_cell<Coordinates::spherical2D>(co, k[c], j[c], i[c], o); break;
    case Coordinates::spherical3D: coords_cell<Coordinates::spherical3D>(co, k[c], j[c], i[c], o); break;
    case Coordinates::axisymmetric: coords_cell<Coordinates::axisymmetric>(co, k[c], j[c], i[c], o); break;
    default: return 1;
    }
  }
  return 0;
}

// One block of nx interior zones and ng ghost zones in every active direction.  prim: [6 or 4 times nsp][nk][nj][ni].
// flux[d]: same shape; pflux[d], vface[d]: [nsp][nk][nj][ni] (gas only, may be null for dust); hface[d]:
// [3][nk][nj][ni], the factors of ScaleMomentumFlux for the faces of direction d.  Unwritten cells keep their values.
int ref_sweep(int system, int fluid, int recon, int solver, double gm1, int nsp, const int *nx, int ng,
              const double *geom, const double *prim, double *const *flux, double *const *pflux,
              double *const *vface, double *const *hface) {
  const Block B(nx, ng, geom);
  switch (static_cast<Coordinates>(system)) {
#define REF_SWEEP_CASE(G)                                                                                              \
  case Coordinates::G:                                                                                                 \
    return sweep_solver<Coordinates::G>(fluid, solver, recon, B, gm1, nsp, prim, flux, pflux, vface, hface);
    REF_SWEEP_CASE(cartesian)
    REF_SWEEP_CASE(cylindrical)
    REF_SWEEP_CASE(spherical1D)
    REF_SWEEP_CASE(spherical2D)
    REF_SWEEP_CASE(spherical3D)
    REF_SWEEP_CASE(axisymmetric)
#undef REF_SWEEP_CASE
  default: return 1;
  }
}

} // extern "C"
