// =======================================================================================
// oracle/artemis_oracle.cpp  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// A plain-array CPU restatement of the lanl/artemis finite-volume hydro update
// (reference @ 2025-01-17).  Only tests/, __graft_entry__.smoke() and bench.py's
// `cpu_baseline` leg may load this library; the product path (artemis_amd/, HIP) never does.
//
// Every function cites the reference file:line whose arithmetic it restates (paths are
// relative to the reference's src/).  Expression trees follow the reference left-to-right
// so that, compiled with -ffp-contract=off, results are reproducible bit-for-bit by an
// independent implementation that uses the same trees.
//
// Pinning (see DESIGN.md "Oracle"): the reference executable cannot be built here (its
// Parthenon/Kokkos/singularity-eos submodules are empty), so this oracle is pinned against
// the known answers the reference's own regression tests hold for this path:
//   * tst/scripts/hydro/linwave.py:98-143   (RMS-L1 magnitudes, convergence, L==R bitwise)
//   * tst/scripts/advection/advection.py:100-187 (dt, cycle count, history integrals, errors)
//   * tst/scripts/coords/blast.py:118,177-183 (Sedov pressure L2 < 1)
// No single-face golden vectors exist in the reference; per-face flux values are pinned only
// through those end-to-end answers.
//
// Third-party arithmetic absent from /root/reference (versions unpinned, restated from the
// published algorithms and the reference's call sites):
//   singularity-eos IdealGas: Gruneisen = gm1; P = gm1*rho*sie; B = (gm1+1)*gm1*rho*sie
//   parthenon: UniformCartesian Xf(i) = xmin + i*dx; LowStorageIntegrator coefficients;
//              outflow/reflecting/periodic ghost fill; dt <= 2*dt_old and tlim clipping.
//
// Layout: SoA [var][k][j][i], i fastest, ng ghost cells in every active dimension.
// =======================================================================================
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include <omp.h>
#include <cstring>
#include <memory>

typedef double Real;
#define SQR(x) ((x) * (x))

extern "C" {
// Enumerations use the reference's order (artemis.hpp:78-90).
enum { RS_HLLC = 0, RS_HLLE = 1, RS_LLF = 2 };
enum { RC_PCM = 0, RC_PLM = 1, RC_PPM = 2 };
enum { FL_GAS = 0, FL_DUST = 1 };
enum { BC_PERIODIC = 0, BC_OUTFLOW = 1, BC_REFLECT = 2, BC_NONE = 3, BC_STRAT_EXTRAP = 4,
       BC_STRAT_INFLOW = 5, BC_CONDUCTIVE = 6, BC_DISK_IC = 7, BC_DISK_EXTRAP = 8, BC_DISK_VISC = 9 }; // 4/5: the `strat` pgen's user conditions (problem_modifier.hpp:114-128)
enum { INT_RK1 = 0, INT_RK2 = 1, INT_VL2 = 2, INT_RK3 = 3 };

struct oracle_cfg {
  int nx1, nx2, nx3, ng;
  double x1min, x1max, x2min, x2max, x3min, x3max; // interior bounds of this block
  int ns_gas, ns_dust;                             // 0 disables the fluid
  int recon_gas, riemann_gas, recon_dust, riemann_dust;
  double gamma, dfloor_gas, siefloor_gas, de_switch, dfloor_dust;
  double cfl_gas, cfl_dust;
  int bc[6]; // ix1, ox1, ix2, ox2, ix3, ox3
  int integrator;
  int nthreads;
  int coords; // artemis.hpp:78-86 order: cartesian, cylindrical, spherical1D/2D/3D, axisymmetric
};
}

namespace {

// Field storage: a vector whose resize() leaves new elements uninitialised, so that the pages of the big
// arrays are first touched by the OpenMP threads that later sweep them (first_touch() below) instead of by
// the constructing thread -- on a multi-socket host the serial zero-fill of std::vector would put every
// page on one NUMA node.  Test infrastructure only; no effect on results.
template <class T>
struct NoInitAlloc : std::allocator<T> {
  template <class U>
  struct rebind {
    typedef NoInitAlloc<U> other;
  };
  template <class U>
  void construct(U *) noexcept {}
  template <class U, class A0, class... A>
  void construct(U *p, A0 &&a0, A &&...a) {
    ::new (static_cast<void *>(p)) U(std::forward<A0>(a0), std::forward<A>(a)...);
  }
};
typedef std::vector<double, NoInitAlloc<double>> RVec;

struct Sim {
  oracle_cfg c;
  int ndim, ni, nj, nk, is, ie, js, je, ks, ke;
  size_t N;
  Real f0[3], dx[3]; // Xf(d, idx) = f0[d] + idx*dx[d]   (parthenon UniformCartesian, recalled)
  int nvg, nvd;      // 6*ns_gas, 4*ns_dust
  // gas
  RVec gprim, gu0, gu1, gflux[3], gpflux[3], gvface[3];
  // dust
  RVec dprim, du0, du1, dflux[3];
  // driver state
  Real time, dt;
  long ncycle;
  // problem parameters kept for the error norms
  Real lw_amp, lw_vflow, lw_lambda, lw_d0, lw_p0, lw_v1_0, lw_k_par;
  Real lw_cos_a2, lw_cos_a3, lw_sin_a2, lw_sin_a3, lw_rem[5][5], lw_ev[5], lw_gamma, lw_gm1;
  int lw_wave_flag;
  Real gx1min, gx1max, gx2min, gx2max, gx3min, gx3max; // global mesh bounds for pgens
  // optional source packages (artemis.cpp:63-72); zero-initialised = disabled
  struct {
    int type = 0; // 0 off, 1 uniform, 2 point, 3 binary
    Real g[3] = {0, 0, 0}, gm = 0, soft = 0, sink = 0, sink_rate = 0, pos[3] = {0, 0, 0};
    // binary (gravity.cpp:77-111): mass ratio, second body's softening / sink, Orbit (gravity.hpp:30-65)
    Real q = 0, soft2 = 0, sink2 = 0, sink_rate2 = 0;
    Real a = 1, e = 0, n = 0, coso = 1, sino = 0, cosO = 1, sinO = 0, cosI = 1, sinI = 0, cosf0 = -1, sinf0 = 0;
    bool given_pos = false; // a caller supplies pos (body 1) and pos2 itself instead of the orbit
    Real pos2[3] = {0, 0, 0};
    Real tstart = std::numeric_limits<Real>::lowest(), tstop = std::numeric_limits<Real>::max();
  } grav;
  struct {
    bool on = false;
    Real omega = 0, qshear = 0;
  } rframe;
  // <gravity/nbody>: the particles of the nbody package as NBodyGravity sees them (nbody/particle_base.hpp:53-93)
  struct NBodyParticle {
    Real GM = 0, pos[3] = {0, 0, 0}, vel[3] = {0, 0, 0}, xf[3] = {0, 0, 0}, vf[3] = {0, 0, 0};
    Real rs = 0, racc = 0, gamma = 0, beta = 0;
    int spline = 0, couple = 1;
  };
  std::vector<NBodyParticle> nbody;
  bool nbody_frame_correction = true; // <nbody> frame = global (nbody.cpp:97,109)
  std::vector<Real> pforce;           // [npart][7], accumulated by every NBodyGravity call (nbody_gravity.hpp:210-212)
  struct SelfDrag { // drag.hpp:68-117 SelfDragParams
    Real ix[3], ox[3], irate[3], orate[3];
    SelfDrag() {
      for (int i = 0; i < 3; i++) {
        ix[i] = -std::numeric_limits<Real>::max(), ox[i] = std::numeric_limits<Real>::max();
        irate[i] = 0.0, orate[i] = 0.0;
      }
    }
  };
  struct {
    int type = 0;  // 0 off, 1 simple_dust, 2 self
    int model = 0; // 0 constant, 1 stokes (drag.hpp:58)
    Real scale = 1.0, grain_density = 1.0;
    std::vector<Real> tau, sizes;
    SelfDrag gas, dust;
    bool damp_to_visc = false; // gas damping relaxes towards the viscous inflow velocity (drag.cpp:109,135)
  } drag;
  struct { // pgen/strat.hpp:44-52 (only what the user BCs read)
    Real q = 0, Om0 = 0;
  } strat;
  struct { // pgen/conduction.hpp:30-37 CondParams (what the `conductive` conditions read)
    Real g_temp = 1, flux = 0;
  } condbc;
  struct DiskParams { // pgen/disk.hpp:50-66 (nbody_temp = false: n-body is out of scope)
    Real r0 = 1, h0 = 0.05, p = -2.25, q = -0.5, flare = 0.25;
    Real rho0 = 1, dens_min = 1e-5, pres_min = 1e-8;
    Real gm = 1, Omega0 = 1, l0 = 0, omf = 0, dust_to_gas = 0.01, rexp = 0, rcav = 0;
    Real Gamma = 1, gamma_gas = 1.4, alpha = 0, nu0 = 0, nu_indx = 0, mdot = 0, temp_soft2 = 0;
    bool quiet_start = false;
  } disk;
  struct { // gas/cooling/cooling.cpp:34-88: beta cooling towards a power-law reference temperature
    bool on = false;
    Real beta0 = 0, beta_min = 1e-12, escale = 0, tfloor = 0, tcyl = 0, cyl_plaw = 0, tsph = 0, sph_plaw = 0;
  } cool;
  // optional: initial primitives kept by a caller; when present the `ic` condition copies ghost
  // zones from here instead of re-evaluating the profile (same values: the profile is static)
  RVec ic_g, ic_d;
  // diffusion (utils/diffusion/diffusion_coeff.hpp:58-136 DiffCoeffParams); type 0 = package off
  struct DiffCoeff {
    int type = 0; // 1 viscosity_plaw, 2 viscosity_alpha, 3 conductivity_plaw, 4 thermaldiff_plaw
    int avg = 0;  // 0 arithmetic, 1 harmonic
    Real nu_s = 0, eta = 0, r_exp = 0, R0 = 1, alpha = 0, Omega0 = 0;
    Real kappa_0 = 0, hcond_0 = 0, temp_exp = 0, rho_exp = 0, d0 = 1, T0 = 1;
  };
  DiffCoeff visc, cond;
  Real cv = 0; // IdealGas Cv = kB / ((gamma-1) amu mu), gas.cpp:106-116 (set at creation)
  RVec qflux[3]; // gas::diff::momentum (3n+d) and gas::diff::energy (3ns+n) face fluxes
};

inline size_t IDX(const Sim &s, int k, int j, int i) {
  return (static_cast<size_t>(k) * s.nj + j) * s.ni + i;
}
inline Real *V(RVec &a, const Sim &s, int n) { return a.data() + n * s.N; }
inline const Real *V(const RVec &a, const Sim &s, int n) {
  return a.data() + n * s.N;
}

// geometry/geometry.hpp:65-72 (BBox from Coordinates_t::Xf), Cartesian only.
struct BBox {
  Real x1[2], x2[2], x3[2];
};
inline BBox bbox(const Sim &s, int k, int j, int i) {
  BBox b;
  b.x1[0] = s.f0[0] + i * s.dx[0];
  b.x1[1] = s.f0[0] + (i + 1) * s.dx[0];
  b.x2[0] = s.f0[1] + j * s.dx[1];
  b.x2[1] = s.f0[1] + (j + 1) * s.dx[1];
  b.x3[0] = s.f0[2] + k * s.dx[2];
  b.x3[1] = s.f0[2] + (k + 1) * s.dx[2];
  return b;
}
// geometry/geometry.hpp:219-225
inline Real volume(const BBox &b) {
  const Real dx1 = b.x1[1] - b.x1[0];
  const Real dx2 = b.x2[1] - b.x2[0];
  const Real dx3 = b.x3[1] - b.x3[0];
  return dx1 * dx2 * dx3;
}
// geometry/geometry.hpp:199-216
inline Real area1(const BBox &b) { return (b.x2[1] - b.x2[0]) * (b.x3[1] - b.x3[0]); }
inline Real area2(const BBox &b) { return (b.x1[1] - b.x1[0]) * (b.x3[1] - b.x3[0]); }
inline Real area3(const BBox &b) { return (b.x1[1] - b.x1[0]) * (b.x2[1] - b.x2[0]); }
// geometry/geometry.hpp:163-166
inline Real x1v(const BBox &b) { return 0.5 * (b.x1[0] + b.x1[1]); }
inline Real x2v(const BBox &b) { return 0.5 * (b.x2[0] + b.x2[1]); }
inline Real x3v(const BBox &b) { return 0.5 * (b.x3[0] + b.x3[1]); }


// ---------------------------------------------------------------------------------------
// geometry::Coords<GEOM> (geometry.hpp:145-420 base = Cartesian defaults; cylindrical.hpp:28-80;
// spherical.hpp:36-146 (3D), :240-345 (2D), :441-512 (1D); axisymmetric.hpp:27-75).  The
// reference uses CRTP classes; here one class switches on the runtime enum and every method
// restates the expression of the class that overrides it (or the base default).
enum { CO_CART = 0, CO_CYL = 1, CO_SPH1D = 2, CO_SPH2D = 3, CO_SPH3D = 4, CO_AXI = 5 };
struct Coords {
  int sys;
  BBox bnds;
  Coords(const Sim &s, int k, int j, int i);
  bool sph23() const { return sys == CO_SPH2D || sys == CO_SPH3D; }
  bool sph() const { return sys == CO_SPH1D || sph23(); }
  // geometry.hpp:98-110
  bool x1dep() const { return sph() || sys == CO_CYL || sys == CO_AXI; }
  bool x2dep() const { return sph23(); }
  bool x3dep() const { return false; }

  Real x1v() const {
    if (sph()) { // spherical.hpp:57-60, :261-264, :458-461
      const Real dr2 = bnds.x1[0] * bnds.x1[0] + bnds.x1[1] * bnds.x1[1];
      return 0.75 * (bnds.x1[0] + bnds.x1[1]) * dr2 / (dr2 + bnds.x1[0] * bnds.x1[1]);
    }
    if (sys == CO_CYL || sys == CO_AXI) // cylindrical.hpp:41-45, axisymmetric.hpp:38-42
      return 2.0 / 3.0 *
             (bnds.x1[0] * bnds.x1[0] + bnds.x1[0] * bnds.x1[1] + bnds.x1[1] * bnds.x1[1]) /
             (bnds.x1[0] + bnds.x1[1]);
    return 0.5 * (bnds.x1[0] + bnds.x1[1]); // geometry.hpp:163
  }
  Real x2v() const {
    if (sph23()) { // spherical.hpp:61-68, :265-270
      const Real ctm = std::cos(bnds.x2[0]);
      const Real ctp = std::cos(bnds.x2[1]);
      const Real dst = std::sin(bnds.x2[1]) - std::sin(bnds.x2[0]);
      return (dst - bnds.x2[1] * ctp + bnds.x2[0] * ctm) / std::abs(ctm - ctp);
    }
    return 0.5 * (bnds.x2[0] + bnds.x2[1]);
  }
  Real x3v() const { return 0.5 * (bnds.x3[0] + bnds.x3[1]); }

  Real hx1(Real, Real, Real) const { return 1.0; }
  Real hx2(Real x1, Real, Real) const { // spherical.hpp:50,254,454; cylindrical.hpp:47
    return (sph() || sys == CO_CYL) ? x1 : 1.0;
  }
  Real hx3(Real x1, Real x2, Real) const {
    if (sph23()) return x1 * std::sin(x2); // spherical.hpp:53-55, :257-259
    if (sys == CO_AXI) return x1;          // axisymmetric.hpp:43-45
    return 1.0;                            // spherical1D and cylindrical keep the base default
  }
  Real hx1v() const { return 1.0; }
  Real hx2v() const { // spherical.hpp:70,274; cylindrical.hpp:51 (spherical1D: base default)
    return (sph23() || sys == CO_CYL) ? x1v() : 1.0;
  }
  Real hx3v() const {
    if (sph23()) { // spherical.hpp:71-82, :275-286
      const Real ctm = std::cos(bnds.x2[0]);
      const Real ctp = std::cos(bnds.x2[1]);
      const Real stm = std::sin(bnds.x2[0]);
      const Real stp = std::sin(bnds.x2[1]);
      const Real dsc = stp * ctp - stm * ctm;
      const Real dx2 = bnds.x2[1] - bnds.x2[0];
      return x1v() * 0.5 * (dx2 - dsc) / std::abs(ctm - ctp);
    }
    if (sys == CO_AXI) return x1v(); // axisymmetric.hpp:46
    return 1.0;
  }
  Real rcen() const { // the 2/3 (r0^2+r0r1+r1^2)/(r0+r1) face-centroid radius
    return 2.0 / 3.0 *
           (bnds.x1[0] * bnds.x1[0] + bnds.x1[0] * bnds.x1[1] + bnds.x1[1] * bnds.x1[1]) /
           (bnds.x1[0] + bnds.x1[1]);
  }
  // geometry.hpp:182-197 defaults; overrides spherical.hpp:88-104, :288-304, :463-479,
  // cylindrical.hpp:53-60 (X3 only), axisymmetric.hpp:47-54 (X2 only)
  void FaceCenX1(int f, Real xf[3]) const {
    xf[0] = bnds.x1[f];
    xf[1] = x2v();
    xf[2] = x3v();
  }
  void FaceCenX2(int f, Real xf[3]) const {
    if (sys == CO_SPH3D || sys == CO_AXI) {
      xf[0] = rcen(), xf[1] = bnds.x2[f], xf[2] = 0.5 * (bnds.x3[0] + bnds.x3[1]);
    } else if (sys == CO_SPH2D) {
      xf[0] = rcen(), xf[1] = bnds.x2[f], xf[2] = 0.0;
    } else if (sys == CO_SPH1D) {
      xf[0] = rcen(), xf[1] = M_PI * 0.5, xf[2] = 0.0;
    } else {
      xf[0] = x1v(), xf[1] = bnds.x2[f], xf[2] = x3v();
    }
  }
  void FaceCenX3(int f, Real xf[3]) const {
    if (sys == CO_SPH3D || sys == CO_CYL) {
      xf[0] = rcen(), xf[1] = 0.5 * (bnds.x2[0] + bnds.x2[1]), xf[2] = bnds.x3[f];
    } else if (sys == CO_SPH2D) {
      xf[0] = rcen(), xf[1] = 0.5 * (bnds.x2[0] + bnds.x2[1]), xf[2] = 0.0;
    } else if (sys == CO_SPH1D) {
      xf[0] = rcen(), xf[1] = M_PI * 0.5, xf[2] = 0.0;
    } else {
      xf[0] = x1v(), xf[1] = x2v(), xf[2] = bnds.x3[f];
    }
  }
  Real AreaX1(const Real x1f) const {
    const Real dx2 = bnds.x2[1] - bnds.x2[0];
    const Real dx3 = bnds.x3[1] - bnds.x3[0];
    switch (sys) {
    case CO_SPH3D: // spherical.hpp:106-109
      return x1f * x1f * std::abs(std::cos(bnds.x2[0]) - std::cos(bnds.x2[1])) * dx3;
    case CO_SPH2D: // :306-308
      return x1f * x1f * std::abs(std::cos(bnds.x2[0]) - std::cos(bnds.x2[1]));
    case CO_SPH1D: // :481-483
      return x1f * x1f;
    case CO_CYL: // cylindrical.hpp:62-66
    case CO_AXI: // axisymmetric.hpp:55-59
      return x1f * dx2 * dx3;
    default:
      return dx2 * dx3; // geometry.hpp:199-204
    }
  }
  Real AreaX2(const Real x2f) const {
    const Real dx1 = bnds.x1[1] - bnds.x1[0];
    const Real dx3 = bnds.x3[1] - bnds.x3[0];
    switch (sys) {
    case CO_SPH3D: // spherical.hpp:110-114
      return 0.5 * (bnds.x1[1] + bnds.x1[0]) * std::sin(x2f) * dx1 * dx3;
    case CO_SPH2D: // :309-312
      return 0.5 * (bnds.x1[1] + bnds.x1[0]) * std::sin(x2f) * dx1;
    case CO_SPH1D: // :484-487
      return 0.5 * (bnds.x1[1] + bnds.x1[0]) * dx1;
    case CO_AXI: // axisymmetric.hpp:60-64
      return (bnds.x1[0] + bnds.x1[1]) * 0.5 * dx1 * dx3;
    default: // cylindrical keeps the base (geometry.hpp:205-210)
      return dx1 * dx3;
    }
  }
  Real AreaX3(const Real) const {
    const Real dx1 = bnds.x1[1] - bnds.x1[0];
    const Real dx2 = bnds.x2[1] - bnds.x2[0];
    switch (sys) {
    case CO_SPH3D: // spherical.hpp:115-119, :313-317
    case CO_SPH2D:
    case CO_CYL: // cylindrical.hpp:67-71
      return 0.5 * (bnds.x1[0] + bnds.x1[1]) * dx1 * dx2;
    case CO_SPH1D: // spherical.hpp:488-491
      return 0.5 * (bnds.x1[0] + bnds.x1[1]) * dx1;
    default: // axisymmetric keeps the base (geometry.hpp:211-216)
      return dx1 * dx2;
    }
  }
  Real Volume() const {
    const Real dx1 = bnds.x1[1] - bnds.x1[0];
    const Real dx2 = bnds.x2[1] - bnds.x2[0];
    const Real dx3 = bnds.x3[1] - bnds.x3[0];
    if (sph()) { // spherical.hpp:124-133, :319-326, :493-499
      const Real rfac =
          (bnds.x1[0] * bnds.x1[0] + bnds.x1[0] * bnds.x1[1] + bnds.x1[1] * bnds.x1[1]) / 3.0;
      if (sys == CO_SPH1D) return rfac * dx1;
      const Real dc = std::abs(std::cos(bnds.x2[0]) - std::cos(bnds.x2[1]));
      if (sys == CO_SPH2D) return rfac * dx1 * dc;
      return rfac * dx1 * dc * dx3;
    }
    if (sys == CO_CYL || sys == CO_AXI) // cylindrical.hpp:73-78, axisymmetric.hpp:65-70
      return (bnds.x1[0] + bnds.x1[1]) * 0.5 * dx1 * dx2 * dx3;
    return dx1 * dx2 * dx3; // geometry.hpp:219-225
  }
  // connection coefficients (geometry.hpp:236-246 zero defaults)
  Real dh2dx1() const {
    if (sph()) // spherical.hpp:135-138, :328-331, :501-504
      return 3.0 / 2.0 * (bnds.x1[0] + bnds.x1[1]) /
             (bnds.x1[0] * bnds.x1[0] + bnds.x1[0] * bnds.x1[1] + bnds.x1[1] * bnds.x1[1]);
    if (sys == CO_CYL) return 1.0 / (0.5 * (bnds.x1[0] + bnds.x1[1])); // cylindrical.hpp:80
    return 0.0;
  }
  Real dh3dx1() const {
    if (sph()) // spherical.hpp:139-142, :332-335, :505-508
      return 3.0 / 2.0 * (bnds.x1[0] + bnds.x1[1]) /
             (bnds.x1[0] * bnds.x1[0] + bnds.x1[0] * bnds.x1[1] + bnds.x1[1] * bnds.x1[1]);
    if (sys == CO_AXI) return 1.0 / (0.5 * (bnds.x1[0] + bnds.x1[1])); // axisymmetric.hpp:71
    return 0.0;
  }
  Real dh3dx2() const {
    if (sph23()) // spherical.hpp:143-146, :336-339
      return (std::sin(bnds.x2[1]) - std::sin(bnds.x2[0])) /
             std::abs(std::cos(bnds.x2[0]) - std::cos(bnds.x2[1]));
    return 0.0;
  }
  // aggregate helpers, geometry.hpp:330-420
  void GetCellWidths(Real w[3]) const {
    const Real xv[3] = {x1v(), x2v(), x3v()};
    w[0] = hx1(xv[0], xv[1], xv[2]) * (bnds.x1[1] - bnds.x1[0]);
    w[1] = hx2(xv[0], xv[1], xv[2]) * (bnds.x2[1] - bnds.x2[0]);
    w[2] = hx3(xv[0], xv[1], xv[2]) * (bnds.x3[1] - bnds.x3[0]);
  }
  void GetScaleFactors(Real h[3]) const { h[0] = hx1v(), h[1] = hx2v(), h[2] = hx3v(); }
  void GetFaceAreaX1(Real a[2]) const { a[0] = AreaX1(bnds.x1[0]), a[1] = AreaX1(bnds.x1[1]); }
  void GetFaceAreaX2(Real a[2]) const { a[0] = AreaX2(bnds.x2[0]), a[1] = AreaX2(bnds.x2[1]); }
  void GetFaceAreaX3(Real a[2]) const { a[0] = AreaX3(bnds.x3[0]), a[1] = AreaX3(bnds.x3[1]); }
  void GetConnX1(Real c[3]) const { c[0] = 0.0, c[1] = dh2dx1(), c[2] = dh3dx1(); }
  void GetConnX2(Real c[3]) const { c[0] = 0.0, c[1] = 0.0, c[2] = dh3dx2(); }
  // ConvertCoordsToCart: spherical.hpp:166-173 (3D), :355-362 (2D), :528-534 (1D);
  // cylindrical.hpp:88-92; axisymmetric.hpp:77-82; identity for Cartesian (geometry.hpp:248)
  void ConvertToCart(const Real xi[3], Real xc[3]) const {
    if (sys == CO_SPH3D || sys == CO_SPH2D) {
      const Real cp = (sys == CO_SPH3D) ? std::cos(xi[2]) : 1.0;
      const Real sp = (sys == CO_SPH3D) ? std::sin(xi[2]) : 0.0;
      const Real ct = std::cos(xi[1]);
      const Real st = std::sin(xi[1]);
      xc[0] = xi[0] * st * cp, xc[1] = xi[0] * st * sp, xc[2] = xi[0] * ct;
    } else if (sys == CO_SPH1D) {
      const Real cp = 1.0, sp = 0.0, ct = 0.0, st = 1.0;
      xc[0] = xi[0] * st * cp, xc[1] = xi[0] * st * sp, xc[2] = xi[0] * ct;
    } else if (sys == CO_CYL) {
      const Real cp = std::cos(xi[1]);
      const Real sp = std::sin(xi[1]);
      xc[0] = xi[0] * cp, xc[1] = xi[0] * sp, xc[2] = xi[2];
    } else if (sys == CO_AXI) {
      const Real cp = std::cos(xi[2]);
      const Real sp = std::sin(xi[2]);
      xc[0] = xi[0] * cp, xc[1] = xi[0] * sp, xc[2] = xi[1];
    } else {
      xc[0] = xi[0], xc[1] = xi[1], xc[2] = xi[2];
    }
  }
};
inline Coords::Coords(const Sim &s, int k, int j, int i) : sys(s.c.coords), bnds(bbox(s, k, j, i)) {}

// ---------------------------------------------------------------------------------------
// Reconstruction
// utils/fluxes/reconstruction/plm.hpp:32-47
inline void PLM(const Real q_im1, const Real q_i, const Real q_ip1, Real &ql_ip1, Real &qr_i) {
  Real dql = (q_i - q_im1);
  Real dqr = (q_ip1 - q_i);
  Real dq2 = dql * dqr;
  Real dqm = dq2 / (dql + dqr);
  if (dq2 <= 0.0) dqm = 0.0;
  ql_ip1 = q_i + dqm;
  qr_i = q_i - dqm;
}
// utils/fluxes/reconstruction/ppm.hpp:33-66
inline void PPM4(const Real q_im2, const Real q_im1, const Real q_i, const Real q_ip1,
                 const Real q_ip2, Real &ql_ip1, Real &qr_i) {
  Real qlv = (7. * (q_i + q_im1) - (q_im2 + q_ip1)) / 12.0;
  Real qrv = (7. * (q_i + q_ip1) - (q_im1 + q_ip2)) / 12.0;
  qlv = std::max(qlv, std::min(q_i, q_im1));
  qlv = std::min(qlv, std::max(q_i, q_im1));
  qrv = std::max(qrv, std::min(q_i, q_ip1));
  qrv = std::min(qrv, std::max(q_i, q_ip1));
  Real qc = qrv - q_i;
  Real qd = qlv - q_i;
  if ((qc * qd) >= 0.0) {
    qlv = q_i;
    qrv = q_i;
  } else {
    if (std::fabs(qc) >= 2.0 * std::fabs(qd)) {
      qrv = q_i - 2.0 * qd;
    }
    if (std::fabs(qd) >= 2.0 * std::fabs(qc)) {
      qlv = q_i - 2.0 * qc;
    }
  }
  ql_ip1 = qrv;
  qr_i = qlv;
}

// utils/fluxes/reconstruction/plm.hpp:54-73  (Mignone 2013 weights)
inline void PLM_G(const Real q_im1, const Real q_i, const Real q_ip1, Real &ql_ip1, Real &qr_i,
                  const Real x_im1, const Real x_i, const Real x_ip1, const Real xf[2],
                  const Real dx) {
  const Real dql = (q_i - q_im1) * dx / (x_i - x_im1);
  const Real dqr = (q_ip1 - q_i) * dx / (x_ip1 - x_i);
  const Real dq2 = dql * dqr;
  const Real cr = (x_ip1 - x_i) / (xf[1] - x_i);
  const Real cl = (x_i - x_im1) / (x_i - xf[0]);
  const Real dqm = (dq2 <= 0.0) ? 0.0
                                : dq2 * (cr * dql + cl * dqr) /
                                      (dql * dql + dqr * dqr + dq2 * (cl + cr - 2.0));
  ql_ip1 = q_i + dqm * (xf[1] - x_i) / dx;
  qr_i = q_i - dqm * (x_i - xf[0]) / dx;
}
// Centroids, face pair and physical width PLM_G receives for cell (k,j,i) along `dir`
// (plm.hpp:93-101, :127-135, :161-169).
struct PlmGeo {
  Real xvm, xvc, xvp, xf[2], dx;
};
inline PlmGeo plm_geo(const Sim &s, int dir, int k, int j, int i) {
  PlmGeo g;
  const int dk = (dir == 3), dj = (dir == 2), di = (dir == 1);
  Coords cm(s, k - dk, j - dj, i - di), cc(s, k, j, i), cp(s, k + dk, j + dj, i + di);
  Real w[3];
  cc.GetCellWidths(w);
  if (dir == 1) {
    g.xvm = cm.x1v(), g.xvc = cc.x1v(), g.xvp = cp.x1v();
    g.xf[0] = cc.bnds.x1[0], g.xf[1] = cc.bnds.x1[1];
  } else if (dir == 2) {
    g.xvm = cm.x2v(), g.xvc = cc.x2v(), g.xvp = cp.x2v();
    g.xf[0] = cc.bnds.x2[0], g.xf[1] = cc.bnds.x2[1];
  } else {
    g.xvm = cm.x3v(), g.xvc = cc.x3v(), g.xvp = cp.x3v();
    g.xf[0] = cc.bnds.x3[0], g.xf[1] = cc.bnds.x3[1];
  }
  g.dx = w[dir - 1];
  return g;
}

// One row of reconstruction along a stride: cells c in [lo,hi] write wl[c+1], wr[c]
// (pcm.hpp:34-88, plm.hpp:82-175, ppm.hpp:75-130).  `q` points at cell index 0 of the row
// along the sweep direction, `st` is the stride between consecutive cells of the sweep.
inline void recon_cell(int recon, const Real *q, ptrdiff_t st, Real &ql_next, Real &qr_here,
                       const PlmGeo *g = nullptr) {
  if (recon == RC_PCM) {
    ql_next = q[0];
    qr_here = q[0];
  } else if (recon == RC_PLM) {
    if (g == nullptr) // GEOM == cartesian (plm.hpp:90)
      PLM(q[-st], q[0], q[st], ql_next, qr_here);
    else
      PLM_G(q[-st], q[0], q[st], ql_next, qr_here, g->xvm, g->xvc, g->xvp, g->xf, g->dx);
  } else {
    PPM4(q[-2 * st], q[-st], q[0], q[st], q[2 * st], ql_next, qr_here);
  }
}

// ---------------------------------------------------------------------------------------
// Riemann solvers.  wl/wr hold the face states of one face: [IDN, ivx, ivy, ivz, IPR, ISE].
// Outputs: f[0..5] = mass, normal mom, t1 mom, t2 mom, total E, internal E; pf; vf.
struct FaceOut {
  Real fd, fmx, fmy, fmz, fe, feg, pf, vf;
};

// utils/fluxes/riemann/hllc.hpp:50-182
inline void hllc_gas(const Real gm1, const Real wl_idn, const Real wl_ivx, const Real wl_ivy,
                     const Real wl_ivz, const Real wl_ipr, const Real wl_ise, const Real wr_idn,
                     const Real wr_ivx, const Real wr_ivy, const Real wr_ivz, const Real wr_ipr,
                     const Real wr_ise, FaceOut &o) {
  Real igm1 = 1.0 / gm1;
  Real gamma = gm1 + 1.0;
  Real alpha = (gamma + 1.0) / (2.0 * gamma);
  Real qa, qb, qc, qd, qe, qf;
  qa = std::sqrt(gamma * wl_ipr / wl_idn);
  qb = std::sqrt(gamma * wr_ipr / wr_idn);
  Real el = wl_ipr * igm1 + 0.5 * wl_idn * (SQR(wl_ivx) + SQR(wl_ivy) + SQR(wl_ivz));
  Real er = wr_ipr * igm1 + 0.5 * wr_idn * (SQR(wr_ivx) + SQR(wr_ivy) + SQR(wr_ivz));
  qc = 0.25 * (wl_idn + wr_idn) * (qa + qb);
  qd = 0.5 * (wl_ipr + wr_ipr + (wl_ivx - wr_ivx) * qc);
  qe = (qd <= wl_ipr) ? 1.0 : std::sqrt(1.0 + alpha * ((qd / wl_ipr) - 1.0));
  qf = (qd <= wr_ipr) ? 1.0 : std::sqrt(1.0 + alpha * ((qd / wr_ipr) - 1.0));
  Real sl = wl_ivx - qa * qe;
  Real sr = wr_ivx + qb * qf;
  qa = sr > 0.0 ? sr : 1.0e-20;  // bp
  qb = sl < 0.0 ? sl : -1.0e-20; // bm
  qe = wl_ivx - sl;
  qf = wr_ivx - sr;
  qc = wl_ipr + qe * wl_idn * wl_ivx;
  qd = wr_ipr + qf * wr_idn * wr_ivx;
  Real ml = wl_idn * qe;
  Real mr = -(wr_idn * qf);
  Real am = (qc - qd) / (ml + mr);
  Real cp = (ml * qd + mr * qc) / (ml + mr);
  cp = cp > 0.0 ? cp : 0.0;
  qe = wl_idn * (wl_ivx - qb);
  qf = wr_idn * (wr_ivx - qa);
  Real fld = qe;
  Real frd = qf;
  Real flmx = qe * wl_ivx;
  Real frmx = qf * wr_ivx;
  Real flmy = qe * wl_ivy;
  Real frmy = qf * wr_ivy;
  Real flmz = qe * wl_ivz;
  Real frmz = qf * wr_ivz;
  Real fle = el * (wl_ivx - qb) + wl_ipr * wl_ivx;
  Real fre = er * (wr_ivx - qa) + wr_ipr * wr_ivx;
  if (am >= 0.0) {
    qc = am / (am - qb);
    qd = 0.0;
    qe = -qb / (am - qb);
  } else {
    qc = 0.0;
    qd = -am / (qa - am);
    qe = qa / (qa - am);
  }
  o.pf = qc * wl_ipr + qd * wr_ipr + qe * cp;
  const Real frho = qc * fld + qd * frd;
  o.fd = frho;
  o.fmx = qc * flmx + qd * frmx;
  o.fmy = qc * flmy + qd * frmy;
  o.fmz = qc * flmz + qd * frmz;
  o.fe = qc * fle + qd * fre + qe * cp * am;
  o.feg = frho * ((frho >= 0.0) ? wl_ise : wr_ise);
  o.vf = frho / ((frho >= 0.0) ? wl_idn : wr_idn);
}

// utils/fluxes/riemann/hlle.hpp:56-222 (FLUID_TYPE == gas)
inline void hlle_gas(const Real gm1, const Real wl_idn, const Real wl_ivx, const Real wl_ivy,
                     const Real wl_ivz, const Real wl_ipr, const Real wl_ise, const Real wr_idn,
                     const Real wr_ivx, const Real wr_ivy, const Real wr_ivz, const Real wr_ipr,
                     const Real wr_ise, FaceOut &o) {
  Real igm1 = 1.0 / gm1;
  Real gamma = gm1 + 1.0;
  Real sqrtdl = std::sqrt(wl_idn);
  Real sqrtdr = std::sqrt(wr_idn);
  Real isdlpdr = 1.0 / (sqrtdl + sqrtdr);
  Real wroe_ivx = (sqrtdl * wl_ivx + sqrtdr * wr_ivx) * isdlpdr;
  Real wroe_ivy = (sqrtdl * wl_ivy + sqrtdr * wr_ivy) * isdlpdr;
  Real wroe_ivz = (sqrtdl * wl_ivz + sqrtdr * wr_ivz) * isdlpdr;
  Real el = wl_ipr * igm1 + 0.5 * wl_idn * (SQR(wl_ivx) + SQR(wl_ivy) + SQR(wl_ivz));
  Real er = wr_ipr * igm1 + 0.5 * wr_idn * (SQR(wr_ivx) + SQR(wr_ivy) + SQR(wr_ivz));
  Real hroe = ((el + wl_ipr) / sqrtdl + (er + wr_ipr) / sqrtdr) * isdlpdr;
  Real qa = std::sqrt(gamma * wl_ipr / wl_idn);
  Real qb = std::sqrt(gamma * wr_ipr / wr_idn);
  Real a = hroe - 0.5 * (SQR(wroe_ivx) + SQR(wroe_ivy) + SQR(wroe_ivz));
  a = (a < 0.0) ? 0.0 : std::sqrt(gm1 * a);
  Real sla = wroe_ivx - a;
  Real slb = wl_ivx - qa;
  Real sra = wroe_ivx + a;
  Real srb = wr_ivx + qb;
  Real sl = std::min(sla, slb);
  Real sr = std::max(sra, srb);
  Real bp = (sr > 0.0) ? sr : 1.0e-20;
  Real bm = (sl < 0.0) ? sl : -1.0e-20;
  qa = wl_ivx - bm;
  qb = wr_ivx - bp;
  Real fl_d = wl_idn * qa;
  Real fr_d = wr_idn * qb;
  Real fl_mx = wl_idn * wl_ivx * qa;
  Real fr_mx = wr_idn * wr_ivx * qb;
  Real fl_my = wl_idn * wl_ivy * qa;
  Real fr_my = wr_idn * wr_ivy * qb;
  Real fl_mz = wl_idn * wl_ivz * qa;
  Real fr_mz = wr_idn * wr_ivz * qb;
  Real fl_e = el * qa + wl_ipr * wl_ivx;
  Real fr_e = er * qb + wr_ipr * wr_ivx;
  qa = 0.0;
  if (bp != bm) qa = 0.5 * (bp + bm) / (bp - bm);
  o.pf = 0.5 * (wl_ipr + wr_ipr) + qa * (wl_ipr - wr_ipr);
  const Real frho = 0.5 * (fl_d + fr_d) + qa * (fl_d - fr_d);
  o.fd = frho;
  o.fmx = 0.5 * (fl_mx + fr_mx) + qa * (fl_mx - fr_mx);
  o.fmy = 0.5 * (fl_my + fr_my) + qa * (fl_my - fr_my);
  o.fmz = 0.5 * (fl_mz + fr_mz) + qa * (fl_mz - fr_mz);
  o.fe = 0.5 * (fl_e + fr_e) + qa * (fl_e - fr_e);
  o.feg = frho * ((frho >= 0.0) ? wl_ise : wr_ise);
  o.vf = frho / ((frho >= 0.0) ? wl_idn : wr_idn);
}

// utils/fluxes/riemann/hlle.hpp:56-222 (FLUID_TYPE == dust)
inline void hlle_dust(const Real wl_idn, const Real wl_ivx, const Real wl_ivy, const Real wl_ivz,
                      const Real wr_idn, const Real wr_ivx, const Real wr_ivy, const Real wr_ivz,
                      FaceOut &o) {
  Real sqrtdl = std::sqrt(wl_idn);
  Real sqrtdr = std::sqrt(wr_idn);
  Real isdlpdr = 1.0 / (sqrtdl + sqrtdr);
  Real wroe_ivx = (sqrtdl * wl_ivx + sqrtdr * wr_ivx) * isdlpdr;
  Real sl = std::min(wroe_ivx, wl_ivx);
  Real sr = std::max(wroe_ivx, wr_ivx);
  Real bp = (sr > 0.0) ? sr : 1.0e-20;
  Real bm = (sl < 0.0) ? sl : -1.0e-20;
  Real qa = wl_ivx - bm;
  Real qb = wr_ivx - bp;
  Real fl_d = wl_idn * qa;
  Real fr_d = wr_idn * qb;
  Real fl_mx = wl_idn * wl_ivx * qa;
  Real fr_mx = wr_idn * wr_ivx * qb;
  Real fl_my = wl_idn * wl_ivy * qa;
  Real fr_my = wr_idn * wr_ivy * qb;
  Real fl_mz = wl_idn * wl_ivz * qa;
  Real fr_mz = wr_idn * wr_ivz * qb;
  qa = 0.0;
  if (bp != bm) qa = 0.5 * (bp + bm) / (bp - bm);
  o.fd = 0.5 * (fl_d + fr_d) + qa * (fl_d - fr_d);
  o.fmx = 0.5 * (fl_mx + fr_mx) + qa * (fl_mx - fr_mx);
  o.fmy = 0.5 * (fl_my + fr_my) + qa * (fl_my - fr_my);
  o.fmz = 0.5 * (fl_mz + fr_mz) + qa * (fl_mz - fr_mz);
}

// utils/fluxes/riemann/llf.hpp:47-170 (gas)
inline void llf_gas(const Real gm1, const Real wl_idn, const Real wl_ivx, const Real wl_ivy,
                    const Real wl_ivz, const Real wl_ipr, const Real wl_ise, const Real wr_idn,
                    const Real wr_ivx, const Real wr_ivy, const Real wr_ivz, const Real wr_ipr,
                    const Real wr_ise, FaceOut &o) {
  Real igm1 = 1.0 / gm1;
  Real gamma = gm1 + 1.0;
  Real qa = wl_idn * wl_ivx;
  Real qb = wr_idn * wr_ivx;
  Real fsum_d = qa + qb;
  Real fsum_mx = qa * wl_ivx + qb * wr_ivx;
  Real fsum_my = qa * wl_ivy + qb * wr_ivy;
  Real fsum_mz = qa * wl_ivz + qb * wr_ivz;
  Real el = wl_ipr * igm1 + 0.5 * wl_idn * (SQR(wl_ivx) + SQR(wl_ivy) + SQR(wl_ivz));
  Real er = wr_ipr * igm1 + 0.5 * wr_idn * (SQR(wr_ivx) + SQR(wr_ivy) + SQR(wr_ivz));
  Real fsum_e = (el + wl_ipr) * wl_ivx + (er + wr_ipr) * wr_ivx;
  qa = std::sqrt(gamma * wl_ipr / wl_idn);
  qb = std::sqrt(gamma * wr_ipr / wr_idn);
  Real a = std::max((std::abs(wl_ivx) + qa), (std::abs(wr_ivx) + qb));
  Real du_d = a * (wr_idn - wl_idn);
  Real du_mx = a * (wr_idn * wr_ivx - wl_idn * wl_ivx);
  Real du_my = a * (wr_idn * wr_ivy - wl_idn * wl_ivy);
  Real du_mz = a * (wr_idn * wr_ivz - wl_idn * wl_ivz);
  Real du_e = a * (er - el);
  o.pf = 0.5 * (wl_ipr + wr_ipr);
  const Real frho = 0.5 * (fsum_d - du_d);
  o.fd = frho;
  o.fmx = 0.5 * (fsum_mx - du_mx);
  o.fmy = 0.5 * (fsum_my - du_my);
  o.fmz = 0.5 * (fsum_mz - du_mz);
  o.fe = 0.5 * (fsum_e - du_e);
  o.feg = frho * ((frho >= 0.0) ? wl_ise : wr_ise);
  o.vf = frho / ((frho >= 0.0) ? wl_idn : wr_idn);
}

// utils/fluxes/riemann/llf.hpp:47-170 (dust)
inline void llf_dust(const Real wl_idn, const Real wl_ivx, const Real wl_ivy, const Real wl_ivz,
                     const Real wr_idn, const Real wr_ivx, const Real wr_ivy, const Real wr_ivz,
                     FaceOut &o) {
  Real qa = wl_idn * wl_ivx;
  Real qb = wr_idn * wr_ivx;
  Real fsum_d = qa + qb;
  Real fsum_mx = qa * wl_ivx + qb * wr_ivx;
  Real fsum_my = qa * wl_ivy + qb * wr_ivy;
  Real fsum_mz = qa * wl_ivz + qb * wr_ivz;
  Real a = std::max(std::abs(wl_ivx), std::abs(wr_ivx));
  Real du_d = a * (wr_idn - wl_idn);
  Real du_mx = a * (wr_idn * wr_ivx - wl_idn * wl_ivx);
  Real du_my = a * (wr_idn * wr_ivy - wl_idn * wl_ivy);
  Real du_mz = a * (wr_idn * wr_ivz - wl_idn * wl_ivz);
  o.fd = 0.5 * (fsum_d - du_d);
  o.fmx = 0.5 * (fsum_mx - du_mx);
  o.fmy = 0.5 * (fsum_my - du_my);
  o.fmz = 0.5 * (fsum_mz - du_mz);
}

// ---------------------------------------------------------------------------------------
// utils/fluxes/fluid_fluxes.hpp:78-213  CalculateFluxesImpl (Cartesian: ScaleMomentumFlux is a
// no-op, :36).  The three sweeps keep the reference's loop ranges:
//   X1: k,j interior; reconstruct cells [is-1,ie+1]; faces [is,ie+1]           (:105-126)
//   X2: k interior, i interior; cells j in [js-1,je+1]; faces [js,je+1]        (:129-168)
//   X3: j,i interior; cells k in [ks-1,ke+1]; faces [ks,ke+1]                  (:171-210)
// Face `f` of a sweep is stored at cell index f (lower face of cell f).
void solve_row(const Sim &s, int fluid, int riemann, int dir, int nsp, const Real *wl,
               const Real *wr, int rowlen, int lo, int hi, size_t base, ptrdiff_t st,
               RVec *flux, RVec *pflux, RVec *vface,
               Real gm1) {
  // wl/wr: [nvars][rowlen] scratch rows (ScratchPad2D of the reference); faces lo..hi.
  const int d = dir - 1;
  for (int n = 0; n < nsp; ++n) {
    const int IDN = n;
    const int ivx = nsp + (n * 3) + ((dir - 1));
    const int ivy = nsp + (n * 3) + ((dir - 1) + 1) % 3;
    const int ivz = nsp + (n * 3) + ((dir - 1) + 2) % 3;
    const int IPR = nsp * 4 + n;
    const int ISE = nsp * 5 + n;
    for (int f = lo; f <= hi; ++f) {
      FaceOut o;
      const size_t c = base + static_cast<size_t>(f) * st;
      if (fluid == FL_GAS) {
        const Real a0 = wl[IDN * rowlen + f], a1 = wl[ivx * rowlen + f],
                   a2 = wl[ivy * rowlen + f], a3 = wl[ivz * rowlen + f],
                   a4 = wl[IPR * rowlen + f], a5 = wl[ISE * rowlen + f];
        const Real b0 = wr[IDN * rowlen + f], b1 = wr[ivx * rowlen + f],
                   b2 = wr[ivy * rowlen + f], b3 = wr[ivz * rowlen + f],
                   b4 = wr[IPR * rowlen + f], b5 = wr[ISE * rowlen + f];
        if (riemann == RS_HLLC)
          hllc_gas(gm1, a0, a1, a2, a3, a4, a5, b0, b1, b2, b3, b4, b5, o);
        else if (riemann == RS_HLLE)
          hlle_gas(gm1, a0, a1, a2, a3, a4, a5, b0, b1, b2, b3, b4, b5, o);
        else
          llf_gas(gm1, a0, a1, a2, a3, a4, a5, b0, b1, b2, b3, b4, b5, o);
        flux[d][IDN * s.N + c] = o.fd;
        flux[d][ivx * s.N + c] = o.fmx;
        flux[d][ivy * s.N + c] = o.fmy;
        flux[d][ivz * s.N + c] = o.fmz;
        flux[d][IPR * s.N + c] = o.fe;  // IEN == IPR slot (hllc.hpp:72)
        flux[d][ISE * s.N + c] = o.feg; // IEG == ISE slot (hllc.hpp:73)
        pflux[d][n * s.N + c] = o.pf;
        vface[d][n * s.N + c] = o.vf;
      } else {
        const Real a0 = wl[IDN * rowlen + f], a1 = wl[ivx * rowlen + f],
                   a2 = wl[ivy * rowlen + f], a3 = wl[ivz * rowlen + f];
        const Real b0 = wr[IDN * rowlen + f], b1 = wr[ivx * rowlen + f],
                   b2 = wr[ivy * rowlen + f], b3 = wr[ivz * rowlen + f];
        if (riemann == RS_HLLE)
          hlle_dust(a0, a1, a2, a3, b0, b1, b2, b3, o);
        else
          llf_dust(a0, a1, a2, a3, b0, b1, b2, b3, o);
        flux[d][IDN * s.N + c] = o.fd;
        flux[d][ivx * s.N + c] = o.fmx;
        flux[d][ivy * s.N + c] = o.fmy;
        flux[d][ivz * s.N + c] = o.fmz;
      }
    }
  }
}

// utils/fluxes/fluid_fluxes.hpp:33-70 ScaleMomentumFlux: the three momentum fluxes of every
// face in [il,iu] of row (k,j) are multiplied by the scale factors at the face centroid
// (lower face of the cell that stores the flux).  No-op for Cartesian (:36).
void scale_momentum_flux(const Sim &s, int dir, int nsp, int k, int j, int il, int iu,
                         RVec *flux) {
  if (s.c.coords == CO_CART) return;
  const int d = dir - 1;
  for (int n = 0; n < nsp; ++n) {
    const int IVX = nsp + 3 * n + 0, IVY = nsp + 3 * n + 1, IVZ = nsp + 3 * n + 2;
    for (int i = il; i <= iu; ++i) {
      Coords coords(s, k, j, i);
      Real xf[3];
      if (dir == 1)
        coords.FaceCenX1(0, xf);
      else if (dir == 2)
        coords.FaceCenX2(0, xf);
      else
        coords.FaceCenX3(0, xf);
      const size_t c = IDX(s, k, j, i);
      flux[d][IVX * s.N + c] *= coords.hx1(xf[0], xf[1], xf[2]);
      flux[d][IVY * s.N + c] *= coords.hx2(xf[0], xf[1], xf[2]);
      flux[d][IVZ * s.N + c] *= coords.hx3(xf[0], xf[1], xf[2]);
    }
  }
}

void calculate_fluxes(Sim &s, int fluid, bool pcm) {
  const bool gas = (fluid == FL_GAS);
  const int nsp = gas ? s.c.ns_gas : s.c.ns_dust;
  if (nsp == 0) return;
  const int nvars = gas ? s.nvg : s.nvd;
  int recon = gas ? s.c.recon_gas : s.c.recon_dust;
  if (pcm) recon = RC_PCM; // fluid_fluxes.hpp:225
  const int riemann = gas ? s.c.riemann_gas : s.c.riemann_dust;
  const RVec &prim = gas ? s.gprim : s.dprim;
  RVec *flux = gas ? s.gflux : s.dflux;
  const Real gm1 = s.c.gamma - 1.0;
  const int ni = s.ni, nj = s.nj, nk = s.nk;
  // plm.hpp:90,124,158: PLM_G for every non-Cartesian system; PCM and PPM4 ignore GEOM
  const bool plmg = (recon == RC_PLM) && (s.c.coords != CO_CART);

  // X1 sweep
  {
#pragma omp parallel
    {
    // (row scratch hoisted out of the loops: one allocation per thread, not one per row)
    std::vector<Real> wl(static_cast<size_t>(nvars) * ni), wr(static_cast<size_t>(nvars) * ni);
#pragma omp for collapse(2) schedule(static)
    for (int k = s.ks; k <= s.ke; ++k) {
      for (int j = s.js; j <= s.je; ++j) {
        const size_t base = IDX(s, k, j, 0);
        for (int n = 0; n < nvars; ++n) {
          const Real *q = prim.data() + n * s.N + base;
          for (int i = s.is - 1; i <= s.ie + 1; ++i) {
            if (plmg) {
              const PlmGeo g = plm_geo(s, 1, k, j, i);
              recon_cell(recon, q + i, 1, wl[n * ni + i + 1], wr[n * ni + i], &g);
            } else {
              recon_cell(recon, q + i, 1, wl[n * ni + i + 1], wr[n * ni + i]);
            }
          }
        }
        solve_row(s, fluid, riemann, 1, nsp, wl.data(), wr.data(), ni, s.is, s.ie + 1, base, 1,
                  flux, s.gpflux, s.gvface, gm1);
        scale_momentum_flux(s, 1, nsp, k, j, s.is, s.ie + 1, flux);
      }
    }
    }
  }
  // X2 sweep: rows along i at fixed (k,j); wl holds ql of face j (from cell j-1).
  if (s.ndim > 1) {
#pragma omp parallel for schedule(static)
    for (int k = s.ks; k <= s.ke; ++k) {
      std::vector<Real> wl(static_cast<size_t>(nvars) * ni), wl_jp1(static_cast<size_t>(nvars) * ni),
          wr(static_cast<size_t>(nvars) * ni);
      for (int j = s.js - 1; j <= s.je + 1; ++j) {
        const size_t base = IDX(s, k, j, 0);
        for (int n = 0; n < nvars; ++n) {
          const Real *q = prim.data() + n * s.N + base;
          for (int i = s.is; i <= s.ie; ++i) {
            if (plmg) {
              const PlmGeo g = plm_geo(s, 2, k, j, i);
              recon_cell(recon, q + i, ni, wl_jp1[n * ni + i], wr[n * ni + i], &g);
            } else {
              recon_cell(recon, q + i, ni, wl_jp1[n * ni + i], wr[n * ni + i]);
            }
          }
        }
        if (j > s.js - 1) {
          solve_row(s, fluid, riemann, 2, nsp, wl.data(), wr.data(), ni, s.is, s.ie, base, 1, flux,
                    s.gpflux, s.gvface, gm1);
          scale_momentum_flux(s, 2, nsp, k, j, s.is, s.ie, flux);
        }
        wl.swap(wl_jp1);
      }
    }
  }
  // X3 sweep
  if (s.ndim > 2) {
    const ptrdiff_t sk = static_cast<ptrdiff_t>(ni) * nj;
#pragma omp parallel for schedule(static)
    for (int j = s.js; j <= s.je; ++j) {
      std::vector<Real> wl(static_cast<size_t>(nvars) * ni), wl_kp1(static_cast<size_t>(nvars) * ni),
          wr(static_cast<size_t>(nvars) * ni);
      for (int k = s.ks - 1; k <= s.ke + 1; ++k) {
        const size_t base = IDX(s, k, j, 0);
        for (int n = 0; n < nvars; ++n) {
          const Real *q = prim.data() + n * s.N + base;
          for (int i = s.is; i <= s.ie; ++i) {
            if (plmg) {
              const PlmGeo g = plm_geo(s, 3, k, j, i);
              recon_cell(recon, q + i, sk, wl_kp1[n * ni + i], wr[n * ni + i], &g);
            } else {
              recon_cell(recon, q + i, sk, wl_kp1[n * ni + i], wr[n * ni + i]);
            }
          }
        }
        if (k > s.ks - 1) {
          solve_row(s, fluid, riemann, 3, nsp, wl.data(), wr.data(), ni, s.is, s.ie, base, 1, flux,
                    s.gpflux, s.gvface, gm1);
          scale_momentum_flux(s, 3, nsp, k, j, s.is, s.ie, flux);
        }
        wl.swap(wl_kp1);
      }
    }
  }
  (void)nk;
}

// ---------------------------------------------------------------------------------------
// utils/integrators/artemis_integrator.hpp:57-110  ApplyUpdate (all Conserved+WithFluxes vars:
// gas D, M, E, eint and dust D, M).
void apply_update_fluid(Sim &s, RVec &u0, const RVec &u1,
                        const RVec *flux, int nvars, Real gam0, Real gam1,
                        Real beta_dt) {
  const bool multi_d = (s.ndim > 1), three_d = (s.ndim > 2);
  const ptrdiff_t sj = s.ni, sk = static_cast<ptrdiff_t>(s.ni) * s.nj;
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        Coords coords(s, k, j, i);
        Real ax1[2], ax2[2] = {0.0, 0.0}, ax3[2] = {0.0, 0.0};
        coords.GetFaceAreaX1(ax1);
        if (multi_d) coords.GetFaceAreaX2(ax2);
        if (three_d) coords.GetFaceAreaX3(ax3);
        const Real vol = coords.Volume();
        const size_t c = IDX(s, k, j, i);
        for (int n = 0; n < nvars; ++n) {
          const Real *f1 = flux[0].data() + n * s.N;
          Real divf = (ax1[0] * f1[c] - ax1[1] * f1[c + 1]);
          if (multi_d) {
            const Real *f2 = flux[1].data() + n * s.N;
            divf += (ax2[0] * f2[c] - ax2[1] * f2[c + sj]);
          }
          if (three_d) {
            const Real *f3 = flux[2].data() + n * s.N;
            divf += (ax3[0] * f3[c] - ax3[1] * f3[c + sk]);
          }
          Real *v0 = u0.data() + n * s.N;
          const Real *v1 = u1.data() + n * s.N;
          v0[c] = gam0 * v0[c] + gam1 * v1[c] + divf * beta_dt / vol;
        }
      }
}
void apply_update(Sim &s, Real gam0, Real gam1, Real beta_dt) {
  if (s.c.ns_gas) apply_update_fluid(s, s.gu0, s.gu1, s.gflux, s.nvg, gam0, gam1, beta_dt);
  if (s.c.ns_dust) apply_update_fluid(s, s.du0, s.du1, s.dflux, s.nvd, gam0, gam1, beta_dt);
}

// utils/integrators/artemis_integrator.hpp:30-51
void deep_copy(Sim &s) {
  auto copy = [&](RVec &dst, const RVec &src, int nvar) {
    if (dst.size() != src.size()) dst.resize(src.size());
    const size_t plane = static_cast<size_t>(s.ni) * s.nj;
    const long nk = s.nk;
#pragma omp parallel for schedule(static)
    for (long k = 0; k < nk; ++k)
      for (int n = 0; n < nvar; ++n)
        std::memcpy(dst.data() + n * s.N + k * plane, src.data() + n * s.N + k * plane, plane * sizeof(Real));
  };
  copy(s.gu1, s.gu0, s.nvg);
  copy(s.du1, s.du0, s.nvd);
}

// ---------------------------------------------------------------------------------------
// Coords<GEOM>::ConvertToCylWithVec / ConvertToCartWithVec (geometry.hpp:438-482): the converted
// point and the three rows ex1, ex2, ex3 (components of the problem's unit vectors in the target
// basis).  Cartesian geometry.hpp:286-301; cylindrical.hpp:96-107, :128-136; spherical.hpp:172-189,
// :202-220 (3D), :373-389, :403-421 (2D), :529-545, :559-577 (1D); axisymmetric.hpp:99-111, :135-145.
struct Frame {
  Real x[3], e1[3], e2[3], e3[3];
};
inline void set3(Real a[3], Real x, Real y, Real z) { a[0] = x, a[1] = y, a[2] = z; }
inline Frame to_cyl_frame(const Coords &co, const Real xi[3]) {
  Frame f;
  const Real fuzz = 1e-99;
  switch (co.sys) {
  case CO_CART: {
    Real R = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1]);
    const Real cp = xi[0] / (R + fuzz);
    const Real sp = xi[1] / (R + fuzz);
    set3(f.x, R, std::atan2(sp, cp), xi[2]);
    set3(f.e1, cp, -sp, 0.0), set3(f.e2, sp, cp, 0.0), set3(f.e3, 0.0, 0.0, 1.0);
  } break;
  case CO_CYL:
    set3(f.x, xi[0], xi[1], xi[2]);
    set3(f.e1, 1.0, 0.0, 0.0), set3(f.e2, 0.0, 1.0, 0.0), set3(f.e3, 0.0, 0.0, 1.0);
    break;
  case CO_SPH3D:
  case CO_SPH2D: {
    const Real ct = std::cos(xi[1]);
    const Real st = std::sin(xi[1]);
    set3(f.x, xi[0] * st, (co.sys == CO_SPH3D) ? xi[2] : 0.0, xi[0] * ct);
    set3(f.e1, st, 0.0, ct), set3(f.e2, ct, 0.0, -st), set3(f.e3, 0.0, 1.0, 0.0);
  } break;
  case CO_SPH1D: {
    const Real ct = 0.0, st = 1.0;
    set3(f.x, xi[0] * st, 0.0, xi[0] * ct);
    set3(f.e1, st, 0.0, ct), set3(f.e2, ct, 0.0, -st), set3(f.e3, 0.0, 1.0, 0.0);
  } break;
  default: // axisymmetric
    set3(f.x, xi[0], xi[2], xi[1]);
    set3(f.e1, 1.0, 0.0, 0.0), set3(f.e2, 0.0, 0.0, 1.0), set3(f.e3, 0.0, 1.0, 0.0);
  }
  return f;
}
inline Frame to_cart_frame(const Coords &co, const Real xi[3]) {
  Frame f;
  switch (co.sys) {
  case CO_CYL: {
    const Real cp = std::cos(xi[1]);
    const Real sp = std::sin(xi[1]);
    set3(f.x, xi[0] * cp, xi[0] * sp, xi[2]);
    set3(f.e1, cp, sp, 0.0), set3(f.e2, -sp, cp, 0.0), set3(f.e3, 0.0, 0.0, 1.0);
  } break;
  case CO_SPH3D:
  case CO_SPH2D:
  case CO_SPH1D: {
    const Real cp = (co.sys == CO_SPH3D) ? std::cos(xi[2]) : 1.0;
    const Real sp = (co.sys == CO_SPH3D) ? std::sin(xi[2]) : 0.0;
    const Real ct = (co.sys == CO_SPH1D) ? 0.0 : std::cos(xi[1]);
    const Real st = (co.sys == CO_SPH1D) ? 1.0 : std::sin(xi[1]);
    set3(f.x, xi[0] * st * cp, xi[0] * st * sp, xi[0] * ct);
    set3(f.e1, st * cp, st * sp, ct), set3(f.e2, ct * cp, ct * sp, -st), set3(f.e3, -sp, cp, 0.0);
  } break;
  case CO_AXI: {
    const Real cp = std::cos(xi[2]);
    const Real sp = std::sin(xi[2]);
    set3(f.x, xi[0] * cp, xi[0] * sp, xi[1]);
    set3(f.e1, cp, 0.0, sp), set3(f.e2, -sp, 0.0, cp), set3(f.e3, 0.0, 1.0, 0.0);
  } break;
  default:
    set3(f.x, xi[0], xi[1], xi[2]);
    set3(f.e1, 1.0, 0.0, 0.0), set3(f.e2, 0.0, 1.0, 0.0), set3(f.e3, 0.0, 0.0, 1.0);
  }
  return f;
}
// ConvertToSph(xi)[0]: the spherical radius (geometry.hpp:262-264, cylindrical.hpp:111-112,
// axisymmetric.hpp:116-117, identity for the spherical systems)
inline Real to_sph_radius(const Coords &co, const Real xi[3]) {
  switch (co.sys) {
  case CO_CART: {
    const Real R = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1]);
    return std::sqrt(R * R + xi[2] * xi[2]);
  }
  case CO_CYL: return std::sqrt(xi[0] * xi[0] + xi[2] * xi[2]);
  case CO_AXI: return std::sqrt(xi[0] * xi[0] + xi[1] * xi[1]);
  default: return xi[0];
  }
}
// RFWeights (geometry.hpp:228-232 zero default; cylindrical.hpp:82-87; axisymmetric.hpp:73-78;
// spherical.hpp:148-169 (3D), :349-370 (2D), :515-526 (1D)): +-(<R^2>_face - <R^2>) weights of
// the mass flux in the angular-momentum-conserving rotating-frame source
inline void rf_weights(const Coords &co, Real bx1[2], Real bx2[2], Real bx3[2]) {
  bx1[0] = bx1[1] = bx2[0] = bx2[1] = bx3[0] = bx3[1] = 0.0;
  const BBox &bnds = co.bnds;
  if (co.sys == CO_CYL || co.sys == CO_AXI) {
    const Real ans = 0.5 * (bnds.x1[0] + bnds.x1[1]) * (bnds.x1[1] - bnds.x1[0]);
    bx1[0] = bx1[1] = ans;
  } else if (co.sys == CO_SPH3D || co.sys == CO_SPH2D) {
    const Real rv = co.x1v();
    const Real stv = std::sin(co.x2v());
    const Real rf = 2.0 / 3.0 *
                    (bnds.x1[0] * bnds.x1[0] + bnds.x1[0] * bnds.x1[1] + bnds.x1[1] * bnds.x1[1]) /
                    (bnds.x1[0] + bnds.x1[1]);
    const Real r2cyl = SQR(rv * stv);
    bx1[0] = r2cyl - SQR(bnds.x1[0] * stv), bx1[1] = SQR(bnds.x1[1] * stv) - r2cyl;
    bx2[0] = r2cyl - SQR(rf * std::sin(bnds.x2[0])), bx2[1] = SQR(rf * std::sin(bnds.x2[1])) - r2cyl;
  } else if (co.sys == CO_SPH1D) {
    const Real rv = co.x1v();
    const Real r2cyl = SQR(rv);
    bx1[0] = r2cyl - SQR(bnds.x1[0]), bx1[1] = SQR(bnds.x1[1]) - r2cyl;
  }
}

// ---------------------------------------------------------------------------------------
// utils/fluxes/fluid_fluxes.hpp:300-420  FluxSourceImpl: pressure gradient and P div(v) work for
// gas (:361-393), then the coordinate source rho*dt*sum_d dh_d/dx_a*(v_d + vf_d)^2 on each
// momentum whose direction the metric depends on (:395-415), vf = RotationVelocity<GEOM>(xv, omf)
// (rotating_frame.hpp:31-47) with omf = rotating_frame/omega when that package is on, else 0
// (:433-437): this is where the centrifugal and Coriolis terms of the curvilinear rotating frame
// enter the radial / polar momentum equations.  Dust::FluxSource runs only for metric-dependent systems (dust.cpp:303-326)
// and has no pressure terms.  The reference loops i over [is-2, ie+1] (:325); the ghost-cell
// writes are overwritten by PrimToCons, so the oracle keeps the range to stay literal (reads
// stay in bounds because ng >= 2).
void flux_source(Sim &s, int fluid, Real dt) {
  const bool gas = (fluid == FL_GAS);
  const int nsp = gas ? s.c.ns_gas : s.c.ns_dust;
  if (!nsp) return;
  const bool multi_d = (s.ndim >= 2), three_d = (s.ndim == 3);
  {
    const Coords probe(s, s.ks, s.js, s.is);
    if (!gas && !(probe.x1dep() || (probe.x2dep() && multi_d) || (probe.x3dep() && three_d)))
      return;
  }
  const ptrdiff_t sj = s.ni, sk = static_cast<ptrdiff_t>(s.ni) * s.nj;
  RVec &u0 = gas ? s.gu0 : s.du0;
  const RVec &prim = gas ? s.gprim : s.dprim;
  const Real omf = s.rframe.on ? s.rframe.omega : 0.0;
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is - 2; i <= s.ie + 1; ++i) {
        Coords coords(s, k, j, i);
        const bool x1dep = coords.x1dep();
        const bool x2dep = coords.x2dep() && multi_d;
        const bool x3dep = coords.x3dep() && three_d;
        Real dhdx1[3] = {0.0, 0.0, 0.0}, dhdx2[3] = {0.0, 0.0, 0.0};
        if (x1dep) coords.GetConnX1(dhdx1);
        if (x2dep) coords.GetConnX2(dhdx2);
        (void)x3dep; // geometry.hpp:107-110: no system has an x3-dependent metric
        Real ax1[2], ax2[2] = {0.0, 0.0}, ax3[2] = {0.0, 0.0};
        coords.GetFaceAreaX1(ax1);
        if (multi_d) coords.GetFaceAreaX2(ax2);
        if (three_d) coords.GetFaceAreaX3(ax3);
        const Real vol = coords.Volume();
        const BBox &b = coords.bnds;
        const Real dx[3] = {b.x1[1] - b.x1[0], b.x2[1] - b.x2[0], b.x3[1] - b.x3[0]};
        const size_t c = IDX(s, k, j, i);
        Real vf[3] = {0.0, omf, 0.0}; // RotationVelocity: Cartesian returns {0, omf, 0} (all dh/dx are 0 there)
        if (coords.sys != CO_CART) {
          const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
          const Frame fr = to_cyl_frame(coords, xv);
          const Real vp = omf * fr.x[0];
          vf[0] = fr.e1[1] * vp, vf[1] = fr.e2[1] * vp, vf[2] = fr.e3[1] * vp;
        }
        for (int n = 0; n < nsp; ++n) {
          // cons pack of FluxSource is <momentum, internal_energy> (gas.cpp:505-511); in the
          // oracle's full cons layout those are slots ns+3n+d and 5ns+n.
          Real *mx = u0.data() + (nsp + 3 * n + 0) * s.N;
          Real *my = u0.data() + (nsp + 3 * n + 1) * s.N;
          Real *mz = u0.data() + (nsp + 3 * n + 2) * s.N;
          if (gas) {
            Real *eg = u0.data() + (5 * nsp + n) * s.N;
            const Real *p1 = s.gpflux[0].data() + n * s.N, *v1 = s.gvface[0].data() + n * s.N;
            mx[c] += dt / dx[0] * (p1[c] - p1[c + 1]);
            eg[c] -= dt / vol * 0.5 * (p1[c] + p1[c + 1]) * (ax1[1] * v1[c + 1] - ax1[0] * v1[c]);
            if (multi_d) {
              const Real *p2 = s.gpflux[1].data() + n * s.N, *v2 = s.gvface[1].data() + n * s.N;
              my[c] += dt / dx[1] * (p2[c] - p2[c + sj]);
              eg[c] -=
                  dt / vol * 0.5 * (p2[c] + p2[c + sj]) * (ax2[1] * v2[c + sj] - ax2[0] * v2[c]);
            }
            if (three_d) {
              const Real *p3 = s.gpflux[2].data() + n * s.N, *v3 = s.gvface[2].data() + n * s.N;
              mz[c] += dt / dx[2] * (p3[c] - p3[c + sk]);
              eg[c] -=
                  dt / vol * 0.5 * (p3[c] + p3[c + sk]) * (ax3[1] * v3[c + sk] - ax3[0] * v3[c]);
            }
          }
          const Real dens = prim[n * s.N + c];
          const Real rdt = dens * dt;
          const Real vx = prim[(nsp + 3 * n + 0) * s.N + c];
          const Real vy = prim[(nsp + 3 * n + 1) * s.N + c];
          const Real vz = prim[(nsp + 3 * n + 2) * s.N + c];
          if (x1dep)
            mx[c] += rdt * (dhdx1[0] * SQR(vx + vf[0]) + dhdx1[1] * SQR(vy + vf[1]) + dhdx1[2] * SQR(vz + vf[2]));
          if (x2dep)
            my[c] += rdt * (dhdx2[0] * SQR(vx + vf[0]) + dhdx2[1] * SQR(vy + vf[1]) + dhdx2[2] * SQR(vz + vf[2]));
        }
      }
}

// ---------------------------------------------------------------------------------------
// Coords<GEOM>::ConvertToCylWithVec (geometry.hpp:476-482): only the cylindrical radius and
// the first component of each basis vector are used by the callers restated here
// (geometry.hpp:289-306 Cartesian, cylindrical.hpp:117-126 identity, spherical.hpp:191-205 /
// :382-396 / :556-577, axisymmetric.hpp:134-145).
struct CylVec {
  Real R, e1, e2, e3; // xcyl[0], ex1[0], ex2[0], ex3[0]
};
inline CylVec to_cyl_with_vec(const Coords &co, const Real xi[3]) {
  CylVec c;
  const Real fuzz = 1e-99; // Fuzz<Real>(), artemis.hpp:113-118
  switch (co.sys) {
  case CO_CART: {
    Real R = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1]);
    const Real cp = xi[0] / (R + fuzz);
    const Real sp = xi[1] / (R + fuzz);
    c.R = R, c.e1 = cp, c.e2 = sp, c.e3 = 0.0;
  } break;
  case CO_SPH3D:
  case CO_SPH2D: {
    const Real ct = std::cos(xi[1]);
    const Real st = std::sin(xi[1]);
    c.R = xi[0] * st, c.e1 = st, c.e2 = ct, c.e3 = 0.0;
  } break;
  case CO_SPH1D: {
    const Real ct = 0.0, st = 1.0;
    c.R = xi[0] * st, c.e1 = st, c.e2 = ct, c.e3 = 0.0;
  } break;
  default: // cylindrical, axisymmetric
    c.R = xi[0], c.e1 = 1.0, c.e2 = 0.0, c.e3 = 0.0;
  }
  return c;
}

// GetSpecificInternalEnergy (artemis_utils.hpp:43-62) on the oracle's gas cons layout
inline Real specific_internal_energy(const Sim &s, int n, size_t c, const Real hx[3]) {
  const int nsp = s.c.ns_gas;
  const Real u_d = std::max(s.gu0[n * s.N + c], s.c.dfloor_gas);
  const Real rv1 = s.gu0[(nsp + 3 * n + 0) * s.N + c] / hx[0];
  const Real rv2 = s.gu0[(nsp + 3 * n + 1) * s.N + c] / hx[1];
  const Real rv3 = s.gu0[(nsp + 3 * n + 2) * s.N + c] / hx[2];
  const Real ke = 0.5 * (SQR(rv1) + SQR(rv2) + SQR(rv3)) / u_d;
  const Real e_cons = s.gu0[(4 * nsp + n) * s.N + c];
  const Real ue_cons = e_cons - ke;
  const Real sie = (ue_cons > s.c.de_switch * e_cons) ? ue_cons / u_d
                                                     : s.gu0[(5 * nsp + n) * s.N + c] / u_d;
  return std::max(sie, s.c.siefloor_gas);
}

// ---------------------------------------------------------------------------------------
// gravity/gravity.cpp:126-155 ExternalGravity -> gravity/uniform.cpp:28-84 UniformGravity,
// gravity/point_mass.cpp:27-198 PointMassGravity.  Point mass: Cartesian (offset mass,
// softening, sink), spherical1D/2D and axisymmetric (mass at the origin); cylindrical and
// spherical3D go through ConvertToCartWithVec like the Cartesian system.
// gravity.hpp:66-94 Orbit::solve: the separation vector of the binary at time t in a frame
// rotating with omf (the true anomaly advances uniformly: exact for e = 0)
template <class G>
inline void orbit_solve(const G &o, Real t, Real omf, Real pos[3]) {
  const Real sint = std::sin(t * (o.n - omf));
  const Real cost = std::cos(t * (o.n - omf));
  Real cosf = o.cosf0 * cost - o.sinf0 * sint;
  Real sinf = o.cosf0 * sint + o.sinf0 * cost;
  const Real rb = o.a * (1.0 - SQR(o.e)) / (1.0 + o.e * cosf);
  const Real xb = rb * cosf;
  const Real yb = rb * sinf;
  cosf = xb * o.coso - o.sino * yb;
  sinf = xb * o.sino + o.coso * yb;
  pos[0] = (o.cosO * cosf - o.sinO * sinf * o.cosI);
  pos[1] = (o.sinO * cosf + o.cosO * sinf * o.cosI);
  pos[2] = sinf * o.sinI;
}

// ---------------------------------------------------------------------------------------
// gravity/nbody_gravity.hpp:28-221 NBodyGravity<GEOM> with nbody/particle_base.hpp:96-258 (RelativePosition,
// idr3, grav_accel, accrete, CartToSph).  One sweep per particle like the reference's loop of par_reduce's;
// the per-particle back-reaction {mass accreted, gravity force x3, accretion force x3} is summed serially in
// loop order (Kokkos leaves the order unspecified: compare those seven numbers to round-off, the fluid bitwise).
inline Real nb_idr3(const Sim::NBodyParticle &p, const Real dr2) { // particle_base.hpp:146-166
  const Real fuzz = 1e-99;
  const Real rs2 = SQR(p.rs);
  const Real idr3_p = 1.0 / (fuzz + std::sqrt(dr2 + rs2) * (dr2 + rs2));
  const Real dr3 = dr2 * std::sqrt(dr2);
  const Real u2 = dr2 / (rs2 + fuzz);
  const Real u = std::sqrt(u2);
  const Real u3 = u * u2;
  const Real h3inv = 1. / (rs2 * p.rs + fuzz);
  const Real idr3_s = (dr2 >= rs2) ? 1.0 / dr3
                                   : ((u < 0.5) ? h3inv * (32.0 / 3.0 - 192.0 / 5.0 * u2 + 32.0 * u3)
                                                : h3inv * (64.0 / 3.0 - 48.0 * u + 192.0 / 5.0 * u2 - 32.0 / 3.0 * u3 -
                                                           1.0 / (15.0 * u3)));
  return idr3_p * (1 - p.spline) + p.spline * idr3_s;
}
inline void nb_accrete(const Sim::NBodyParticle &p, const Real x[3], const Real den, const Real v[3], const Real vb[3],
                       const Real dt, Real *dm, Real *dmom, Real *dEk, Real * /*dEi*/) { // particle_base.hpp:190-245
  const Real fuzz = 1e-99;
  const Real vrel[3] = {v[0] + vb[0], v[1] + vb[1], v[2] + vb[2]};
  Real dx[3], dv[3];
  for (int d = 0; d < 3; d++) dx[d] = x[d] - (p.pos[d] - p.xf[d]), dv[d] = vrel[d] - (p.vel[d] - p.vf[d]);
  const Real dv2 = SQR(dv[0]) + SQR(dv[1]) + SQR(dv[2]);
  // CartToSph (:247-262): [dr, er, et, ep] = {xout, ex1, ex2, ex3} (:201), i.e. et = ex2 = {st sp, ct sp, cp} and
  // ep = ex3 = {ct, -st, 0} exactly as written at :256-257 (rows of the matrix, not the textbook unit vectors)
  const Real R = std::sqrt(SQR(dx[0]) + SQR(dx[1]));
  const Real r = std::sqrt(SQR(R) + SQR(dx[2]));
  const Real ct = dx[2] / (r + fuzz), st = R / (r + fuzz);
  const Real cp = dx[0] / (R + fuzz), sp = dx[1] / (R + fuzz);
  const Real et[3] = {st * sp, ct * sp, cp}, ep[3] = {ct, -st, 0.0};
  const Real dvt = dv[0] * et[0] + dv[1] * et[1] + dv[2] * et[2];
  const Real dvp = dv[0] * ep[0] + dv[1] * ep[1] + dv[2] * ep[2];
  const bool acc = ((p.racc > 0.0) && (r <= p.racc) && (-p.GM / (r + fuzz) + 0.5 * dv2 <= 0.0));
  const Real ramp = SQR((p.racc - r) / (p.racc + fuzz));
  const Real gdt = acc * std::min(ramp * p.gamma * dt, 1.0 / 9.0);
  const Real bdt = acc * std::min(ramp * p.beta * dt, 1.0 / 9.0);
  const Real fm = -gdt / (1.0 + gdt);
  *dm += den * fm;
  const Real fp = (gdt - bdt) / ((1.0 + gdt) * (1.0 + bdt));
  const Real denp = den * (1.0 + fm);
  for (int i = 0; i < 3; i++) {
    const Real dmv = den * (fm * v[i] + fp * (dvt * et[i] + dvp * ep[i]));
    dmom[i] += dmv;
    const Real vxp = (den * v[i] + dmv) / denp;
    *dEk += 0.5 * (v[i] + vxp) * den * (vxp - v[i]) + 0.5 * den * fm * vxp * vxp;
  }
}
void nbody_gravity(Sim &s, Real /*time*/, Real dt) {
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const int npart = static_cast<int>(s.nbody.size());
  s.pforce.resize(static_cast<size_t>(7) * npart, 0.0);
  Real omf = 0.0;
  if (s.rframe.on && s.nbody_frame_correction) omf = s.rframe.omega; // nbody_gravity.hpp:179-186
  for (int np = 0; np < npart; ++np) {
    const Sim::NBodyParticle &pl = s.nbody[np];
    Real lforce[7] = {0, 0, 0, 0, 0, 0, 0};
    if (!pl.couple) continue;
    for (int k = s.ks; k <= s.ke; ++k)
      for (int j = s.js; j <= s.je; ++j)
        for (int i = s.is; i <= s.ie; ++i) {
          const Coords coords(s, k, j, i);
          const Real x[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
          const Frame fr = to_cart_frame(coords, x);
          const Real *xcart = fr.x, *ex1 = fr.e1, *ex2 = fr.e2, *ex3 = fr.e3;
          Real hx[3];
          coords.GetScaleFactors(hx);
          const Real vol = coords.Volume();
          Real g[3] = {0.0, 0.0, 0.0};
          { // grav_accel (:178-187)
            Real dxp[3];
            for (int d = 0; d < 3; d++) dxp[d] = xcart[d] - (pl.pos[d] - pl.xf[d]);
            const Real dr2 = SQR(dxp[0]) + SQR(dxp[1]) + SQR(dxp[2]);
            const Real idr3_ = nb_idr3(pl, dr2);
            for (int d = 0; d < 3; d++) g[d] += -pl.GM * idr3_ * dxp[d];
          }
          const Real gx1 = g[0] * ex1[0] + g[1] * ex1[1] + g[2] * ex1[2];
          const Real gx2 = g[0] * ex2[0] + g[1] * ex2[1] + g[2] * ex2[2];
          const Real gx3 = g[0] * ex3[0] + g[1] * ex3[1] + g[2] * ex3[2];
          Real vf[3] = {0.0, 0.0, 0.0};
          if (omf != 0.0) {
            Real vrot[3] = {0.0, omf, 0.0};
            if (coords.sys != CO_CART) {
              const Frame fc = to_cyl_frame(coords, x);
              const Real vp = omf * fc.x[0];
              vrot[0] = fc.e1[1] * vp, vrot[1] = fc.e2[1] * vp, vrot[2] = fc.e3[1] * vp;
            }
            vf[0] = ex1[0] * vrot[0] + ex2[0] * vrot[1] + ex3[0] * vrot[2];
            vf[1] = ex1[1] * vrot[0] + ex2[1] * vrot[1] + ex3[1] * vrot[2];
            vf[2] = ex1[2] * vrot[0] + ex2[2] * vrot[1] + ex3[2] * vrot[2];
          }
          const size_t c = IDX(s, k, j, i);
          auto fluid = [&](RVec &prim, RVec &u0, int nsp, int n, bool gas) {
            const Real dens = prim[n * s.N + c];
            const Real v[3] = {prim[(nsp + 3 * n + 0) * s.N + c], prim[(nsp + 3 * n + 1) * s.N + c],
                               prim[(nsp + 3 * n + 2) * s.N + c]};
            Real vcart[3];
            vcart[0] = ex1[0] * v[0] + ex2[0] * v[1] + ex3[0] * v[2];
            vcart[1] = ex1[1] * v[0] + ex2[1] * v[1] + ex3[1] * v[2];
            vcart[2] = ex1[2] * v[0] + ex2[2] * v[1] + ex3[2] * v[2];
            Real dm = 0.0, dmom[3] = {0.0, 0.0, 0.0}, dek = 0.0, dei = 0.0;
            nb_accrete(pl, xcart, dens, vcart, vf, dt, &dm, dmom, &dek, &dei);
            const Real dmx1 = dmom[0] * ex1[0] + dmom[1] * ex1[1] + dmom[2] * ex1[2];
            const Real dmx2 = dmom[0] * ex2[0] + dmom[1] * ex2[1] + dmom[2] * ex2[2];
            const Real dmx3 = dmom[0] * ex3[0] + dmom[1] * ex3[1] + dmom[2] * ex3[2];
            const Real rdt = dens * dt;
            u0[n * s.N + c] += dm;
            u0[(nsp + 3 * n + 0) * s.N + c] += hx[0] * (rdt * gx1 + dmx1);
            u0[(nsp + 3 * n + 1) * s.N + c] += hx[1] * (rdt * gx2 + dmx2);
            u0[(nsp + 3 * n + 2) * s.N + c] += hx[2] * (rdt * gx3 + dmx3);
            if (gas) {
              u0[(4 * nsp + n) * s.N + c] += dek + dei + rdt * (v[0] * gx1 + v[1] * gx2 + v[2] * gx3);
              u0[(5 * nsp + n) * s.N + c] += dei;
            }
            lforce[0] -= vol * dm / dt;
            lforce[1] -= g[0] * dens * vol;
            lforce[2] -= g[1] * dens * vol;
            lforce[3] -= g[2] * dens * vol;
            lforce[4] -= dmom[0] / dt;
            lforce[5] -= dmom[1] / dt;
            lforce[6] -= dmom[2] / dt;
          };
          for (int n = 0; n < ng_; ++n) fluid(s.gprim, s.gu0, ng_, n, true);
          for (int n = 0; n < nd_; ++n) fluid(s.dprim, s.du0, nd_, n, false);
        }
    for (int q = 0; q < 7; ++q) s.pforce[7 * np + q] += lforce[q];
  }
}

void external_gravity(Sim &s, Real time, Real dt) {
  if (s.grav.type == 0) return;
  if (!((time >= s.grav.tstart) && (time < s.grav.tstop))) return; // gravity.cpp:134
  if (s.grav.type == 4) { // gravity.cpp:150-155
    nbody_gravity(s, time, dt);
    return;
  }
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const bool multi_d = (s.ndim >= 2), three_d = (s.ndim == 3);
  const Real gm = s.grav.gm;
  const Real sink_rate = dt * s.grav.sink_rate;
  const Real sink_rad = s.grav.sink;
  const Real rsft2 = SQR(s.grav.soft);
  // binary_mass.cpp:41-70: positions of the two bodies about the centre of mass `pos`
  Real pos1[3] = {0, 0, 0}, pos2[3] = {0, 0, 0};
  const Real mu1 = 1. / (1.0 + s.grav.q), mu2 = s.grav.q / (1.0 + s.grav.q);
  if (s.grav.type == 3 && s.grav.given_pos) {
    for (int n = 0; n < 3; n++) pos1[n] = s.grav.pos[n], pos2[n] = s.grav.pos2[n];
  } else if (s.grav.type == 3) {
    const Real omf = s.rframe.on ? s.rframe.omega : 0.0;
    Real rb[3];
    orbit_solve(s.grav, time, omf, rb);
    for (int n = 0; n < 3; n++) {
      pos1[n] = s.grav.pos[n] - mu2 * rb[n];
      pos2[n] = s.grav.pos[n] + mu1 * rb[n];
    }
  }
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const Coords coords(s, k, j, i);
        const Real dx[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
        Real hx[3];
        coords.GetScaleFactors(hx);
        Real gx1 = 0.0, gx2 = 0.0, gx3 = 0.0, fd = 0.0;
        if (s.grav.type == 1) {
          gx1 = s.grav.g[0], gx2 = s.grav.g[1], gx3 = s.grav.g[2];
        } else if (s.grav.type == 3) { // binary_mass.cpp:86-160
          const Frame fr = to_cart_frame(coords, dx);
          Real dxc1[3] = {fr.x[0], fr.x[1], fr.x[2]}, dxc2[3];
          for (int n = 0; n < 3; n++) {
            dxc2[n] = dxc1[n] - pos2[n];
            dxc1[n] -= pos1[n];
          }
          auto sph_r = [](const Real x[3]) {
            const Real R = std::sqrt(x[0] * x[0] + x[1] * x[1]);
            return std::sqrt(R * R + x[2] * x[2]);
          };
          const Real r1 = sph_r(dxc1), r2 = sph_r(dxc2);
          const Real rad2_1 = SQR(r1) + SQR(s.grav.soft);
          const Real rad2_2 = SQR(r2) + SQR(s.grav.soft2);
          const Real idr3_1 = 1.0 / (std::sqrt(rad2_1) * rad2_1);
          const Real idr3_2 = 1.0 / (std::sqrt(rad2_2) * rad2_2);
          Real g[3] = {-gm * (mu1 * dxc1[0] * idr3_1 + mu2 * dxc2[0] * idr3_2),
                       multi_d * (-gm * (mu1 * dxc1[1] * idr3_1 + mu2 * dxc2[1] * idr3_2)),
                       three_d * (-gm * (mu1 * dxc1[2] * idr3_1 + mu2 * dxc2[2] * idr3_2))};
          gx1 = g[0] * fr.e1[0] + g[1] * fr.e1[1] + g[2] * fr.e1[2];
          gx2 = g[0] * fr.e2[0] + g[1] * fr.e2[1] + g[2] * fr.e2[2];
          gx3 = g[0] * fr.e3[0] + g[1] * fr.e3[1] + g[2] * fr.e3[2];
          const Real sink_rate2 = dt * s.grav.sink_rate2;
          const Real sramp1 = sink_rate * SQR((r1 - sink_rad) / sink_rad);
          const Real sramp2 = sink_rate2 * SQR((r2 - s.grav.sink2) / s.grav.sink2);
          Real fd1 = std::min(0.25, sramp1 / (1.0 + sramp1));
          Real fd2 = std::min(0.25, sramp2 / (1.0 + sramp2));
          fd1 *= ((sink_rate > 0.0) && (sink_rad > 0.0) && (r1 <= sink_rad));
          fd2 *= ((sink_rate2 > 0.0) && (s.grav.sink2 > 0.0) && (r2 <= s.grav.sink2));
          fd = fd1 + fd2;
        } else {
          Real dr;
          if (coords.sys == CO_SPH1D || coords.sys == CO_SPH2D) { // point_mass.cpp:78-81
            const Real rad2 = SQR(dx[0]) + rsft2;
            gx1 = -gm / rad2;
            dr = std::sqrt(rad2);
          } else if (coords.sys == CO_AXI) { // :82-89 with axisymmetric.hpp ConvertToSphWithVec
            const Real rsph = std::sqrt(dx[0] * dx[0] + dx[1] * dx[1]);
            const Real ct = dx[1] / (rsph + 1e-99);
            const Real st = dx[0] / (rsph + 1e-99);
            dr = rsph;
            const Real rad2 = SQR(dr) + rsft2;
            const Real g = -gm / rad2;
            gx1 = g * st; // ex1[0]
            gx2 = g * ct; // ex3[0]
          } else { // Cartesian, cylindrical, spherical3D: through the Cartesian frame (:91-112)
            const Frame fr = to_cart_frame(coords, dx);
            Real dxc[3] = {fr.x[0], fr.x[1], fr.x[2]};
            for (int n = 0; n < 3; n++)
              dxc[n] -= s.grav.pos[n];
            const Real R = std::sqrt(dxc[0] * dxc[0] + dxc[1] * dxc[1]); // geometry.hpp:262-264
            const Real r = std::sqrt(R * R + dxc[2] * dxc[2]);
            dr = r;
            const Real rad2 = SQR(dr) + rsft2;
            const Real idr3 = 1.0 / (std::sqrt(rad2) * rad2);
            Real g[3] = {-gm * dxc[0] * idr3, (multi_d) * (-gm * dxc[1] * idr3),
                         (three_d) * (-gm * dxc[2] * idr3)};
            gx1 = g[0] * fr.e1[0] + g[1] * fr.e1[1] + g[2] * fr.e1[2];
            gx2 = g[0] * fr.e2[0] + g[1] * fr.e2[1] + g[2] * fr.e2[2];
            gx3 = g[0] * fr.e3[0] + g[1] * fr.e3[1] + g[2] * fr.e3[2];
          }
          const Real sramp = sink_rate * SQR((dr - sink_rad) / sink_rad); // quad_ramp, gravity.hpp:116
          fd = std::min(0.5, sramp / (1.0 + sramp));
          fd *= ((sink_rate > 0.0) && (dr <= sink_rad));
        }
        const size_t c = IDX(s, k, j, i);
        for (int n = 0; n < ng_; ++n) {
          const Real rho = s.gprim[n * s.N + c];
          const Real v1 = s.gprim[(ng_ + 3 * n + 0) * s.N + c];
          const Real v2 = s.gprim[(ng_ + 3 * n + 1) * s.N + c];
          const Real v3 = s.gprim[(ng_ + 3 * n + 2) * s.N + c];
          Real &m1 = s.gu0[(ng_ + 3 * n + 0) * s.N + c], &m2 = s.gu0[(ng_ + 3 * n + 1) * s.N + c];
          Real &m3 = s.gu0[(ng_ + 3 * n + 2) * s.N + c], &en = s.gu0[(4 * ng_ + n) * s.N + c];
          if (s.grav.type == 1) { // uniform.cpp:58-68
            const Real rdt = dt * rho;
            m1 += rdt * hx[0] * gx1;
            m2 += rdt * hx[1] * gx2;
            m3 += rdt * hx[2] * gx3;
            en += rdt * (v1 * gx1 + v2 * gx2 + v3 * gx3);
          } else { // point_mass.cpp:137-156
            const Real sie = s.gprim[(5 * ng_ + n) * s.N + c];
            const Real tote = rho * (sie + 0.5 * (SQR(v1) + SQR(v2) + SQR(v3)));
            m1 += dt * rho * hx[0] * gx1;
            m2 += dt * rho * hx[1] * gx2;
            m3 += dt * rho * hx[2] * gx3;
            en += dt * rho * (v1 * gx1 + v2 * gx2 + v3 * gx3);
            s.gu0[n * s.N + c] -= fd * rho;
            m1 -= fd * hx[0] * rho * v1;
            m2 -= fd * hx[1] * rho * v2;
            m3 -= fd * hx[2] * rho * v3;
            en -= fd * tote;
          }
        }
        for (int n = 0; n < nd_; ++n) {
          const Real rho = s.dprim[n * s.N + c];
          const Real v1 = s.dprim[(nd_ + 3 * n + 0) * s.N + c];
          const Real v2 = s.dprim[(nd_ + 3 * n + 1) * s.N + c];
          const Real v3 = s.dprim[(nd_ + 3 * n + 2) * s.N + c];
          Real &m1 = s.du0[(nd_ + 3 * n + 0) * s.N + c], &m2 = s.du0[(nd_ + 3 * n + 1) * s.N + c];
          Real &m3 = s.du0[(nd_ + 3 * n + 2) * s.N + c];
          if (s.grav.type == 1) { // uniform.cpp:71-78
            const Real rdt = dt * rho;
            m1 += rdt * hx[0] * gx1;
            m2 += rdt * hx[1] * gx2;
            m3 += rdt * hx[2] * gx3;
          } else { // point_mass.cpp:160-176
            m1 += dt * rho * hx[0] * gx1;
            m2 += dt * rho * hx[1] * gx2;
            m3 += dt * rho * hx[2] * gx3;
            s.du0[n * s.N + c] -= fd * rho;
            m1 -= fd * hx[0] * rho * v1;
            m2 -= fd * hx[1] * rho * v2;
            m3 -= fd * hx[2] * rho * v3;
          }
        }
      }
}

// ---------------------------------------------------------------------------------------
// rotating_frame/rotating_frame.cpp:56-86 RotatingFrameForce -> Cartesian:
// rotating_frame_impl.hpp:28-93 ShearingBoxImpl (tidal potential differenced across the cell
// + Coriolis force).  The curvilinear flux-form variant (:95-199) is not restated.
// rotating_frame_impl.hpp:95-199 RotatingFrameImpl<GEOM>: every non-Cartesian system
// (rotating_frame.cpp:63-79).  Reads the MASS fluxes of the stage.
void rotating_frame_curvilinear(Sim &s, Real dt) {
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const int multi_d = (s.ndim >= 2), three_d = (s.ndim == 3);
  const Real om0 = s.rframe.omega;
  const Real omdt = om0 * dt;
  const Real om2dt = omdt * om0;
  const ptrdiff_t sj = s.ni, sk = static_cast<ptrdiff_t>(s.ni) * s.nj;
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const Coords coords(s, k, j, i);
        const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
        const Frame fr = to_cyl_frame(coords, xv);
        Real bx1[2], bx2[2], bx3[2];
        rf_weights(coords, bx1, bx2, bx3);
        Real ax1[2], ax2[2] = {0.0, 0.0}, ax3[2] = {0.0, 0.0};
        coords.GetFaceAreaX1(ax1);
        if (multi_d) coords.GetFaceAreaX2(ax2);
        if (three_d) coords.GetFaceAreaX3(ax3);
        const Real vol = coords.Volume();
        const size_t c = IDX(s, k, j, i);
        const size_t c2 = c + multi_d * sj, c3 = c + three_d * sk;
        auto body = [&](const RVec *flux, RVec &u0, int nsp, int n, bool gas) {
          const Real *f1 = flux[0].data() + n * s.N, *f2 = flux[1].data() + n * s.N;
          const Real *f3 = flux[2].data() + n * s.N;
          const Real divf = (f1[c] * ax1[0] * bx1[0] + f1[c + 1] * ax1[1] * bx1[1]) +
                            multi_d * (f2[c] * ax2[0] * bx2[0] + f2[c2] * ax2[1] * bx2[1]) +
                            three_d * (f3[c] * ax3[0] * bx3[0] + f3[c3] * ax3[1] * bx3[1]);
          u0[(nsp + 3 * n + 0) * s.N + c] -= omdt * (divf / vol) * fr.e1[1];
          u0[(nsp + 3 * n + 1) * s.N + c] -= omdt * (divf / vol) * fr.e2[1];
          u0[(nsp + 3 * n + 2) * s.N + c] -= omdt * (divf / vol) * fr.e3[1];
          if (!gas) return;
          const Real fx[3] = {0.5 * (f1[c] + f1[c + 1]), multi_d * 0.5 * (f2[c] + f2[c2]),
                              three_d * 0.5 * (f3[c] + f3[c3])};
          u0[(4 * nsp + n) * s.N + c] +=
              om2dt * fr.x[0] * (fx[0] * fr.e1[0] + fx[1] * fr.e2[0] + fx[2] * fr.e3[0]);
        };
        for (int n = 0; n < ng_; ++n) body(s.gflux, s.gu0, ng_, n, true);
        for (int n = 0; n < nd_; ++n) body(s.dflux, s.du0, nd_, n, false);
      }
}

void rotating_frame_force(Sim &s, Real dt) {
  if (!s.rframe.on) return;
  if (s.c.coords != CO_CART) return rotating_frame_curvilinear(s, dt);
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const int three_d = (s.ndim == 3);
  const Real om0 = s.rframe.omega, qshear = s.rframe.qshear;
  const Real omsq = SQR(om0);
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const BBox b = bbox(s, k, j, i);
        const Real dx = b.x1[1] - b.x1[0];
        const Real dz = b.x3[1] - b.x3[0];
        const Real phi_xm1 = -qshear * omsq * b.x1[0] * b.x1[0];
        const Real phi_xp1 = -qshear * omsq * b.x1[1] * b.x1[1];
        const Real phi_zm1 = 0.5 * omsq * b.x3[0] * b.x3[0];
        const Real phi_zp1 = 0.5 * omsq * b.x3[1] * b.x3[1];
        const Real dpx = (phi_xp1 - phi_xm1) / dx;
        const Real dpz = three_d * ((phi_zp1 - phi_zm1) / dz);
        const size_t c = IDX(s, k, j, i);
        for (int n = 0; n < ng_; ++n) {
          const Real dens = s.gprim[n * s.N + c];
          const Real v1 = s.gprim[(ng_ + 3 * n + 0) * s.N + c];
          const Real v2 = s.gprim[(ng_ + 3 * n + 1) * s.N + c];
          const Real v3 = s.gprim[(ng_ + 3 * n + 2) * s.N + c];
          const Real rdt = dens * dt;
          s.gu0[(ng_ + 3 * n + 0) * s.N + c] -= rdt * (dpx - 2.0 * om0 * v2);
          s.gu0[(ng_ + 3 * n + 1) * s.N + c] -= rdt * 2.0 * om0 * v1;
          s.gu0[(ng_ + 3 * n + 2) * s.N + c] -= rdt * dpz;
          s.gu0[(4 * ng_ + n) * s.N + c] -= rdt * (v1 * dpx + v3 * dpz);
        }
        for (int n = 0; n < nd_; ++n) {
          const Real dens = s.dprim[n * s.N + c];
          const Real v1 = s.dprim[(nd_ + 3 * n + 0) * s.N + c];
          const Real v2 = s.dprim[(nd_ + 3 * n + 1) * s.N + c];
          const Real rdt = dens * dt;
          s.du0[(nd_ + 3 * n + 0) * s.N + c] -= rdt * (dpx - 2.0 * om0 * v2);
          s.du0[(nd_ + 3 * n + 1) * s.N + c] -= rdt * 2.0 * om0 * v1;
          s.du0[(nd_ + 3 * n + 2) * s.N + c] -= rdt * dpz;
        }
      }
}

// ---------------------------------------------------------------------------------------
// drag/drag.cpp:89-175 DragSource with damp_to_visc = false (DiffType::null: the viscous
// target velocity has mu = 0, utils/diffusion/diffusion_coeff.hpp:170-190):
//   type 2 -> drag.hpp:171-294 SelfDragSourceImpl (quadratic damping ramps near the mesh edges)
//   type 1 -> drag.hpp:296-482 SimpleDragSourceImpl (implicit gas-dust coupling, one gas species)
inline void damping_ramps(const Sim &s, const Sim::SelfDrag &p, const Real xv[3], Real dt,
                          Real f[3]) {
  const int multi_d = (s.ndim >= 2), three_d = (s.ndim == 3);
  const Real x1min = s.gx1min, x1max = s.gx1max, x2min = s.gx2min, x2max = s.gx2max;
  const Real x3min = s.gx3min, x3max = s.gx3max;
  f[0] = dt * (p.irate[0] * ((xv[0] < p.ix[0]) * SQR((xv[0] - p.ix[0]) / (p.ix[0] - x1min))) +
               p.orate[0] * ((xv[0] > p.ox[0]) * SQR((xv[0] - p.ox[0]) / (p.ox[0] - x1max))));
  f[1] = multi_d * dt *
         (p.irate[1] * ((xv[1] < p.ix[1]) * SQR((xv[1] - p.ix[1]) / (p.ix[1] - x2min))) +
          p.orate[1] * ((xv[1] > p.ox[1]) * SQR((xv[1] - p.ox[1]) / (p.ox[1] - x2max))));
  f[2] = three_d * dt *
         (p.irate[2] * ((xv[2] < p.ix[2]) * SQR((xv[2] - p.ix[2]) / (p.ix[2] - x3min))) +
          p.orate[2] * ((xv[2] > p.ox[2]) * SQR((xv[2] - p.ox[2]) / (p.ox[2] - x3max))));
}
inline Real diff_coeff_at(const Sim &s, const Sim::DiffCoeff &dp, Real dens, Real sie, int k, int j, int i);
void drag_source(Sim &s, Real dt) {
  if (s.drag.type == 0) return;
  const bool dvisc = s.drag.damp_to_visc; // DiffType::null otherwise: mu = 0 (diffusion_coeff.hpp:185-189)
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const Real gm1 = s.c.gamma - 1.0;
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const Coords coords(s, k, j, i);
        const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
        Real hx[3];
        coords.GetScaleFactors(hx);
        const CylVec cv = to_cyl_with_vec(coords, xv);
        const size_t c = IDX(s, k, j, i);
        Real bg[3], bd[3];
        damping_ramps(s, s.drag.gas, xv, dt, bg);
        damping_ramps(s, s.drag.dust, xv, dt, bd);
        if (s.drag.type == 2) { // SelfDragSourceImpl
          for (int n = 0; n < ng_; ++n) {
            const Real dens = s.gu0[n * s.N + c];
            Real *m[3] = {&s.gu0[(ng_ + 3 * n + 0) * s.N + c], &s.gu0[(ng_ + 3 * n + 1) * s.N + c],
                          &s.gu0[(ng_ + 3 * n + 2) * s.N + c]};
            const Real vg[3] = {*m[0] / (hx[0] * dens), *m[1] / (hx[1] * dens), *m[2] / (hx[2] * dens)};
            const Real sien = specific_internal_energy(s, n, c, hx); // drag.hpp:234-235
            const Real mu = dvisc ? diff_coeff_at(s, s.visc, dens, sien, k, j, i) : 0.0;
            const Real vR = -1.5 * mu / (cv.R * dens);
            const Real vd[3] = {cv.e1 * vR, cv.e2 * vR, cv.e3 * vR};
            const Real dm1 = -bg[0] * dens * (vg[0] - vd[0]) / (1.0 + bg[0]);
            const Real dm2 = -bg[1] * dens * (vg[1] - vd[1]) / (1.0 + bg[1]);
            const Real dm3 = -bg[2] * dens * (vg[2] - vd[2]) / (1.0 + bg[2]);
            *m[0] += hx[0] * dm1;
            *m[1] += hx[1] * dm2;
            *m[2] += hx[2] * dm3;
            s.gu0[(4 * ng_ + n) * s.N + c] += dm1 * (vg[0] + 0.5 * dm1 / dens) +
                                              dm2 * (vg[1] + 0.5 * dm2 / dens) +
                                              dm3 * (vg[2] + 0.5 * dm3 / dens);
          }
          for (int n = 0; n < nd_; ++n) {
            Real *m[3] = {&s.du0[(nd_ + 3 * n + 0) * s.N + c], &s.du0[(nd_ + 3 * n + 1) * s.N + c],
                          &s.du0[(nd_ + 3 * n + 2) * s.N + c]};
            const Real mom[3] = {*m[0], *m[1], *m[2]};
            *m[0] -= bd[0] * mom[0] / (1.0 + bd[0]);
            *m[1] -= bd[1] * mom[1] / (1.0 + bd[1]);
            *m[2] -= bd[2] * mom[2] / (1.0 + bd[2]);
          }
          continue;
        }
        // SimpleDragSourceImpl
        const Real dg = s.gu0[0 * s.N + c];
        Real *mg[3] = {&s.gu0[(ng_ + 0) * s.N + c], &s.gu0[(ng_ + 1) * s.N + c],
                       &s.gu0[(ng_ + 2) * s.N + c]};
        const Real vg[3] = {*mg[0] / (hx[0] * dg), *mg[1] / (hx[1] * dg), *mg[2] / (hx[2] * dg)};
        const Real sieg = specific_internal_energy(s, 0, c, hx);
        const Real mu = dvisc ? diff_coeff_at(s, s.visc, dg, sieg, k, j, i) : 0.0; // drag.hpp:392-393
        const Real vR = -1.5 * mu / (cv.R * dg);
        const Real vt[3] = {cv.e1 * vR, cv.e2 * vR, cv.e3 * vR};
        Real fd[3] = {0., 0., 0.};
        Real fvd[3] = {0., 0., 0.};
        Real vth = 0.0;
        if (s.drag.model == 1) vth = std::sqrt(8.0 / M_PI * gm1 * sieg); // Gruneisen = gm1
        const Real vdt[3] = {0.0, 0.0, 0.0};
        for (int n = 0; n < nd_; ++n) {
          const Real dens = s.du0[n * s.N + c];
          const Real vd[3] = {s.du0[(nd_ + 3 * n + 0) * s.N + c] / (hx[0] * dens),
                              s.du0[(nd_ + 3 * n + 1) * s.N + c] / (hx[1] * dens),
                              s.du0[(nd_ + 3 * n + 2) * s.N + c] / (hx[2] * dens)};
          Real tc = s.drag.tau[n];
          if (s.drag.model == 1) tc = s.drag.scale * s.drag.grain_density / dg * s.drag.sizes[n] / vth;
          const Real alpha = dt * ((tc <= 0.0) ? std::numeric_limits<Real>::max() : 1.0 / tc);
          for (int d = 0; d < 3; d++) {
            const Real rhop = dens * alpha / (1.0 + alpha + bd[d]);
            fd[d] += rhop * (1.0 + bd[d]);
            fvd[d] += rhop * (vd[d] + bd[d] * vdt[d]);
          }
        }
        Real vgp[3];
        for (int d = 0; d < 3; d++)
          vgp[d] = (dg * (vg[d] + bg[d] * vt[d]) + fvd[d]) / (dg * (1.0 + bg[d]) + fd[d]);
        Real delta_g[3] = {0.0, 0.0, 0.0};
        for (int d = 0; d < 3; d++)
          fvd[d] = 0.;
        for (int n = 0; n < nd_; ++n) {
          const Real dens = s.du0[n * s.N + c];
          const Real vd[3] = {s.du0[(nd_ + 3 * n + 0) * s.N + c] / (hx[0] * dens),
                              s.du0[(nd_ + 3 * n + 1) * s.N + c] / (hx[1] * dens),
                              s.du0[(nd_ + 3 * n + 2) * s.N + c] / (hx[2] * dens)};
          Real tc = s.drag.tau[n];
          if (s.drag.model == 1) tc = s.drag.scale * s.drag.grain_density / dg * s.drag.sizes[n] / vth;
          const Real alpha = dt * ((tc <= 0.0) ? std::numeric_limits<Real>::max() : 1.0 / tc);
          for (int d = 0; d < 3; d++) {
            Real delta_d = 0.;
            const Real rhop = dens * alpha / (1.0 + alpha + bd[d]);
            const Real delta = rhop * ((vgp[d] - vd[d] + bd[d] * (vgp[d] - vdt[d])));
            delta_d += delta;
            delta_g[d] -= delta;
            delta_d -= bd[d] * dens / (1. + alpha + bd[d]) * (vd[d] - vdt[d] + alpha * (vgp[d] - vdt[d]));
            fvd[d] += rhop * (vd[d] - vt[d] + bd[d] * (vdt[d] - vt[d]));
            s.du0[(nd_ + 3 * n + d) * s.N + c] += hx[d] * delta_d;
          }
        }
        for (int d = 0; d < 3; d++) {
          const Real prefac = dg * bg[d] / (1.0 + bg[d] + fd[d]);
          delta_g[d] -= prefac * (dg * (vg[d] - vt[d]) + fvd[d]);
          *mg[d] += hx[d] * delta_g[d];
          s.gu0[(4 * ng_) * s.N + c] += 0.5 * (vg[d] + vgp[d]) * delta_g[d];
        }
      }
}

// ---------------------------------------------------------------------------------------
// Gas diffusion (artemis_driver.cpp:189-193, :218-221): ZeroDiffusionFlux, ViscousFlux,
// ThermalFlux, DiffusionUpdate and the diffusive timestep limit.
//
// Coords<GEOM>::Distance (geometry.hpp:407-412): Cartesian distance between two points given in
// the problem's coordinates.
inline Real distance(const Coords &co, const Real a[3], const Real b[3]) {
  Real xc1[3], xc2[3];
  co.ConvertToCart(a, xc1);
  co.ConvertToCart(b, xc2);
  return std::sqrt(SQR(xc1[0] - xc2[0]) + SQR(xc1[1] - xc2[1]) + SQR(xc1[2] - xc2[2]));
}
// DiffusionCoeff<DIFF>::Get / evaluate (diffusion_coeff.hpp:190-381): dynamic viscosity rho*nu or
// heat conductivity K of species n in cell (k,j,i).  EOS calls are the IdealGas closed forms
// (singularity-eos, recalled): T = sie/Cv, Cv constant, B = gamma*gm1*rho*sie.
inline Real diff_coeff_at(const Sim &s, const Sim::DiffCoeff &dp, Real dens, Real sie, int k, int j, int i);
inline Real diff_coeff(const Sim &s, const Sim::DiffCoeff &dp, int n, int k, int j, int i) {
  const int nsp = s.c.ns_gas;
  const size_t c = IDX(s, k, j, i);
  return diff_coeff_at(s, dp, s.gprim[n * s.N + c], s.gprim[(5 * nsp + n) * s.N + c], k, j, i);
}
// Get(dp, coords, dens, sie, eos) with an explicit state (drag.hpp:240,393 pass the conserved density and
// GetSpecificInternalEnergy)
inline Real diff_coeff_at(const Sim &s, const Sim::DiffCoeff &dp, Real dens, Real sie, int k, int j, int i) {
  const Coords coords(s, k, j, i);
  const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
  switch (dp.type) {
  case 1: { // viscosity_plaw, :222-224
    const CylVec cv = to_cyl_with_vec(coords, xv);
    return dp.nu_s * dens * std::pow(cv.R / dp.R0, dp.r_exp);
  }
  case 2: { // viscosity_alpha, :262-268 (spherical radius of the cell centre)
    const Real r = to_sph_radius(coords, xv); // coords.ConvertToSph(xv)[0]
    const Real Omk = dp.Omega0 * std::pow(r / dp.R0, -1.5);
    const Real gm1 = s.c.gamma - 1.0;
    const Real blk = (gm1 + 1.0) * gm1 * dens * sie;
    return dp.alpha * blk / Omk;
  }
  case 3: { // conductivity_plaw, :312-316
    const Real T = std::max(0.0, sie / s.cv);
    return dp.hcond_0 * std::pow(T / dp.T0, dp.temp_exp) * std::pow(dens / dp.d0, dp.rho_exp);
  }
  default: { // thermaldiff_plaw, :353-359
    const Real cv = s.cv;
    const Real T = std::max(0.0, sie / s.cv);
    return dp.kappa_0 * std::pow(T / dp.T0, dp.temp_exp) * std::pow(dens / dp.d0, dp.rho_exp) *
           dens * cv;
  }
  }
}
inline Real face_average(int avg, Real mu1, Real mu2) { // diffusion_coeff.hpp:139-150
  return (avg == 0) ? 0.5 * (mu1 + mu2) : 2.0 * mu1 * mu2 / (mu1 + mu2);
}

// diffusion.hpp:27-64 ZeroDiffusionImpl
void zero_diffusion_flux(Sim &s) {
  for (int d = 0; d < 3; ++d) std::fill(s.qflux[d].begin(), s.qflux[d].end(), 0.0);
}

// momentum_diffusion.hpp:562-591 VelocityDivergence of cell (k,j,i)
inline Real velocity_divergence(const Sim &s, int n, int k, int j, int i) {
  const int nsp = s.c.ns_gas;
  const int multid = (s.ndim >= 2), threed = (s.ndim == 3);
  const Coords coords(s, k, j, i);
  const Real vol = coords.Volume();
  Real a1[2], a2[2] = {0.0, 0.0}, a3[2] = {0.0, 0.0};
  coords.GetFaceAreaX1(a1);
  if (multid) coords.GetFaceAreaX2(a2);
  if (threed) coords.GetFaceAreaX3(a3);
  const Real *v1 = s.gprim.data() + (nsp + 3 * n + 0) * s.N;
  const Real *v2 = s.gprim.data() + (nsp + 3 * n + 1) * s.N;
  const Real *v3 = s.gprim.data() + (nsp + 3 * n + 2) * s.N;
  const Real divv = a1[1] * (v1[IDX(s, k, j, i)] + v1[IDX(s, k, j, i + 1)]) -
                    a1[0] * (v1[IDX(s, k, j, i)] + v1[IDX(s, k, j, i - 1)]) +
                    multid * a2[1] * (v2[IDX(s, k, j, i)] + v2[IDX(s, k, j + multid, i)]) -
                    multid * a2[0] * (v2[IDX(s, k, j, i)] + v2[IDX(s, k, j - multid, i)]) +
                    threed * a3[1] * (v3[IDX(s, k, j, i)] + v3[IDX(s, k + threed, j, i)]) -
                    threed * a3[0] * (v3[IDX(s, k, j, i)] + v3[IDX(s, k - threed, j, i)]);
  return divv / (2.0 * vol);
}

// momentum_diffusion.hpp:28-377 StrainTensorFace<XDIR>: the three components T_*^dir on the lower
// dir-face of cell (k,j,i).  Written once for the three directions with index offsets:
// `a` = the face-normal direction, `b`, `c` = the two transverse ones in cyclic x1,x2,x3 order of
// the reference's per-direction code (x1: b=x2,c=x3; x2: b=x1,c=x3; x3: b=x1,c=x2).
struct Off {
  int dk, dj, di;
};
inline void strain_face(const Sim &s, int dir, int n, int k, int j, int i, Real flx[3]) {
  const int nsp = s.c.ns_gas;
  const int multid = (s.ndim >= 2), threed = (s.ndim == 3);
  auto vel = [&](int comp, int kk, int jj, int ii) {
    return s.gprim[(nsp + 3 * n + comp) * s.N + IDX(s, kk, jj, ii)];
  };
  auto centre = [&](const Coords &co, Real x[3]) { x[0] = co.x1v(), x[1] = co.x2v(), x[2] = co.x3v(); };
  const Coords coords(s, k, j, i);
  Real xv[3], hx[3];
  centre(coords, xv);
  coords.GetScaleFactors(hx);
  const Real v[3] = {vel(0, k, j, i) / hx[0], vel(1, k, j, i) / hx[1], vel(2, k, j, i) / hx[2]};
  Real xf[3];
  if (dir == 1) coords.FaceCenX1(0, xf);
  else if (dir == 2) coords.FaceCenX2(0, xf);
  else coords.FaceCenX3(0, xf);
  const Real hxf[3] = {coords.hx1(xf[0], xf[1], xf[2]), coords.hx2(xf[0], xf[1], xf[2]),
                       coords.hx3(xf[0], xf[1], xf[2])};
  const Real fuzz = 1e-99;
  // scaled velocity component `comp` of the cell at (kk,jj,ii): v / hx_v
  auto sv = [&](int comp, int kk, int jj, int ii) {
    Real h[3];
    Coords(s, kk, jj, ii).GetScaleFactors(h);
    return vel(comp, kk, jj, ii) / h[comp];
  };
  auto dist = [&](int k1, int j1, int i1, int k2, int j2, int i2) {
    Real a[3], b[3];
    centre(Coords(s, k1, j1, i1), a);
    centre(Coords(s, k2, j2, i2), b);
    return distance(coords, a, b);
  };
  // dh_a/dx_k contraction v^k dh_a/dx_k / h_a of a cell (only dh2dx1, dh3dx1, dh3dx2 are non-zero)
  auto src_of = [&](int a, int kk, int jj, int ii) {
    const Coords co(s, kk, jj, ii);
    Real h[3];
    co.GetScaleFactors(h);
    const Real dh[3][3] = {{0.0, 0.0, 0.0}, {co.dh2dx1(), 0.0, 0.0}, {co.dh3dx1(), co.dh3dx2(), 0.0}};
    return vel(0, kk, jj, ii) / h[0] * dh[a][0] + vel(1, kk, jj, ii) / h[1] * dh[a][1] +
           vel(2, kk, jj, ii) / h[2] * dh[a][2];
  };
  if (dir == 1) {
    const Real dx1 = dist(k, j, i, k, j, i - 1);
    const Real dx2 = multid ? dist(k, j - multid, i, k, j + multid, i) : fuzz;
    const Real dx2_xm = multid ? dist(k, j - multid, i - 1, k, j + multid, i - 1) : fuzz;
    const Real dx3 = threed ? dist(k - threed, j, i, k + threed, j, i) : fuzz;
    const Real dx3_xm = threed ? dist(k - threed, j, i - 1, k + threed, j, i - 1) : fuzz;
    const Real dv1 = v[0] - sv(0, k, j, i - 1);
    const Real src = src_of(0, k, j, i);
    const Real src_xm = src_of(0, k, j, i - 1);
    flx[0] = 2 * dv1 / dx1 + 0.5 * (src + src_xm);
    const Real dv2 = v[1] - sv(1, k, j, i - 1);
    const Real dv12 = sv(0, k, j + multid, i) - sv(0, k, j - multid, i);
    const Real dv12_xm = sv(0, k, j + multid, i - 1) - sv(0, k, j - multid, i - 1);
    flx[1] = multid * 0.5 * (dv12 / dx2 + dv12_xm / dx2_xm) + SQR(hxf[1] / hxf[0]) * dv2 / dx1;
    const Real dv3 = v[2] - sv(2, k, j, i - 1);
    const Real dv13 = sv(0, k + threed, j, i) - sv(0, k - threed, j, i);
    const Real dv13_xm = sv(0, k + threed, j, i - 1) - sv(0, k - threed, j, i - 1);
    flx[2] = threed * 0.5 * (dv13 / dx3 + dv13_xm / dx3_xm) + SQR(hxf[2] / hxf[0]) * dv3 / dx1;
  } else if (dir == 2) {
    const Real dx1 = dist(k, j, i - 1, k, j, i + 1);
    const Real dx1_ym = dist(k, j - 1, i - 1, k, j - 1, i + 1);
    const Real dx2 = dist(k, j, i, k, j - 1, i);
    const Real dx3 = threed ? dist(k - threed, j, i, k + threed, j, i) : fuzz;
    const Real dx3_ym = threed ? dist(k - threed, j - 1, i, k + threed, j - 1, i) : fuzz;
    const Real dv1 = v[0] - sv(0, k, j - 1, i);
    const Real dv21 = sv(1, k, j, i + 1) - sv(1, k, j, i - 1);
    const Real dv21_ym = sv(1, k, j - 1, i + 1) - sv(1, k, j - 1, i - 1);
    flx[0] = 0.5 * (dv21 / dx1 + dv21_ym / dx1_ym) + SQR(hxf[0] / hxf[1]) * dv1 / dx2;
    const Real dv2 = v[1] - sv(1, k, j - 1, i);
    const Real src = src_of(1, k, j, i);
    const Real src_ym = src_of(1, k, j - 1, i);
    flx[1] = 2 * dv2 / dx2 + 0.5 * (src + src_ym);
    const Real dv3 = v[2] - sv(2, k, j - 1, i);
    const Real dv23 = sv(1, k + threed, j, i) - sv(1, k - threed, j, i);
    const Real dv23_ym = sv(1, k + threed, j - 1, i) - sv(1, k - threed, j - 1, i);
    flx[2] = threed * 0.5 * (dv23 / dx3 + dv23_ym / dx3_ym) + SQR(hxf[2] / hxf[1]) * dv3 / dx2;
  } else {
    const Real dx1 = dist(k, j, i - 1, k, j, i + 1);
    const Real dx1_zm = dist(k - 1, j, i - 1, k - 1, j, i + 1);
    const Real dx2 = dist(k, j - 1, i, k, j + 1, i);
    const Real dx2_zm = dist(k - 1, j - 1, i, k - 1, j + 1, i);
    const Real dx3 = dist(k, j, i, k - 1, j, i);
    const Real dv1 = v[0] - sv(0, k - 1, j, i);
    const Real dv31 = sv(2, k, j, i + 1) - sv(2, k, j, i - 1);
    const Real dv31_zm = sv(2, k - 1, j, i + 1) - sv(2, k - 1, j, i - 1);
    flx[0] = 0.5 * (dv31 / dx1 + dv31_zm / dx1_zm) + SQR(hxf[0] / hxf[2]) * dv1 / dx3;
    const Real dv2 = v[1] - sv(1, k - 1, j, i);
    const Real dv32 = sv(2, k, j + 1, i) - sv(2, k, j - 1, i);
    const Real dv32_zm = sv(2, k - 1, j + 1, i) - sv(2, k - 1, j - 1, i);
    flx[1] = 0.5 * (dv32 / dx2 + dv32_zm / dx2_zm) + SQR(hxf[1] / hxf[2]) * dv2 / dx3;
    const Real dv3 = v[2] - sv(2, k - 1, j, i);
    const Real src = src_of(2, k, j, i);
    const Real src_zm = src_of(2, k - 1, j, i);
    flx[2] = 2 * dv3 / dx3 + 0.5 * (src + src_zm);
  }
}

// momentum_diffusion.hpp:597-755 MomentumFluxImpl + StressTensorFaceX1/2/3 (:379-560): viscous
// momentum and energy fluxes ADDED to the diffusion flux arrays on faces [s, e+1] of each active
// direction (the face's value is a pure function of its neighbourhood, so the reference's
// scratch-row bookkeeping reduces to a loop over faces).
void viscous_flux(Sim &s) {
  const Sim::DiffCoeff &dp = s.visc;
  if (dp.type == 0 || !s.c.ns_gas) return;
  const int nsp = s.c.ns_gas;
  for (int dir = 1; dir <= s.ndim; ++dir) {
    const int dk = (dir == 3), dj = (dir == 2), di = (dir == 1);
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = s.ks; k <= s.ke + dk; ++k)
      for (int j = s.js; j <= s.je + dj; ++j)
        for (int i = s.is; i <= s.ie + di; ++i) {
          const Coords coords(s, k, j, i), coords_m(s, k - dk, j - dj, i - di);
          Real hx[3], hx_m[3], xf[3];
          coords.GetScaleFactors(hx), coords_m.GetScaleFactors(hx_m);
          Real hf;
          if (dir == 1) coords.FaceCenX1(0, xf), hf = coords.hx1(xf[0], xf[1], xf[2]);
          else if (dir == 2) coords.FaceCenX2(0, xf), hf = coords.hx2(xf[0], xf[1], xf[2]);
          else coords.FaceCenX3(0, xf), hf = coords.hx3(xf[0], xf[1], xf[2]);
          const size_t c = IDX(s, k, j, i), cm = IDX(s, k - dk, j - dj, i - di);
          for (int n = 0; n < nsp; ++n) {
            Real flx[3];
            strain_face(s, dir, n, k, j, i, flx);
            const Real mu = diff_coeff(s, dp, n, k, j, i);
            const Real mu_m = diff_coeff(s, dp, n, k - dk, j - dj, i - di);
            const Real divu = velocity_divergence(s, n, k, j, i);
            const Real divu_m = velocity_divergence(s, n, k - dk, j - dj, i - di);
            const Real mus = (dp.avg == 0) * face_average(0, mu, mu_m) + (dp.avg == 1) * face_average(1, mu, mu_m);
            Real f[3];
            for (int q = 0; q < 3; ++q) f[q] = hf * mus * flx[q];
            // the normal component carries the bulk term (:411, :468, :524)
            f[dir - 1] = hf * mus * (flx[dir - 1] - 1. / 3 * (1. - dp.eta) * (divu + divu_m));
            RVec &qf = s.qflux[dir - 1];
            for (int q = 0; q < 3; ++q) qf[(3 * n + q) * s.N + c] += f[q];
            const Real *v1 = s.gprim.data() + (nsp + 3 * n + 0) * s.N;
            const Real *v2 = s.gprim.data() + (nsp + 3 * n + 1) * s.N;
            const Real *v3 = s.gprim.data() + (nsp + 3 * n + 2) * s.N;
            qf[(3 * nsp + n) * s.N + c] += 0.5 * (v1[c] / hx[0] + v1[cm] / hx_m[0]) * f[0] +
                                           0.5 * (v2[c] / hx[1] + v2[cm] / hx_m[1]) * f[1] +
                                           0.5 * (v3[c] / hx[2] + v3[cm] / hx_m[2]) * f[2];
          }
        }
  }
}

// thermal_diffusion.hpp:30-222 ThermalFluxImpl: F = K (T - T_m) / |x - x_m| added to the energy
// diffusion flux on faces [s, e+1] of each active direction.
void thermal_flux(Sim &s) {
  const Sim::DiffCoeff &dp = s.cond;
  if (dp.type == 0 || !s.c.ns_gas) return;
  const int nsp = s.c.ns_gas;
  for (int dir = 1; dir <= s.ndim; ++dir) {
    const int dk = (dir == 3), dj = (dir == 2), di = (dir == 1);
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = s.ks; k <= s.ke + dk; ++k)
      for (int j = s.js; j <= s.je + dj; ++j)
        for (int i = s.is; i <= s.ie + di; ++i) {
          const Coords coords(s, k, j, i), coords_m(s, k - dk, j - dj, i - di);
          const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
          const Real xv_m[3] = {coords_m.x1v(), coords_m.x2v(), coords_m.x3v()};
          const Real dx = distance(coords, xv, xv_m);
          const size_t c = IDX(s, k, j, i), cm = IDX(s, k - dk, j - dj, i - di);
          for (int n = 0; n < nsp; ++n) {
            const Real T = std::max(0.0, s.gprim[(5 * nsp + n) * s.N + c] / s.cv);
            const Real Tm = std::max(0.0, s.gprim[(5 * nsp + n) * s.N + cm] / s.cv);
            const Real ka = diff_coeff(s, dp, n, k, j, i);
            const Real kb = diff_coeff(s, dp, n, k - dk, j - dj, i - di);
            const Real kcond = (dp.avg == 0) * face_average(0, ka, kb) + (dp.avg == 1) * face_average(1, ka, kb);
            s.qflux[dir - 1][(3 * nsp + n) * s.N + c] += kcond * (T - Tm) / dx;
          }
        }
  }
}

// diffusion.hpp:110-241 DiffusionUpdateImpl
void diffusion_update(Sim &s, Real dt) {
  if ((s.visc.type == 0 && s.cond.type == 0) || !s.c.ns_gas) return;
  const bool do_viscosity = (s.visc.type != 0);
  const int nsp = s.c.ns_gas;
  const int multi_d = (s.ndim > 1), three_d = (s.ndim > 2);
  const ptrdiff_t sj = s.ni, sk = static_cast<ptrdiff_t>(s.ni) * s.nj;
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const Coords coords(s, k, j, i);
        const bool x1dep = coords.x1dep();
        const bool x2dep = coords.x2dep() && multi_d;
        const bool x3dep = false;
        Real ax1[2], ax2[2] = {0.0, 0.0}, ax3[2] = {0.0, 0.0};
        coords.GetFaceAreaX1(ax1);
        if (multi_d) coords.GetFaceAreaX2(ax2);
        if (three_d) coords.GetFaceAreaX3(ax3);
        Real dhdx1[3] = {0.0, 0.0, 0.0}, dhdx2[3] = {0.0, 0.0, 0.0}, dhdx3[3] = {0.0, 0.0, 0.0};
        if (x1dep) coords.GetConnX1(dhdx1);
        if (x2dep) coords.GetConnX2(dhdx2);
        Real hx[3];
        coords.GetScaleFactors(hx);
        const Real vol = coords.Volume();
        const size_t c = IDX(s, k, j, i);
        const size_t c2 = c + multi_d * sj, c3 = c + three_d * sk;
        for (int n = 0; n < nsp; ++n) {
          auto F = [&](int d, int var, size_t cc) { return s.qflux[d][var * s.N + cc]; };
          const int imx1 = 3 * n + 0, imx2 = 3 * n + 1, imx3 = 3 * n + 2, ien = 3 * nsp + n;
          Real divfxm = 0., divfym = 0., divfzm = 0.;
          if (do_viscosity) {
            auto divergence = [&](int var) {
              return (ax1[0] * F(0, var, c) - ax1[1] * F(0, var, c + 1)) +
                     multi_d * (ax2[0] * F(1, var, c) - ax2[1] * F(1, var, c2)) +
                     three_d * (ax3[0] * F(2, var, c) - ax3[1] * F(2, var, c3));
            };
            auto metric_src = [&](const Real dh[3]) {
              return dh[0] * 0.5 * (F(0, imx1, c) + F(0, imx1, c + 1)) +
                     multi_d * dh[1] * 0.5 * (F(1, imx2, c) + F(1, imx2, c2)) +
                     three_d * dh[2] * 0.5 * (F(2, imx3, c) + F(2, imx3, c3));
            };
            divfxm = divergence(imx1);
            divfxm /= vol;
            divfxm += x1dep * metric_src(dhdx1);
            divfym = divergence(imx2);
            divfym /= vol;
            divfym += x2dep * metric_src(dhdx2);
            divfzm = divergence(imx3);
            divfzm /= vol;
            divfzm += x3dep * metric_src(dhdx3);
          }
          Real divfe = (ax1[0] * F(0, ien, c) - ax1[1] * F(0, ien, c + 1)) +
                       multi_d * (ax2[0] * F(1, ien, c) - ax2[1] * F(1, ien, c2)) +
                       three_d * (ax3[0] * F(2, ien, c) - ax3[1] * F(2, ien, c3));
          divfe /= vol;
          s.gu0[(nsp + 3 * n + 0) * s.N + c] -= dt * divfxm;
          s.gu0[(nsp + 3 * n + 1) * s.N + c] -= dt * divfym;
          s.gu0[(nsp + 3 * n + 2) * s.N + c] -= dt * divfzm;
          s.gu0[(4 * nsp + n) * s.N + c] -= dt * divfe;
          s.gu0[(5 * nsp + n) * s.N + c] -=
              dt * divfe - dt * (divfxm * s.gprim[(nsp + 3 * n + 0) * s.N + c] / hx[0] +
                                 divfym * s.gprim[(nsp + 3 * n + 1) * s.N + c] / hx[1] +
                                 divfzm * s.gprim[(nsp + 3 * n + 2) * s.N + c] / hx[2]);
        }
      }
}

// diffusion.hpp:66-108 EstimateTimestep<DIFF>: min over cells of dx_min^2 / diffusivity, / (2 ndim)
Real diffusion_dt(const Sim &s, const Sim::DiffCoeff &dp) {
  Real min_dt = std::numeric_limits<Real>::max();
  if (dp.type == 0 || !s.c.ns_gas) return min_dt;
  const int nsp = s.c.ns_gas;
#pragma omp parallel for collapse(2) schedule(static) reduction(min : min_dt)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        Real dx[3];
        Coords(s, k, j, i).GetCellWidths(dx);
        Real min_dx = std::numeric_limits<Real>::max();
        for (int d = 0; d < s.ndim; d++) min_dx = std::min(min_dx, dx[d]);
        const size_t c = IDX(s, k, j, i);
        for (int n = 0; n < nsp; ++n) {
          const Real dens = s.gprim[n * s.N + c];
          Real mu = diff_coeff(s, dp, n, k, j, i);
          if (dp.type == 3) mu /= (dens * s.cv);
          else if (dp.type == 1 || dp.type == 2) mu *= (1.0 + (dp.eta > 1.0) * (dp.eta - 1.0)) / dens;
          min_dt = std::min(min_dt, SQR(min_dx) / (mu + 1e-99));
        }
      }
  return min_dt / (2.0 * s.ndim);
}

// ---------------------------------------------------------------------------------------
// gas/cooling/beta_cooling.cpp:40-126 BetaCooling<GEOM, powerlaw> (cooling.cpp:94-106 dispatch,
// cooling.hpp:47-58 TemperatureProfile): backward-Euler relaxation of T towards T0(R, r) on the
// local orbital time scaled by beta; acts on the conserved total and internal energies.
void cooling_source(Sim &s, Real /*time*/, Real dt) {
  if (!s.cool.on || !s.c.ns_gas) return;
  const int nsp = s.c.ns_gas;
  const Real gm = (s.grav.type != 0) ? s.grav.gm : std::numeric_limits<Real>::quiet_NaN(); // Null<Real>()
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const Coords coords(s, k, j, i);
        const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
        const Frame fr = to_cyl_frame(coords, xv);
        const Real *xcyl = fr.x;
        const Real rsph2 = xcyl[0] * xcyl[0] + xcyl[2] * xcyl[2];
        Real ir1 = 1.0 / std::sqrt(rsph2);
        const Real T0 = s.cool.tfloor + s.cool.tcyl * std::pow(xcyl[0], s.cool.cyl_plaw) +
                        s.cool.tsph * std::pow(to_sph_radius(coords, xv), s.cool.sph_plaw);
        const Real efac = (T0 > 0.) ? std::exp(-s.cool.escale * xcyl[2] * xcyl[2] / T0) : 1.;
        const Real beta = s.cool.beta_min + s.cool.beta0 * efac;
        const Real omdt = dt * std::sqrt(gm * ir1 * ir1 * ir1);
        Real hx[3];
        coords.GetScaleFactors(hx);
        const size_t c = IDX(s, k, j, i);
        for (int n = 0; n < nsp; ++n) {
          const Real sie = specific_internal_energy(s, n, c, hx);
          const Real dens = s.gu0[n * s.N + c];
          const Real cv = s.cv;
          const Real Tn = std::max(0.0, sie / s.cv);
          const Real dE = -dens * cv * omdt / (beta + omdt) * (Tn - T0);
          s.gu0[(4 * nsp + n) * s.N + c] += dE;
          s.gu0[(5 * nsp + n) * s.N + c] += dE;
        }
      }
}

// ---------------------------------------------------------------------------------------
// derived/fill_derived.cpp:30-75 SetAuxillaryFields + utils/artemis_utils.hpp:43-62
// GetSpecificInternalEnergy (hx = volume-averaged scale factors, fill_derived.cpp:127 analogue).
void set_aux(Sim &s) {
  const int nsp = s.c.ns_gas;
  if (!nsp) return;
  const Real dflr = s.c.dfloor_gas, sieflr = s.c.siefloor_gas, de_switch = s.c.de_switch;
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const size_t c = IDX(s, k, j, i);
        Real hx[3];
        Coords(s, k, j, i).GetScaleFactors(hx); // artemis_utils.hpp:73-75
        for (int n = 0; n < nsp; ++n) {
          Real u_d = s.gu0[n * s.N + c];
          u_d = (u_d > dflr) ? u_d : dflr;
          // GetSpecificInternalEnergy
          const Real u_d2 = std::max(s.gu0[n * s.N + c], dflr);
          const Real rv1 = s.gu0[(nsp + 3 * n + 0) * s.N + c] / hx[0];
          const Real rv2 = s.gu0[(nsp + 3 * n + 1) * s.N + c] / hx[1];
          const Real rv3 = s.gu0[(nsp + 3 * n + 2) * s.N + c] / hx[2];
          const Real ke = 0.5 * (SQR(rv1) + SQR(rv2) + SQR(rv3)) / u_d2;
          const Real e_cons = s.gu0[(4 * nsp + n) * s.N + c];
          const Real ue_cons = e_cons - ke;
          Real sie = (ue_cons > de_switch * e_cons) ? ue_cons / u_d2
                                                    : s.gu0[(5 * nsp + n) * s.N + c] / u_d2;
          sie = std::max(sie, sieflr);
          Real &u_u = s.gu0[(5 * nsp + n) * s.N + c];
          u_u = sie * u_d;
          const Real uflr = sieflr * u_d;
          u_u = (u_u > uflr) ? u_u : uflr;
        }
      }
}

// derived/fill_derived.cpp:82-167 ConsToPrim (interior)
void cons_to_prim(Sim &s) {
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
#pragma omp parallel for collapse(2) schedule(static)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const size_t c = IDX(s, k, j, i);
        Real hx[3];
        Coords(s, k, j, i).GetScaleFactors(hx); // fill_derived.cpp:125-127, :217-219
        for (int n = 0; n < ng_; ++n) {
          const Real u_d = s.gu0[n * s.N + c];
          Real &w_d = s.gprim[n * s.N + c];
          w_d = (u_d > s.c.dfloor_gas) ? u_d : s.c.dfloor_gas;
          for (int d = 0; d < 3; ++d)
            s.gprim[(ng_ + 3 * n + d) * s.N + c] =
                s.gu0[(ng_ + 3 * n + d) * s.N + c] / (w_d * hx[d]);
          const Real w_s = s.gu0[(5 * ng_ + n) * s.N + c] / w_d;
          s.gprim[(5 * ng_ + n) * s.N + c] = (w_s > s.c.siefloor_gas) ? w_s : s.c.siefloor_gas;
        }
        for (int n = 0; n < nd_; ++n) {
          const Real u_d = s.du0[n * s.N + c];
          Real &w_d = s.dprim[n * s.N + c];
          w_d = (u_d > s.c.dfloor_dust) ? u_d : s.c.dfloor_dust;
          for (int d = 0; d < 3; ++d)
            s.dprim[(nd_ + 3 * n + d) * s.N + c] =
                s.du0[(nd_ + 3 * n + d) * s.N + c] / (w_d * hx[d]);
        }
      }
}

// derived/fill_derived.cpp:173-277 PrimToCons (entire block, ghosts included).  Pressure is
// singularity-eos IdealGas::PressureFromDensityInternalEnergy = gm1*rho*sie (recalled; its
// max(0,.) clamp is inactive because both factors are floored positive).
void prim_to_cons(Sim &s) {
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const Real gm1 = s.c.gamma - 1.0;
#pragma omp parallel for schedule(static)
  for (int k = 0; k < s.nk; ++k)
    for (int j = 0; j < s.nj; ++j)
      for (int i = 0; i < s.ni; ++i) {
        const size_t c = IDX(s, k, j, i);
        Real hx[3];
        Coords(s, k, j, i).GetScaleFactors(hx); // fill_derived.cpp:125-127, :217-219
        for (int n = 0; n < ng_; ++n) {
          Real &w_d = s.gprim[n * s.N + c];
          Real &u_d = s.gu0[n * s.N + c];
          w_d = (w_d > s.c.dfloor_gas) ? w_d : s.c.dfloor_gas;
          u_d = w_d;
          const Real vel1 = s.gprim[(ng_ + 3 * n + 0) * s.N + c];
          const Real vel2 = s.gprim[(ng_ + 3 * n + 1) * s.N + c];
          const Real vel3 = s.gprim[(ng_ + 3 * n + 2) * s.N + c];
          s.gu0[(ng_ + 3 * n + 0) * s.N + c] = w_d * vel1 * hx[0];
          s.gu0[(ng_ + 3 * n + 1) * s.N + c] = w_d * vel2 * hx[1];
          s.gu0[(ng_ + 3 * n + 2) * s.N + c] = w_d * vel3 * hx[2];
          Real &w_s = s.gprim[(5 * ng_ + n) * s.N + c];
          Real &w_p = s.gprim[(4 * ng_ + n) * s.N + c];
          Real &u_u = s.gu0[(5 * ng_ + n) * s.N + c];
          w_s = (w_s > s.c.siefloor_gas) ? w_s : s.c.siefloor_gas;
          u_u = w_s * u_d;
          w_p = std::max(0.0, gm1 * w_d * w_s);
          const Real ke = 0.5 * w_d * (SQR(vel1) + SQR(vel2) + SQR(vel3));
          s.gu0[(4 * ng_ + n) * s.N + c] = u_u + ke;
        }
        for (int n = 0; n < nd_; ++n) {
          Real &w_d = s.dprim[n * s.N + c];
          Real &u_d = s.du0[n * s.N + c];
          w_d = (w_d > s.c.dfloor_dust) ? w_d : s.c.dfloor_dust;
          u_d = w_d;
          for (int d = 0; d < 3; ++d)
            s.du0[(nd_ + 3 * n + d) * s.N + c] =
                w_d * s.dprim[(nd_ + 3 * n + d) * s.N + c] * hx[d];
        }
      }
}

// ---------------------------------------------------------------------------------------
// gas/gas.cpp:392-433 and dust/dust.cpp:239-276 EstimateTimestepMesh (cfl applied at :467 /
// :275).  Bulk modulus = gamma*gm1*rho*sie (singularity-eos IdealGas, recalled:
// BulkModulusFromDensityInternalEnergy = (gm1+1)*gm1*rho*sie).
Real estimate_dt(const Sim &s, int fluid) {
  Real min_dt = std::numeric_limits<Real>::max();
  const Real gm1 = s.c.gamma - 1.0;
  const int nsp = (fluid == FL_GAS) ? s.c.ns_gas : s.c.ns_dust;
#pragma omp parallel for collapse(2) schedule(static) reduction(min : min_dt)
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        Real dx[3];
        Coords(s, k, j, i).GetCellWidths(dx); // gas.cpp:416-417
        const size_t c = IDX(s, k, j, i);
        for (int n = 0; n < nsp; ++n) {
          Real denom = 0.0;
          if (fluid == FL_GAS) {
            const Real dens = s.gprim[n * s.N + c];
            const Real sie = s.gprim[(5 * nsp + n) * s.N + c];
            const Real bulk = (gm1 + 1.0) * gm1 * dens * sie;
            const Real cs = std::sqrt(bulk / dens);
            for (int d = 0; d < s.ndim; d++) {
              const Real ss = std::abs(s.gprim[(nsp + 3 * n + d) * s.N + c]) + cs;
              denom += ss / dx[d];
            }
          } else {
            for (int d = 0; d < s.ndim; d++)
              denom += std::abs(s.dprim[(nsp + 3 * n + d) * s.N + c]) / dx[d];
          }
          min_dt = std::min(min_dt, 1.0 / denom);
        }
      }
  if (fluid == FL_GAS) { // gas.cpp:435-467: cfl * min(hydro, viscous, conductive)
    const Real diff_dt = std::min(diffusion_dt(s, s.visc), diffusion_dt(s, s.cond));
    return s.c.cfl_gas * std::min(min_dt, diff_dt);
  }
  return s.c.cfl_dust * min_dt;
}

// ---------------------------------------------------------------------------------------
// Ghost fill of the FillGhost variables = primitives rho, v, sie (gas; pressure is not
// FillGhost, gas.cpp:251-252) and rho, v (dust, dust.cpp:201-213).  Parthenon semantics
// (upstream, recalled): periodic images arrive by communication first, then physical BCs are
// applied in the order x1, x2, x3, each over the ENTIRE extent of the other two dimensions
// (IndexDomain::inner_x1 etc.), so edges/corners inherit from the previously filled faces.
// outflow: copy the nearest interior cell; reflecting: mirror about the face and flip the sign
// of the vector component normal to it.
void fill_dir(Sim &s, RVec &prim, int nvar, int nsp, bool gas, int d, int pass) {
  // pass 0: periodic only; pass 1: physical only
  const int n_act[3] = {s.c.nx1, s.c.nx2, s.c.nx3};
  if (d >= s.ndim) return;
  const int ng = s.c.ng;
  const int st[3] = {s.is, s.js, s.ks}, en[3] = {s.ie, s.je, s.ke};
  const int ext[3] = {s.ni, s.nj, s.nk};
  for (int side = 0; side < 2; ++side) {
    const int bc = s.c.bc[2 * d + side];
    if (bc == BC_NONE || bc == BC_STRAT_EXTRAP || bc == BC_STRAT_INFLOW || bc == BC_CONDUCTIVE ||
        bc == BC_DISK_IC || bc == BC_DISK_EXTRAP || bc == BC_DISK_VISC)
      continue;
    if ((pass == 0) != (bc == BC_PERIODIC)) continue;
    for (int n = 0; n < nvar; ++n) {
      if (gas && n >= 4 * nsp && n < 5 * nsp) continue; // pressure slot is not FillGhost
      const bool is_vel = (n >= nsp && n < 4 * nsp);
      const bool normal = is_vel && (((n - nsp) % 3) == d);
      Real *q = prim.data() + n * s.N;
      for (int g = 0; g < ng; ++g) {
        // ghost index along d and its source index
        int gi, si;
        if (side == 0) {
          gi = st[d] - 1 - g;
          if (bc == BC_PERIODIC) si = gi + n_act[d];
          else if (bc == BC_OUTFLOW) si = st[d];
          else si = 2 * st[d] - 1 - gi;
        } else {
          gi = en[d] + 1 + g;
          if (bc == BC_PERIODIC) si = gi - n_act[d];
          else if (bc == BC_OUTFLOW) si = en[d];
          else si = 2 * en[d] + 1 - gi;
        }
        const Real sgn = (bc == BC_REFLECT && normal) ? -1.0 : 1.0;
        int lo[3] = {0, 0, 0}, hi[3] = {ext[0] - 1, ext[1] - 1, ext[2] - 1};
        lo[d] = hi[d] = gi;
        for (int k = lo[2]; k <= hi[2]; ++k)
          for (int j = lo[1]; j <= hi[1]; ++j)
            for (int i = lo[0]; i <= hi[0]; ++i) {
              int src[3] = {i, j, k};
              src[d] = si;
              q[IDX(s, k, j, i)] = sgn * q[IDX(s, src[2], src[1], src[0])];
            }
      }
    }
  }
}
// pgen/strat.hpp:158-466: the `strat` problem's user boundary conditions, registered for
// `extrap` (x1, x3) and `inflow` (x2) (problem_modifier.hpp:114-128).  par_for_bndry covers the
// ghost zones of direction d over the ENTIRE extent of the other two (upstream parthenon), like
// the built-in conditions.  x1 `extrap`: density / sie / v3 copied from the first active zone,
// v1 copied unless it points into the domain, v2 extrapolated linearly in x (:188-226,
// :262-299).  x2 `inflow`: copy, except v2 = Keplerian shear where the box inflows (x_face >= 0
// at the inner edge, < 0 at the outer) and one-way outflow elsewhere (:352-392, :437-466).
// The x3 `extrap` condition uses std::pow on the density ratio (:520-523) and is not restated.
void strat_bc(Sim &s, int d, int side) {
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const int lo[3] = {s.is, s.js, s.ks}, hi[3] = {s.ie, s.je, s.ke};
  int b0[3] = {0, 0, 0}, b1[3] = {s.ni - 1, s.nj - 1, s.nk - 1};
  if (side == 0) b1[d] = lo[d] - 1;
  else b0[d] = hi[d] + 1;
  for (int k = b0[2]; k <= b1[2]; ++k)
    for (int j = b0[1]; j <= b1[1]; ++j)
      for (int i = b0[0]; i <= b1[0]; ++i) {
        const size_t c = IDX(s, k, j, i);
        if (d == 0) {
          const int ia = (side == 0) ? s.is : s.ie, ib = (side == 0) ? s.is + 1 : s.ie - 1;
          const Real x0 = x1v(bbox(s, k, j, ia));
          const Real x1 = x1v(bbox(s, k, j, ib));
          const Real dx = (side == 0) ? (x1 - x0) : (x0 - x1);
          const Real x = x1v(bbox(s, k, j, i));
          const size_t ca = IDX(s, k, j, ia), cb = IDX(s, k, j, ib);
          auto fill = [&](RVec &q, int nsp, int n) {
            const Real v1 = q[(nsp + 3 * n + 0) * s.N + ca];
            const Real v2 = q[(nsp + 3 * n + 1) * s.N + ca];
            const Real v3 = q[(nsp + 3 * n + 2) * s.N + ca];
            const Real v2n = q[(nsp + 3 * n + 1) * s.N + cb];
            const Real vx1 = (side == 0) ? ((v1 > 0.0) ? 0.0 : v1) : ((v1 < 0.0) ? 0.0 : v1);
            const Real vx2 = (side == 0) ? (v2 + (v2n - v2) * (x - x0) / dx)
                                         : (v2 + (v2 - v2n) * (x - x0) / dx);
            q[(nsp + 3 * n + 0) * s.N + c] = vx1;
            q[(nsp + 3 * n + 1) * s.N + c] = vx2;
            q[(nsp + 3 * n + 2) * s.N + c] = v3;
            q[n * s.N + c] = q[n * s.N + ca];
          };
          if (ng_) {
            fill(s.gprim, ng_, 0);
            s.gprim[(5 * ng_) * s.N + c] = s.gprim[(5 * ng_) * s.N + ca];
          }
          for (int n = 0; n < nd_; ++n)
            fill(s.dprim, nd_, n);
        } else if (d == 2) { // strat.hpp:476-555 ExtrapInnerX3, :559-640 ExtrapOuterX3
          const int ka = (side == 0) ? s.ks : s.ke, kb = (side == 0) ? s.ks + 1 : s.ke - 1;
          const Real z = x3v(bbox(s, k, j, i));
          const Real z0 = x3v(bbox(s, ka, j, i));
          const Real z1 = x3v(bbox(s, kb, j, i));
          const Real dz = (side == 0) ? (z1 - z0) : (z0 - z1);
          const size_t ca = IDX(s, ka, j, i), cb = IDX(s, kb, j, i);
          auto fill = [&](RVec &q, int nsp, int n) {
            const Real v1 = q[(nsp + 3 * n + 0) * s.N + ca];
            const Real v2 = q[(nsp + 3 * n + 1) * s.N + ca];
            const Real v3 = q[(nsp + 3 * n + 2) * s.N + ca];
            const Real vx3 = (side == 0) ? ((v3 > 0.0) ? 0.0 : v3) : ((v3 < 0.0) ? 0.0 : v3);
            const Real dd = q[n * s.N + ca];
            const Real dn = q[n * s.N + cb];
            const Real drho = (side == 0) ? dn / dd : dd / dn;
            const Real dens = dd * std::pow(drho, (z - z0) / dz);
            q[(nsp + 3 * n + 0) * s.N + c] = v1;
            q[(nsp + 3 * n + 1) * s.N + c] = v2;
            q[(nsp + 3 * n + 2) * s.N + c] = vx3;
            q[n * s.N + c] = dens;
          };
          if (ng_) {
            fill(s.gprim, ng_, 0);
            s.gprim[(5 * ng_) * s.N + c] = s.gprim[(5 * ng_) * s.N + ca];
          }
          for (int n = 0; n < nd_; ++n)
            fill(s.dprim, nd_, n);
        } else {
          const int ja = (side == 0) ? s.js : s.je;
          const BBox b = bbox(s, k, j, i);
          const Real x = x1v(b);
          const Real xf = b.x1[0];
          const Real vy0 = -s.strat.q * s.strat.Om0 * x;
          const size_t ca = IDX(s, k, ja, i);
          auto fill = [&](RVec &q, int nsp, int n) {
            const Real v1 = q[(nsp + 3 * n + 0) * s.N + ca];
            const Real v2 = q[(nsp + 3 * n + 1) * s.N + ca];
            const Real v3 = q[(nsp + 3 * n + 2) * s.N + ca];
            const Real vx2 = (side == 0) ? ((xf >= 0) ? ((v2 > 0.) ? 0.0 : v2) : vy0)
                                         : ((xf < 0) ? ((v2 < 0.0) ? 0.0 : v2) : vy0);
            q[(nsp + 3 * n + 0) * s.N + c] = v1;
            q[(nsp + 3 * n + 1) * s.N + c] = vx2;
            q[(nsp + 3 * n + 2) * s.N + c] = v3;
            q[n * s.N + c] = q[n * s.N + ca];
          };
          if (ng_) {
            fill(s.gprim, ng_, 0);
            s.gprim[(5 * ng_) * s.N + c] = s.gprim[(5 * ng_) * s.N + ca];
          }
          for (int n = 0; n < nd_; ++n)
            fill(s.dprim, nd_, n);
        }
      }
}
// pgen/conduction.hpp:105-232 CondBoundaryImpl (`conductive`, problem = conduction): fixed heat flux
// through the inner face, fixed temperature at the outer one, hydrostatic density, velocities
// copied from the first active zone.  `ia` = the active zone next to the boundary along d.
void conductive_bc(Sim &s, int d, int side) {
  const int nsp = s.c.ns_gas;
  if (!nsp) return;
  const bool INNER = (side == 0);
  const int lo[3] = {s.is, s.js, s.ks}, hi[3] = {s.ie, s.je, s.ke};
  int b0[3] = {0, 0, 0}, b1[3] = {s.ni - 1, s.nj - 1, s.nk - 1};
  if (INNER) b1[d] = lo[d] - 1;
  else b0[d] = hi[d] + 1;
  const Real gx1 = (s.grav.type == 1) ? s.grav.g[d] : 0.0; // :181-196
  const Real gm1 = s.c.gamma - 1.0;
  for (int k = b0[2]; k <= b1[2]; ++k)
    for (int j = b0[1]; j <= b1[1]; ++j)
      for (int i = b0[0]; i <= b1[0]; ++i) {
        int ia[3] = {i, j, k};
        ia[d] = INNER ? lo[d] : hi[d];
        const Coords coords(s, k, j, i), ca(s, ia[2], ia[1], ia[0]);
        const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
        const Real xva[3] = {ca.x1v(), ca.x2v(), ca.x3v()};
        const Real xma = (INNER ? -1. : 1.) * distance(coords, xv, xva);
        const size_t c = IDX(s, k, j, i), cA = IDX(s, ia[2], ia[1], ia[0]);
        const Real da = s.gprim[0 * s.N + cA];
        const Real siea = s.gprim[(5 * nsp) * s.N + cA];
        const Real Ta = std::max(0.0, siea / s.cv);
        const Real Pa = std::max(0.0, gm1 * da * siea);
        (void)Pa;
        const Real ka = diff_coeff(s, s.cond, 0, ia[2], ia[1], ia[0]);
        Real Tg = s.condbc.g_temp;
        if (INNER) Tg = Ta - s.condbc.flux * xma / ka;
        const Real densg = da * (Ta - 0.5 * gx1 * xma) / (Tg + 0.5 * gx1 * xma);
        const Real sieg = std::max(0.0, s.cv * Tg);
        s.gprim[0 * s.N + c] = densg;
        s.gprim[(5 * nsp) * s.N + c] = sieg;
        for (int q = 0; q < 3; ++q) s.gprim[(nsp + q) * s.N + c] = s.gprim[(nsp + q) * s.N + cA];
      }
}
// ---------------------------------------------------------------------------------------
// pgen/disk.hpp:69-135 profiles.  IdealGas closed forms (singularity-eos, recalled):
// P(rho, T) = gm1 rho Cv T, sie(rho, T) = Cv T.
inline Real disk_den(const Sim::DiskParams &pg, const Real R, const Real z) {
  const Real r = std::sqrt(R * R + z * z);
  const Real h = pg.h0 * std::pow(R / pg.r0, pg.flare);
  const Real sig0 = pg.rho0;
  const Real exp_fac = (pg.rexp == 0.) ? 1. : std::exp(-SQR(R / pg.rexp));
  const Real dmid = (sig0 * std::pow(R / pg.r0, pg.p)) * (1. - pg.l0 * std::sqrt(pg.r0 / R)) *
                    (pg.dens_min / pg.rho0 +
                     (1. - pg.dens_min / pg.rho0) * std::exp(-std::pow(pg.rcav / R, 12.0))) *
                    exp_fac;
  const Real sint = (r == 0.0) ? 1.0 : R / r;
  const Real efac = (1. - sint) / (h * h);
  if (pg.Gamma == 1.) return std::max(pg.dens_min, dmid * std::exp(-efac));
  const Real pfac = 1. - (pg.Gamma - 1) * efac;
  return std::max(pg.dens_min, dmid * std::pow(pfac + 1e-99, 1. / (pg.Gamma - 1)));
}
inline Real disk_temp(const Sim::DiskParams &pg, const Real R, const Real z) {
  const Real rho = disk_den(pg, R, z);
  const Real rho0 = disk_den(pg, R, 0.0);
  const Real H = R * pg.h0 * std::pow(R / pg.r0, pg.flare);
  const Real ir1 = 1.0 / std::sqrt(R * R + pg.temp_soft2);
  const Real omk2 = SQR(pg.Omega0) * ir1 * ir1 * ir1;
  const Real T0 = omk2 * H * H / pg.Gamma;
  return T0 * std::pow(rho / rho0, pg.Gamma - 1.0);
}
inline Real disk_pres(const Sim &s, const Real tf, const Real R, const Real z) {
  const Real df = disk_den(s.disk, R, z);
  return std::max(s.disk.pres_min, std::max(0.0, (s.c.gamma - 1.0) * df * s.cv * tf));
}
inline Real disk_visc(const Sim::DiskParams &pg, const Real R) { return pg.nu0 * std::pow(R / pg.r0, pg.nu_indx); }

struct DiskState {
  Real gdens, gtemp, gv[3], ddens, dv[3];
};
// disk.hpp:141-247 ComputeDiskProfile.  The pressure gradient is restated literally: the two
// `(pfm = pgen.pres_min) ? ...` conditions (:186, :203, :220) ASSIGN pres_min to pfm, so both face
// pressures end up equal to pres_min and pgrad = 0 whenever pres_min != 0 -- the rotation
// profile the reference starts from is exactly Keplerian in R^2+z^2.
inline DiskState disk_profile(const Sim &s, int k, int j, int i) {
  const Sim::DiskParams &pg = s.disk;
  const Coords coords(s, k, j, i);
  const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
  const Frame fr = to_cyl_frame(coords, xv);
  const Real *xcyl = fr.x;
  DiskState o;
  o.gdens = disk_den(pg, xcyl[0], xcyl[2]);
  const Real rt = xcyl[0];
  o.gtemp = disk_temp(pg, rt, xcyl[2]);
  const Real fpts[3][2][3] = {{{coords.bnds.x1[0], xv[1], xv[2]}, {coords.bnds.x1[1], xv[1], xv[2]}},
                              {{xv[0], coords.bnds.x2[0], xv[2]}, {xv[0], coords.bnds.x2[1], xv[2]}},
                              {{xv[0], xv[1], coords.bnds.x3[0]}, {xv[0], xv[1], coords.bnds.x3[1]}}};
  Real widths[3];
  coords.GetCellWidths(widths);
  Real pgrad[3];
  for (int d = 0; d < 3; ++d) {
    Frame xf = to_cyl_frame(coords, fpts[d][0]);
    const Real tfm = disk_temp(pg, xf.x[0], xf.x[2]);
    Real pfm = disk_pres(s, tfm, xf.x[0], xf.x[2]);
    xf = to_cyl_frame(coords, fpts[d][1]);
    const Real tfp = disk_temp(pg, xf.x[0], xf.x[2]);
    const Real pfp = (pfm = pg.pres_min) ? pg.pres_min : disk_pres(s, tfp, xf.x[0], xf.x[2]);
    pfm = (pfp == pg.pres_min) ? pg.pres_min : pfm;
    pgrad[d] = (pfp - pfm) / widths[d];
  }
  const Real eR[3] = {fr.e1[0], fr.e2[0], fr.e3[0]};
  const Real dpdr = pgrad[0] * eR[0] + pgrad[1] * eR[1] + pgrad[2] * eR[2]; // ArtemisUtils::VDot
  const Real r = std::sqrt(SQR(xcyl[0]) + SQR(xcyl[2]));
  const Real omk2 = pg.gm / (r * r * r);
  const Real vk2 = omk2 * SQR(xcyl[0]);
  const Real vp = std::sqrt(vk2 + dpdr * xcyl[0] / o.gdens);
  const Real nu = disk_visc(pg, rt);
  const Real vr = pg.quiet_start ? 0.0 : -1.5 * nu / xcyl[0];
  const Real vcyl[3] = {vr, vp - pg.omf * xcyl[0], 0.0};
  auto vdot = [](const Real a[3], const Real b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  o.gv[0] = vdot(vcyl, fr.e1), o.gv[1] = vdot(vcyl, fr.e2), o.gv[2] = vdot(vcyl, fr.e3);
  o.ddens = pg.dust_to_gas * o.gdens;
  const Real vkep[3] = {0.0, std::sqrt(vk2) - pg.omf * xcyl[0], 0.0};
  o.dv[0] = vdot(vkep, fr.e1), o.dv[1] = vdot(vkep, fr.e2), o.dv[2] = vdot(vkep, fr.e3);
  return o;
}
// disk.hpp:325-354 DiskICImpl
inline void disk_ic_cell(Sim &s, int k, int j, int i) {
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const DiskState o = disk_profile(s, k, j, i);
  const size_t c = IDX(s, k, j, i);
  s.gprim[0 * s.N + c] = o.gdens;
  for (int q = 0; q < 3; ++q) s.gprim[(ng_ + q) * s.N + c] = o.gv[q];
  s.gprim[(5 * ng_) * s.N + c] = s.cv * o.gtemp;
  for (int n = 0; n < nd_; ++n) {
    s.dprim[n * s.N + c] = o.ddens;
    for (int q = 0; q < 3; ++q) s.dprim[(nd_ + 3 * n + q) * s.N + c] = o.dv[q];
  }
}
// disk.hpp:597-632 DiskBoundaryIC and :634-825 DiskBoundaryExtrap on the ghost slab of face
// (d, side), over the entire extent of the other dimensions (parthenon par_for_bndry, upstream).
void disk_bc(Sim &s, int d, int side, bool extrap, bool visc = false) {
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const bool INNER = (side == 0);
  const int lo[3] = {s.is, s.js, s.ks}, hi[3] = {s.ie, s.je, s.ke};
  int b0[3] = {0, 0, 0}, b1[3] = {s.ni - 1, s.nj - 1, s.nk - 1};
  if (INNER) b1[d] = lo[d] - 1;
  else b0[d] = hi[d] + 1;
  const bool lnx = (s.c.coords != CO_CART);
  const Sim::DiskParams &dp = s.disk;
  auto vdot = [](const Real a[3], const Real b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  for (int k = b0[2]; k <= b1[2]; ++k)
    for (int j = b0[1]; j <= b1[1]; ++j)
      for (int i = b0[0]; i <= b1[0]; ++i) {
        if (!extrap) {
          if (s.ic_g.empty() && s.ic_d.empty()) {
            disk_ic_cell(s, k, j, i);
          } else {
            const size_t c0 = IDX(s, k, j, i);
            const int vars[5] = {0, ng_ + 0, ng_ + 1, ng_ + 2, 5 * ng_};
            if (ng_)
              for (int q = 0; q < 5; ++q) s.gprim[vars[q] * s.N + c0] = s.ic_g[vars[q] * s.N + c0];
            for (int v = 0; v < 4 * nd_; ++v) s.dprim[v * s.N + c0] = s.ic_d[v * s.N + c0];
          }
          continue;
        }
        int ia[3] = {i, j, k}, ip1[3] = {i, j, k}, im1[3] = {i, j, k}; // (i, j, k) order here
        ia[d] = INNER ? lo[d] : hi[d];
        ip1[d] = INNER ? lo[d] + 1 : hi[d];
        im1[d] = INNER ? lo[d] : hi[d] - 1;
        const int ix1 = d, ix2 = (d + 1) % 3, ix3 = (d + 2) % 3;
        const Coords coords(s, k, j, i), ca(s, ia[2], ia[1], ia[0]), cp1(s, ip1[2], ip1[1], ip1[0]),
            cm1(s, im1[2], im1[1], im1[0]);
        const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
        const Real xva[3] = {ca.x1v(), ca.x2v(), ca.x3v()};
        const Real xvp1[3] = {cp1.x1v(), cp1.x2v(), cp1.x3v()};
        const Real xvm1[3] = {cm1.x1v(), cm1.x2v(), cm1.x3v()};
        const Frame fr = to_cyl_frame(coords, xv), fa = to_cyl_frame(ca, xva);
        const Frame fp1 = to_cyl_frame(cp1, xvp1), fm1 = to_cyl_frame(cm1, xvm1);
        const Real eRa[3] = {fa.e1[0], fa.e2[0], fa.e3[0]};
        const Real epa[3] = {fa.e1[1], fa.e2[1], fa.e3[1]};
        const Real eza[3] = {fa.e1[2], fa.e2[2], fa.e3[2]};
        const Real epp1[3] = {fp1.e1[1], fp1.e2[1], fp1.e3[1]};
        const Real epm1[3] = {fm1.e1[1], fm1.e2[1], fm1.e3[1]};
        const Real xma = (lnx) ? std::log(xv[ix1] / xva[ix1]) : xv[ix1] - xva[ix1];
        const Real dx = (lnx) ? std::log(xvp1[ix1] / xvm1[ix1]) : xvp1[ix1] - xvm1[ix1];
        const Real xmadx = xma / dx;
        const size_t c = IDX(s, k, j, i), cA = IDX(s, ia[2], ia[1], ia[0]);
        const size_t cP = IDX(s, ip1[2], ip1[1], ip1[0]), cM = IDX(s, im1[2], im1[1], im1[0]);
        const Real *rho = s.gprim.data(), *sie = s.gprim.data() + (5 * ng_) * s.N;
        Real dgvp = 0.0;
        if (ng_) {
          Real dgrho = visc ? 0.0 : std::log(rho[cP] / rho[cM]);
          Real dgsie = std::log(sie[cP] / sie[cM]);
          const Real grhoexp = std::exp(dgrho * xmadx);
          const Real gsieexp = std::exp(dgsie * xmadx);
          Real rhog = rho[cA] * grhoexp;
          const Real sieg = sie[cA] * gsieexp;
          auto vel = [&](int q, size_t cc) { return s.gprim[(ng_ + q) * s.N + cc]; };
          Real gva[3] = {vel(0, cA), vel(1, cA), vel(2, cA)};
          Real gvp1[3] = {vel(0, cP), vel(1, cP), vel(2, cP)};
          Real gvm1[3] = {vel(0, cM), vel(1, cM), vel(2, cM)};
          const Real gvp = vdot(gva, epa) + dp.omf * fa.x[0];
          Real gvR = vdot(gva, eRa);
          const Real gvz = vdot(gva, eza);
          const Real gvp1p = vdot(gvp1, epp1) + dp.omf * fp1.x[0];
          const Real gvm1p = vdot(gvm1, epm1) + dp.omf * fm1.x[0];
          dgvp = std::log(gvp1p / gvm1p);
          if (visc) { // disk.hpp:415-595 DiskBoundaryVisc: steady viscous accretion sets rho and v_R
            const Real nua = disk_visc(dp, fa.x[0]);
            const Real nug = disk_visc(dp, fr.x[0]);
            const Real vpg = gvp * std::exp(dgvp * xmadx);
            const Real rhoa = rho[cA];
            if (INNER) {
              rhog = rhoa * nua / nug;
              gvR = -1.5 * nug / fr.x[0];
            } else { // dFnu/dl = Mdot
              const Real lg = fr.x[0] * vpg;
              const Real la = fa.x[0] * gvp;
              rhog = (3.0 * M_PI * rhoa * nua * la + dp.mdot * (lg - la)) / (3.0 * M_PI * nug * lg);
              gvR = -dp.mdot / (2 * M_PI * fr.x[0] * rhog);
            }
          }
          const Real gvcyl[3] = {gvR, gvp * std::exp(dgvp * xmadx) - dp.omf * fr.x[0], gvz};
          const Real gvel[3] = {vdot(gvcyl, fr.e1), vdot(gvcyl, fr.e2), vdot(gvcyl, fr.e3)};
          s.gprim[0 * s.N + c] = rhog;
          s.gprim[(5 * ng_) * s.N + c] = sieg;
          s.gprim[(ng_ + ix1) * s.N + c] = gvel[ix1];
          s.gprim[(ng_ + ix2) * s.N + c] = gvel[ix2];
          s.gprim[(ng_ + ix3) * s.N + c] = gvel[ix3];
        }
        for (int n = 0; n < nd_; ++n) {
          const Real *dr = s.dprim.data() + n * s.N;
          Real ddrho = std::log(dr[cP] / dr[cM]);
          const Real drhoexp = std::exp(ddrho * xmadx);
          const Real rhod = dr[cA] * drhoexp;
          auto vel = [&](int q, size_t cc) { return s.dprim[(nd_ + 3 * n + q) * s.N + cc]; };
          Real dva[3] = {vel(0, cA), vel(1, cA), vel(2, cA)};
          const Real dvp = vdot(dva, epa) + dp.omf * fa.x[0];
          const Real dvR = vdot(dva, eRa);
          const Real dvz = vdot(dva, eza);
          // the dust azimuthal velocity is scaled with the GAS exponent dgvp (:795-797)
          const Real dvcyl[3] = {dvR, dvp * std::exp(dgvp * xmadx) - dp.omf * fr.x[0], dvz};
          const Real dvel[3] = {vdot(dvcyl, fr.e1), vdot(dvcyl, fr.e2), vdot(dvcyl, fr.e3)};
          s.dprim[n * s.N + c] = rhod;
          s.dprim[(nd_ + 3 * n + ix1) * s.N + c] = dvel[ix1];
          s.dprim[(nd_ + 3 * n + ix2) * s.N + c] = dvel[ix2];
          s.dprim[(nd_ + 3 * n + ix3) * s.N + c] = dvel[ix3];
        }
      }
}
void apply_bcs(Sim &s) {
  for (int pass = 0; pass < 2; ++pass)
    for (int d = 0; d < 3; ++d) {
      if (s.c.ns_gas) fill_dir(s, s.gprim, s.nvg, s.c.ns_gas, true, d, pass);
      if (s.c.ns_dust) fill_dir(s, s.dprim, s.nvd, s.c.ns_dust, false, d, pass);
      if (pass == 1 && d < s.ndim)
        for (int side = 0; side < 2; ++side) {
          const int bc = s.c.bc[2 * d + side];
          if ((d != 1 && bc == BC_STRAT_EXTRAP) || (d == 1 && bc == BC_STRAT_INFLOW))
            strat_bc(s, d, side);
          if (bc == BC_CONDUCTIVE) conductive_bc(s, d, side);
          if (bc == BC_DISK_IC || bc == BC_DISK_EXTRAP) disk_bc(s, d, side, bc == BC_DISK_EXTRAP);
          if (bc == BC_DISK_VISC && d == 0) disk_bc(s, d, side, true, true); // x1 faces only (:448-455)
        }
    }
}

// ---------------------------------------------------------------------------------------
// parthenon LowStorageIntegrator (upstream, recalled): (gam0, gam1, beta) per stage.
int integrator_coeffs(int integ, Real g0[3], Real g1[3], Real be[3]) {
  switch (integ) {
  case INT_RK1:
    g0[0] = 0.0, g1[0] = 1.0, be[0] = 1.0;
    return 1;
  case INT_RK2:
    g0[0] = 0.0, g1[0] = 1.0, be[0] = 1.0;
    g0[1] = 0.5, g1[1] = 0.5, be[1] = 0.5;
    return 2;
  case INT_VL2:
    g0[0] = 0.0, g1[0] = 1.0, be[0] = 0.5;
    g0[1] = 0.0, g1[1] = 1.0, be[1] = 1.0;
    return 2;
  default:
    g0[0] = 0.0, g1[0] = 1.0, be[0] = 1.0;
    g0[1] = 0.25, g1[1] = 0.75, be[1] = 0.25;
    g0[2] = 2.0 / 3.0, g1[2] = 1.0 / 3.0, be[2] = 2.0 / 3.0;
    return 3;
  }
}

// artemis_driver.cpp:145-273 StepTasks for gas/dust with every optional package disabled.
// `after_c2p` (may be null) lets a test inject the inter-rank halo exchange exactly where
// AddBoundaryExchangeTasks sits (:258).
typedef void (*exchange_fn)(void *);
void step(Sim &s, exchange_fn xchg, void *ctx) {
  Real g0[3], g1[3], be[3];
  const int nstages = integrator_coeffs(s.c.integrator, g0, g1, be);
  deep_copy(s); // :157-163
  for (int stage = 1; stage <= nstages; ++stage) {
    const Real bdt = be[stage - 1] * s.dt;                               // :168
    const bool do_pcm = ((stage == 1) && (s.c.integrator == INT_VL2));   // :182
    calculate_fluxes(s, FL_GAS, do_pcm);                                 // :184
    calculate_fluxes(s, FL_DUST, do_pcm);                                // :185
    if (s.visc.type || s.cond.type) {                                    // :189-194
      zero_diffusion_flux(s);
      viscous_flux(s);
      thermal_flux(s);
    }
    apply_update(s, g0[stage - 1], g1[stage - 1], be[stage - 1] * s.dt); // :205-207
    flux_source(s, FL_GAS, bdt);                                         // :211
    flux_source(s, FL_DUST, bdt);                                        // :212
    diffusion_update(s, bdt);                                            // :218-221
    external_gravity(s, s.time, bdt);                                    // :224-228
    rotating_frame_force(s, bdt);                                        // :231-235
    drag_source(s, bdt);                                                 // :238-241
    cooling_source(s, s.time, bdt);                                      // :243-248
    set_aux(s);                                                          // :251-252
    cons_to_prim(s);                                                     // :255
    if (xchg) xchg(ctx);                                                 // :258 (inter-block)
    apply_bcs(s);                                                        // :258 (physical)
    prim_to_cons(s);                                                     // :261
  }
}

Real new_dt(const Sim &s) {
  Real dt = std::numeric_limits<Real>::max();
  if (s.c.ns_gas) dt = std::min(dt, estimate_dt(s, FL_GAS));
  if (s.c.ns_dust) dt = std::min(dt, estimate_dt(s, FL_DUST));
  return dt;
}

} // namespace

// =======================================================================================
extern "C" {

void *oracle_create(const oracle_cfg *cfg) {
  Sim *s = new Sim();
  s->c = *cfg;
  const oracle_cfg &c = s->c;
  s->ndim = (c.nx3 > 1) ? 3 : ((c.nx2 > 1) ? 2 : 1);
  const int g1 = c.ng, g2 = (c.nx2 > 1) ? c.ng : 0, g3 = (c.nx3 > 1) ? c.ng : 0;
  s->ni = c.nx1 + 2 * g1, s->nj = c.nx2 + 2 * g2, s->nk = c.nx3 + 2 * g3;
  s->is = g1, s->ie = g1 + c.nx1 - 1;
  s->js = g2, s->je = g2 + c.nx2 - 1;
  s->ks = g3, s->ke = g3 + c.nx3 - 1;
  s->N = static_cast<size_t>(s->ni) * s->nj * s->nk;
  s->dx[0] = (c.x1max - c.x1min) / c.nx1;
  s->dx[1] = (c.x2max - c.x2min) / c.nx2;
  s->dx[2] = (c.x3max - c.x3min) / c.nx3;
  s->f0[0] = c.x1min - g1 * s->dx[0];
  s->f0[1] = c.x2min - g2 * s->dx[1];
  s->f0[2] = c.x3min - g3 * s->dx[2];
  s->nvg = 6 * c.ns_gas, s->nvd = 4 * c.ns_dust;
  if (c.nthreads > 0) omp_set_num_threads(c.nthreads);
  // zero-fill plane by plane with the static k-decomposition the sweeps use (NUMA first touch)
  auto first_touch = [&](RVec &v, size_t nvar) {
    v.resize(nvar * s->N);
    const size_t plane = static_cast<size_t>(s->ni) * s->nj;
    Real *p = v.data();
    const long nk = s->nk, N = static_cast<long>(s->N);
#pragma omp parallel for schedule(static)
    for (long k = 0; k < nk; ++k)
      for (size_t n = 0; n < nvar; ++n) std::memset(p + n * N + k * plane, 0, plane * sizeof(Real));
  };
  first_touch(s->gprim, s->nvg), first_touch(s->gu0, s->nvg), first_touch(s->gu1, s->nvg);
  first_touch(s->dprim, s->nvd), first_touch(s->du0, s->nvd), first_touch(s->du1, s->nvd);
  for (int d = 0; d < 3; ++d) {
    first_touch(s->gflux[d], s->nvg), first_touch(s->gpflux[d], c.ns_gas), first_touch(s->gvface[d], c.ns_gas);
    first_touch(s->dflux[d], s->nvd);
  }
  for (int d = 0; d < 3; ++d) first_touch(s->qflux[d], static_cast<size_t>(4) * c.ns_gas);
  s->cv = 1.0 / ((c.gamma - 1.) * 1.0 * 1.0);
  s->time = 0.0, s->dt = std::numeric_limits<Real>::max(), s->ncycle = 0;
  s->gx1min = c.x1min, s->gx1max = c.x1max, s->gx2min = c.x2min, s->gx2max = c.x2max;
  s->gx3min = c.x3min, s->gx3max = c.x3max;
  return s;
}
void oracle_destroy(void *h) { delete static_cast<Sim *>(h); }

// Global mesh bounds (the pgens use mesh_size, not the block's bounds).
void oracle_set_mesh_bounds(void *h, double x1min, double x1max, double x2min, double x2max,
                            double x3min, double x3max) {
  Sim &s = *static_cast<Sim *>(h);
  s.gx1min = x1min, s.gx1max = x1max, s.gx2min = x2min, s.gx2max = x2max;
  s.gx3min = x3min, s.gx3max = x3max;
}

void oracle_dims(void *h, int *out) {
  Sim &s = *static_cast<Sim *>(h);
  out[0] = s.ni, out[1] = s.nj, out[2] = s.nk, out[3] = s.is, out[4] = s.ie, out[5] = s.js;
  out[6] = s.je, out[7] = s.ks, out[8] = s.ke, out[9] = s.ndim;
}
// which: 0 gprim 1 gu0 2 gu1 3..5 gflux 6..8 gpflux 9..11 gvface 12 dprim 13 du0 14 du1
// 15..17 dflux
double *oracle_field(void *h, int which) {
  Sim &s = *static_cast<Sim *>(h);
  switch (which) {
  case 0: return s.gprim.data();
  case 1: return s.gu0.data();
  case 2: return s.gu1.data();
  case 3: case 4: case 5: return s.gflux[which - 3].data();
  case 6: case 7: case 8: return s.gpflux[which - 6].data();
  case 9: case 10: case 11: return s.gvface[which - 9].data();
  case 12: return s.dprim.data();
  case 13: return s.du0.data();
  case 14: return s.du1.data();
  case 15: case 16: case 17: return s.dflux[which - 15].data();
  }
  return nullptr;
}

void oracle_calculate_fluxes(void *h, int fluid, int pcm) {
  calculate_fluxes(*static_cast<Sim *>(h), fluid, pcm != 0);
}
void oracle_apply_update(void *h, double gam0, double gam1, double beta_dt) {
  apply_update(*static_cast<Sim *>(h), gam0, gam1, beta_dt);
}
void oracle_flux_source(void *h, int fluid, double dt) {
  flux_source(*static_cast<Sim *>(h), fluid, dt);
}
void oracle_set_aux(void *h) { set_aux(*static_cast<Sim *>(h)); }
void oracle_cons_to_prim(void *h) { cons_to_prim(*static_cast<Sim *>(h)); }
void oracle_prim_to_cons(void *h) { prim_to_cons(*static_cast<Sim *>(h)); }
void oracle_deep_copy(void *h) { deep_copy(*static_cast<Sim *>(h)); }
double oracle_estimate_dt(void *h, int fluid) { return estimate_dt(*static_cast<Sim *>(h), fluid); }
void oracle_apply_bcs(void *h) { apply_bcs(*static_cast<Sim *>(h)); }

double oracle_time(void *h) { return static_cast<Sim *>(h)->time; }
double oracle_dt(void *h) { return static_cast<Sim *>(h)->dt; }
long oracle_ncycle(void *h) { return static_cast<Sim *>(h)->ncycle; }
void oracle_set_dt(void *h, double dt) { static_cast<Sim *>(h)->dt = dt; }

// One step with the current dt; exchange callback optional.
void oracle_step(void *h, void (*xchg)(void *), void *ctx) {
  step(*static_cast<Sim *>(h), xchg, ctx);
}
// parthenon Mesh::Initialize after ProblemGenerator + PostInitialization (upstream, recalled):
// boundaries are communicated once before the first step, i.e. PreCommFillDerived (ConsToPrim,
// artemis.cpp:122) -> exchange + physical BCs -> FillDerived (PrimToCons, artemis.cpp:123).
void oracle_post_init(void *h, void (*xchg)(void *), void *ctx) {
  Sim &s = *static_cast<Sim *>(h);
  cons_to_prim(s);
  if (xchg) xchg(ctx);
  apply_bcs(s);
  prim_to_cons(s);
}
// Local (this block) dt estimate: min over fluids, cfl included.
double oracle_new_dt(void *h) { return new_dt(*static_cast<Sim *>(h)); }

// parthenon EvolutionDriver::Execute / SetGlobalTimeStep (upstream, recalled; pinned by
// advection.py:100-118: dt = 1.11612e-02, cycle = 56):
//   init: dt = estimate;  loop while time < tlim && (nlim < 0 || ncycle < nlim):
//   Step(); time += dt; ncycle++; dt = min(2*dt, estimate); if (time < tlim && tlim-time < dt)
//   dt = tlim - time.
// Single-block driver; returns the number of cycles taken.
long oracle_evolve(void *h, double tlim, long nlim) {
  Sim &s = *static_cast<Sim *>(h);
  if (s.ncycle == 0 && s.time == 0.0) {
    s.dt = new_dt(s);
    if (tlim > 0.0 && s.time < tlim && (tlim - s.time) < s.dt) s.dt = tlim - s.time;
  }
  long n = 0;
  while ((tlim < 0.0 || s.time < tlim) && (nlim < 0 || s.ncycle < nlim)) {
    step(s, nullptr, nullptr);
    s.time += s.dt;
    s.ncycle++;
    n++;
    Real dt = s.dt;
    if (dt < 0.1 * std::numeric_limits<Real>::max()) dt *= 2.0;
    dt = std::min(dt, new_dt(s));
    if (tlim > 0.0 && s.time < tlim && (tlim - s.time) < dt) dt = tlim - s.time;
    s.dt = dt;
  }
  return n;
}

// ---------------------------------------------------------------------------------------
// pgen/blast.hpp:134-228 (gas prim rho, v, sie over the entire block incl. ghosts,
// then PostInitialization = PrimToCons, main.cpp:43).
void oracle_pgen_blast(void *h, double rinit, double internal_energy, double p0, double d0,
                       double x0, double y0, double z0, int samples, int type) {
  Sim &s = *static_cast<Sim *>(h);
  const Real gm1 = s.c.gamma - 1.0;
  const int nsp = s.c.ns_gas;
  for (int k = 0; k < s.nk; ++k)
    for (int j = 0; j < s.nj; ++j)
      for (int i = 0; i < s.ni; ++i) {
        const Coords coords(s, k, j, i);
        const BBox &b = coords.bnds;
        Real total_vol = coords.Volume();
        const Real xv[3] = {coords.x1v(), coords.x2v(), coords.x3v()};
        Real den = d0;
        Real e0 = p0 / gm1;
        Real ie = 0.0;
        Real xcart[3], xc[3];
        const Real x0v[3] = {x0, y0, z0};
        coords.ConvertToCart(xv, xcart); // blast.hpp:181-185
        coords.ConvertToCart(x0v, xc);
        for (int n = 0; n < 3; n++)
          xcart[n] -= xc[n];
        Real vol;
        if (type == 1) { // spherical (blast.hpp:188-201)
          if (samples > 0 && s.c.coords == CO_AXI) {
            // compute_overlap_sph, axisymmetric branch (blast.hpp:107-121)
            const Real dxf = (b.x1[1] - b.x1[0]) / (Real)samples;
            const Real dyf = (b.x2[1] - b.x2[0]) / (Real)samples;
            Real dV = dxf * dyf;
            Real tot = 0.0;
            for (int ii = 0; ii < samples; ii++) {
              const Real xc_ = b.x1[0] + (ii + 0.5) * dxf;
              for (int jj = 0; jj < samples; jj++) {
                const Real yc_ = b.x2[0] + (jj + 0.5) * dyf;
                if (SQR(xc_) + SQR(yc_) <= SQR(rinit)) tot += xc_ * dV;
              }
            }
            vol = tot;
          } else if (samples > 0 && s.c.coords != CO_CART) {
            vol = 0.0; // blast.hpp:122: every other system falls through to `return 0.0`
          } else if (samples > 0) {
            // compute_overlap_sph, Cartesian branch (blast.hpp:91-106): NOT offset by x0
            const Real dxf = (b.x1[1] - b.x1[0]) / (Real)samples;
            const Real dyf = (b.x2[1] - b.x2[0]) / (Real)samples;
            const Real dzf = (b.x3[1] - b.x3[0]) / (Real)samples;
            int tot = 0;
            for (int ii = 0; ii < samples; ii++) {
              const Real xc_ = b.x1[0] + (ii + 0.5) * dxf;
              for (int jj = 0; jj < samples; jj++) {
                const Real yc_ = b.x2[0] + (jj + 0.5) * dyf;
                for (int kk = 0; kk < samples; kk++) {
                  const Real zc_ = b.x3[0] + (kk + 0.5) * dzf;
                  if (SQR(xc_) + SQR(yc_) + SQR(zc_) <= SQR(rinit)) tot++;
                }
              }
            }
            vol = tot * dxf * dyf * dzf;
          } else {
            vol = ((SQR(xcart[0]) + SQR(xcart[1]) + SQR(xcart[2]) < rinit * rinit) ? total_vol
                                                                                   : 0.0);
          }
          ie = e0 * (1.0 - vol / total_vol) +
               internal_energy * vol / total_vol / (4.0 * M_PI / 3.0 * rinit * rinit * rinit);
        } else { // cylindrical (blast.hpp:202-213)
          if (samples > 0 && s.c.coords != CO_CART) {
            vol = 0.0; // compute_overlap_cyl has a Cartesian branch only (blast.hpp:68-81)
          } else if (samples > 0) {
            // compute_overlap_cyl (blast.hpp:65-80)
            const Real dxf = (b.x1[1] - b.x1[0]) / (Real)samples;
            const Real dyf = (b.x2[1] - b.x2[0]) / (Real)samples;
            int tot = 0;
            for (int ii = 0; ii < samples; ii++) {
              const Real xc_ = b.x1[0] + ((Real)ii + 0.5) * dxf;
              for (int jj = 0; jj < samples; jj++) {
                const Real yc_ = b.x2[0] + ((Real)jj + 0.5) * dyf;
                if (SQR(xc_) + SQR(yc_) <= SQR(rinit)) tot++;
              }
            }
            vol = tot * dxf * dyf;
          } else {
            vol = ((SQR(xcart[0]) + SQR(xcart[1]) + SQR(xcart[2]) < rinit * rinit) ? total_vol
                                                                                   : 0.0);
          }
          ie = e0 * (1.0 - vol / total_vol) +
               internal_energy * vol / total_vol / (M_PI * rinit * rinit);
        }
        const size_t c = IDX(s, k, j, i);
        s.gprim[0 * s.N + c] = den;
        s.gprim[(nsp + 0) * s.N + c] = 0.0;
        s.gprim[(nsp + 1) * s.N + c] = 0.0;
        s.gprim[(nsp + 2) * s.N + c] = 0.0;
        s.gprim[(5 * nsp) * s.N + c] = ie / den;
      }
  prim_to_cons(s);
}

// Source-package parameters (gravity.cpp:25-118, rotating_frame.cpp:24-50, drag.cpp:25-84,
// dust.cpp:102-176 sizes / grain_density).  G = 1 in scale-free units (units.cpp:68-76).
void oracle_set_gravity_uniform(void *h, double gx1, double gx2, double gx3) {
  Sim &s = *static_cast<Sim *>(h);
  s.grav.type = 1, s.grav.g[0] = gx1, s.grav.g[1] = gx2, s.grav.g[2] = gx3;
}
void oracle_set_gravity_point(void *h, double mass, double soft, double sink, double sink_rate,
                              double x, double y, double z) {
  Sim &s = *static_cast<Sim *>(h);
  s.grav.type = 2, s.grav.gm = 1.0 * mass, s.grav.soft = soft, s.grav.sink = sink;
  s.grav.sink_rate = sink_rate, s.grav.pos[0] = x, s.grav.pos[1] = y, s.grav.pos[2] = z;
}
// <gravity/binary> (gravity.cpp:77-111); angles in radians (the deck's degrees * M_PI / 180.)
// p = {mass, q, a, e, i, omega, Omega, f, soft1, soft2, sink1, sink2, sink_rate1, sink_rate2, x, y, z}
void oracle_set_gravity_binary(void *h, const double *p) {
  Sim &s = *static_cast<Sim *>(h);
  auto &g = s.grav;
  g.type = 3, g.gm = 1.0 * p[0], g.q = p[1], g.a = p[2], g.e = p[3];
  g.n = std::sqrt(g.gm / (g.a * g.a * g.a));
  g.coso = std::cos(p[5]), g.sino = std::sin(p[5]);
  g.cosI = std::cos(p[4]), g.sinI = std::sin(p[4]);
  g.cosO = std::cos(p[6]), g.sinO = std::sin(p[6]);
  g.cosf0 = std::cos(p[7]), g.sinf0 = std::sin(p[7]);
  g.soft = p[8], g.soft2 = p[9], g.sink = p[10], g.sink2 = p[11], g.sink_rate = p[12], g.sink_rate2 = p[13];
  g.pos[0] = p[14], g.pos[1] = p[15], g.pos[2] = p[16];
}
// <gravity/nbody> with the nbody package's particles: par[20 * n + ...] = {GM, pos[3], vel[3], xf[3], vf[3], rs, racc,
// gamma, beta, spline, couple, 0}
void oracle_set_gravity_nbody(void *h, int npart, const double *par, int frame_correction) {
  Sim &s = *static_cast<Sim *>(h);
  s.grav.type = 4;
  s.nbody.assign(npart, Sim::NBodyParticle());
  double gm = 0.0;
  for (int n = 0; n < npart; ++n) {
    const double *q = par + 20 * n;
    Sim::NBodyParticle &p = s.nbody[n];
    p.GM = q[0];
    for (int d = 0; d < 3; ++d) p.pos[d] = q[1 + d], p.vel[d] = q[4 + d], p.xf[d] = q[7 + d], p.vf[d] = q[10 + d];
    p.rs = q[13], p.racc = q[14], p.gamma = q[15], p.beta = q[16];
    p.spline = static_cast<int>(q[17]), p.couple = static_cast<int>(q[18]);
    gm += p.GM;
  }
  s.grav.gm = gm; // gravity.cpp:117: gm of the nbody package = G * mtot
  s.nbody_frame_correction = frame_correction != 0;
  s.pforce.assign(static_cast<size_t>(7) * npart, 0.0);
}
// gm of the gravity package when it is not the plain sum of the particles' GM: nbody.cpp:109 registers G * mtot with mtot
// = <nbody> mtot or the sum of the deck's masses BEFORE the rescale of nbody_setup.cpp:707 (which can move the sum by an ulp)
void oracle_set_gravity_gm(void *h, double gm) { static_cast<Sim *>(h)->grav.gm = gm; }
// the accumulated particle_force rows (nbody_gravity.hpp:210-212); `reset` zeroes them like NBody::Advance does
void oracle_nbody_force(void *h, double *out, int reset) {
  Sim &s = *static_cast<Sim *>(h);
  for (size_t q = 0; q < s.pforce.size(); ++q) out[q] = s.pforce[q];
  if (reset) std::fill(s.pforce.begin(), s.pforce.end(), 0.0);
}
void oracle_set_gravity_window(void *h, double tstart, double tstop) {
  Sim &s = *static_cast<Sim *>(h);
  s.grav.tstart = tstart, s.grav.tstop = tstop;
}
// ---------------------------------------------------------------------------------------
// utils/refinement/restriction.hpp:42-114 RestrictAverage<GEOM> and prolongation.hpp:39-184
// ProlongateSharedMinMod<GEOM> for cell-centred fields, between the gas primitives of a fine Sim and
// a coarse Sim (the operators only; the mesh-refinement framework around them is out of scope).
// r = {cis, cie, cjs, cje, cks, cke,  cib, cjb, ckb,  fib, fjb, fkb}: coarse cells processed and the
// coarse <-> fine origin (the reference's cib.s <-> ib.s).  SIGN(a) = (a < 0) ? -1 : 1 (parthenon
// defs.hpp, upstream, recalled).  Parity unpinned: no reference test isolates these operators.
// `field` selects the cell-centred arrays the operator acts on (the reference registers the same operators for every
// field, utils/artemis_utils.cpp:92-112): 0 gas primitives, 1 gas conserved u0, 2 dust primitives, 3 dust conserved u0
static RVec &refine_field(Sim &s, int field, int *nvar) {
  *nvar = (field < 2) ? s.nvg : s.nvd;
  return field == 0 ? s.gprim : (field == 1 ? s.gu0 : (field == 2 ? s.dprim : s.du0));
}
void oracle_restrict_average_field(void *hf, void *hc, const int *r, int field);
void oracle_restrict_average(void *hf, void *hc, const int *r) { oracle_restrict_average_field(hf, hc, r, 0); }
void oracle_restrict_average_field(void *hf, void *hc, const int *r, int field) {
  Sim &f = *static_cast<Sim *>(hf), &c = *static_cast<Sim *>(hc);
  const int DIM = f.ndim;
  const bool X1 = DIM > 0, X2 = DIM > 1, X3 = DIM > 2;
  int nvar = 0;
  RVec &fq = refine_field(f, field, &nvar), &cq = refine_field(c, field, &nvar);
  for (int v = 0; v < nvar; ++v)
    for (int ck = r[4]; ck <= r[5]; ++ck)
      for (int cj = r[2]; cj <= r[3]; ++cj)
        for (int ci = r[0]; ci <= r[1]; ++ci) {
          const int i = X1 ? (ci - r[6]) * 2 + r[9] : r[9];
          const int j = X2 ? (cj - r[7]) * 2 + r[10] : r[10];
          const int k = X3 ? (ck - r[8]) * 2 + r[11] : r[11];
          Real vol[2][2][2], terms[2][2][2];
          for (int ok = 0; ok < 2; ++ok)
            for (int oj = 0; oj < 2; ++oj)
              for (int oi = 0; oi < 2; ++oi) vol[ok][oj][oi] = terms[ok][oj][oi] = 0;
          for (int ok = 0; ok < 1 + X3; ++ok)
            for (int oj = 0; oj < 1 + X2; ++oj)
              for (int oi = 0; oi < 1 + X1; ++oi) {
                vol[ok][oj][oi] = Coords(f, k + ok, j + oj, i + oi).Volume();
                terms[ok][oj][oi] = vol[ok][oj][oi] * fq[v * f.N + IDX(f, k + ok, j + oj, i + oi)];
              }
          const Real tvol = ((vol[0][0][0] + vol[0][1][0]) + (vol[0][0][1] + vol[0][1][1])) +
                            ((vol[1][0][0] + vol[1][1][0]) + (vol[1][0][1] + vol[1][1][1]));
          cq[v * c.N + IDX(c, ck, cj, ci)] =
              (((terms[0][0][0] + terms[0][1][0]) + (terms[0][0][1] + terms[0][1][1])) +
               ((terms[1][0][0] + terms[1][1][0]) + (terms[1][0][1] + terms[1][1][1]))) /
              tvol;
        }
}
// Refinement criteria (utils/refinement/amr_criteria.hpp:28-168) on component `var` of the gas primitives
// (or, var < 0, on the stored gas pressure of species 0): the block maximum and the AmrTag (-1 derefine, 0 same,
// +1 refine).  Parity unpinned: no reference test isolates the criteria.
int oracle_amr_first_derivative(void *h, int var, double thr, double *maxeps_out) {
  Sim &s = *static_cast<Sim *>(h);
  // FIELD = gas::prim::pressure reads the STORED pressure of species 0 (amr_criteria.hpp:45-46: a pack of FIELD),
  // pack slot 4 ns_gas -- what FillDerived left there (fill_derived.cpp:246-262), ghost zones included
  const Real *q = s.gprim.data() + (var < 0 ? 4 * s.c.ns_gas : var) * s.N;
  *maxeps_out = 0.0;
  if (s.ndim == 1) return 0; // :122-124
  const bool X3 = s.ndim == 3;
  Real maxeps = 0.0;
  for (int k = X3 ? s.ks - 1 : s.ks; k <= (X3 ? s.ke + 1 : s.ks); ++k)
    for (int j = s.js - 1; j <= s.je + 1; ++j)
      for (int i = s.is - 1; i <= s.ie + 1; ++i) {
        const Real sdx1 = Coords(s, k, j, i + 1).x1v() - Coords(s, k, j, i - 1).x1v();
        const Real sdx2 = Coords(s, k, j + 1, i).x2v() - Coords(s, k, j - 1, i).x2v();
        Coords co(s, k, j, i);
        Real hx[3];
        co.GetScaleFactors(hx); // 2-D: hx1(cc), hx2(cc) at the centre = the same values (:104-105)
        Real eps;
        if (X3) {
          const Real sdx3 = Coords(s, k + 1, j, i).x3v() - Coords(s, k - 1, j, i).x3v();
          eps = std::sqrt(SQR((q[IDX(s, k, j, i + 1)] - q[IDX(s, k, j, i - 1)]) / sdx1 / hx[0]) +
                          SQR((q[IDX(s, k, j + 1, i)] - q[IDX(s, k, j - 1, i)]) / sdx2 / hx[1]) +
                          SQR((q[IDX(s, k + 1, j, i)] - q[IDX(s, k - 1, j, i)]) / sdx3 / hx[2]));
          eps /= (q[IDX(s, k, j, i)] / std::sqrt(SQR(sdx1 * hx[0]) + SQR(sdx2 * hx[1]) + SQR(sdx3 * hx[2])));
        } else {
          eps = std::sqrt(SQR((q[IDX(s, k, j, i + 1)] - q[IDX(s, k, j, i - 1)]) / sdx1 / hx[0]) +
                          SQR((q[IDX(s, k, j + 1, i)] - q[IDX(s, k, j - 1, i)]) / sdx2 / hx[1]));
          eps /= (q[IDX(s, k, j, i)] / std::sqrt(SQR(sdx1 * hx[0]) + SQR(sdx2 * hx[1])));
        }
        maxeps = std::max(maxeps, eps);
      }
  *maxeps_out = maxeps;
  if (maxeps > thr) return 1;
  if (maxeps < 0.25 * thr) return -1;
  return 0;
}
int oracle_amr_magnitude(void *h, int var, double refine_above, double deref_below, double *max_out) {
  Sim &s = *static_cast<Sim *>(h);
  Real maxvv = 0.0;
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const long n = IDX(s, k, j, i);
        const Real q = var < 0 ? s.gprim[(4 * s.c.ns_gas) * s.N + n] : s.gprim[var * s.N + n];
        maxvv = std::max(maxvv, q);
      }
  *max_out = maxvv;
  if (maxvv > refine_above) return 1;
  if (maxvv < deref_below) return -1;
  return 0;
}
void oracle_prolongate_minmod_field(void *hf, void *hc, const int *r, int field);
void oracle_prolongate_minmod(void *hf, void *hc, const int *r) { oracle_prolongate_minmod_field(hf, hc, r, 0); }
void oracle_prolongate_minmod_field(void *hf, void *hc, const int *r, int field) {
  Sim &f = *static_cast<Sim *>(hf), &c = *static_cast<Sim *>(hc);
  const int DIM = f.ndim;
  const bool X1 = DIM > 0, X2 = DIM > 1, X3 = DIM > 2;
  int nvar = 0;
  RVec &fq = refine_field(f, field, &nvar), &cq = refine_field(c, field, &nvar);
  auto sign = [](Real a) { return (a < 0.) ? -1. : 1.; };
  auto centre = [](const Coords &co, int d) { return d == 1 ? co.x1v() : (d == 2 ? co.x2v() : co.x3v()); };
  for (int v = 0; v < nvar; ++v)
    for (int k = r[4]; k <= r[5]; ++k)
      for (int j = r[2]; j <= r[3]; ++j)
        for (int i = r[0]; i <= r[1]; ++i) {
          const int fi = X1 ? (i - r[6]) * 2 + r[9] : r[9];
          const int fj = X2 ? (j - r[7]) * 2 + r[10] : r[10];
          const int fk = X3 ? (k - r[8]) * 2 + r[11] : r[11];
          const Real *q = cq.data() + v * c.N;
          const Real fc = q[IDX(c, k, j, i)];
          Real dxfm[3] = {0, 0, 0}, dxfp[3] = {0, 0, 0}, g[3] = {0, 0, 0};
          for (int d = 1; d <= DIM; ++d) { // GetGridSpacings<GEOM, d> + GradMinMod
            const int dk = (d == 3), dj = (d == 2), di = (d == 1);
            const Real xm = centre(Coords(c, k - dk, j - dj, i - di), d), xc = centre(Coords(c, k, j, i), d);
            const Real xp = centre(Coords(c, k + dk, j + dj, i + di), d);
            const Real fxm = centre(Coords(f, fk, fj, fi), d), fxp = centre(Coords(f, fk + dk, fj + dj, fi + di), d);
            const Real dxm = xc - xm, dxp = xp - xc;
            dxfm[d - 1] = xc - fxm, dxfp[d - 1] = fxp - xc;
            const Real gxm = (fc - q[IDX(c, k - dk, j - dj, i - di)]) / dxm;
            const Real gxp = (q[IDX(c, k + dk, j + dj, i + di)] - fc) / dxp;
            g[d - 1] = 0.5 * (sign(gxm) + sign(gxp)) * std::min(std::abs(gxm), std::abs(gxp));
          }
          const Real gx1m = g[0], gx1p = g[0], gx2m = g[1], gx2p = g[1], gx3m = g[2], gx3p = g[2];
          const Real dx1fm = dxfm[0], dx1fp = dxfp[0], dx2fm = dxfm[1], dx2fp = dxfp[1], dx3fm = dxfm[2], dx3fp = dxfp[2];
          Real *o = fq.data() + v * f.N;
          o[IDX(f, fk, fj, fi)] = fc - (gx1m * dx1fm + gx2m * dx2fm + gx3m * dx3fm);
          if (X1) o[IDX(f, fk, fj, fi + 1)] = fc + (gx1p * dx1fp - gx2m * dx2fm - gx3m * dx3fm);
          if (X2) o[IDX(f, fk, fj + 1, fi)] = fc - (gx1m * dx1fm - gx2p * dx2fp + gx3m * dx3fm);
          if (X2 && X1) o[IDX(f, fk, fj + 1, fi + 1)] = fc + (gx1p * dx1fp + gx2p * dx2fp - gx3m * dx3fm);
          if (X3) o[IDX(f, fk + 1, fj, fi)] = fc - (gx1m * dx1fm + gx2m * dx2fm - gx3p * dx3fp);
          if (X3 && X1) o[IDX(f, fk + 1, fj, fi + 1)] = fc + (gx1p * dx1fp - gx2m * dx2fm + gx3p * dx3fp);
          if (X3 && X2) o[IDX(f, fk + 1, fj + 1, fi)] = fc - (gx1m * dx1fm - gx2p * dx2fp - gx3p * dx3fp);
          if (X3 && X2 && X1) o[IDX(f, fk + 1, fj + 1, fi + 1)] = fc + (gx1p * dx1fp + gx2p * dx2fp + gx3p * dx3fp);
        }
}

// Lower-face areas Coords<GEOM>::GetFaceArea<dir> (and cell volumes, dir = 0) of every cell of the block,
// for the multilevel oracle's flux correction (RestrictAverage with el = F1/F2/F3, restriction.hpp:88-94).
void oracle_face_areas(void *h, int dir, double *out) {
  Sim &s = *static_cast<Sim *>(h);
  for (int k = 0; k < s.nk; ++k)
    for (int j = 0; j < s.nj; ++j)
      for (int i = 0; i < s.ni; ++i) {
        Coords co(s, k, j, i);
        Real a[2] = {0, 0};
        if (dir == 1) co.GetFaceAreaX1(a);
        else if (dir == 2) co.GetFaceAreaX2(a);
        else if (dir == 3) co.GetFaceAreaX3(a);
        else a[0] = co.Volume();
        out[IDX(s, k, j, i)] = a[0];
      }
}

// <cooling> type = beta, tref = powerlaw (cooling.cpp:34-63)
void oracle_set_cooling(void *h, const double *p) {
  Sim &s = *static_cast<Sim *>(h);
  s.cool.on = true;
  s.cool.beta0 = p[0], s.cool.beta_min = p[1], s.cool.escale = p[2], s.cool.tfloor = p[3];
  s.cool.tcyl = p[4], s.cool.cyl_plaw = p[5], s.cool.tsph = p[6], s.cool.sph_plaw = p[7];
}
void oracle_cooling_source(void *h, double time, double dt) { cooling_source(*static_cast<Sim *>(h), time, dt); }
void oracle_set_rotating_frame(void *h, double omega, double qshear) {
  Sim &s = *static_cast<Sim *>(h);
  s.rframe.on = true, s.rframe.omega = omega, s.rframe.qshear = qshear;
  s.strat.q = qshear, s.strat.Om0 = omega; // strat.hpp:60-61
}
// type: 1 simple_dust, 2 self; model: 0 constant (tau[n] *= scale, drag.hpp:129-137), 1 stokes
void oracle_set_drag(void *h, int type, int model, double scale, double grain_density,
                     const double *tau, const double *sizes) {
  Sim &s = *static_cast<Sim *>(h);
  s.drag.type = type, s.drag.model = model, s.drag.scale = scale;
  s.drag.grain_density = grain_density;
  s.drag.tau.assign(s.c.ns_dust, 0.0), s.drag.sizes.assign(s.c.ns_dust, 0.0);
  for (int n = 0; n < s.c.ns_dust; ++n) {
    s.drag.tau[n] = (model == 0) ? scale * tau[n] : scale;
    if (sizes) s.drag.sizes[n] = sizes[n];
  }
}
// fluid 0 gas / 1 dust; p = {inner_x1..3, inner_x1..3_rate, outer_x1..3, outer_x1..3_rate}
void oracle_set_damping(void *h, int fluid, const double *p) {
  Sim &s = *static_cast<Sim *>(h);
  Sim::SelfDrag &d = fluid ? s.drag.dust : s.drag.gas;
  for (int i = 0; i < 3; ++i)
    d.ix[i] = p[i], d.irate[i] = p[3 + i], d.ox[i] = p[6 + i], d.orate[i] = p[9 + i];
}
// <gas/damping> damp_to_visc (drag.hpp:101): needs viscosity_plaw or viscosity_alpha (drag.cpp:113-121)
int oracle_set_damp_to_visc(void *h, int on) {
  Sim &s = *static_cast<Sim *>(h);
  if (on && s.visc.type != 1 && s.visc.type != 2) return 1; // "The chosen viscosity model does not work with damping"
  s.drag.damp_to_visc = on != 0;
  return 0;
}
void oracle_external_gravity(void *h, double time, double dt) {
  external_gravity(*static_cast<Sim *>(h), time, dt);
}
void oracle_rotating_frame_force(void *h, double dt) { rotating_frame_force(*static_cast<Sim *>(h), dt); }
void oracle_drag_source(void *h, double dt) { drag_source(*static_cast<Sim *>(h), dt); }

// <gas/viscosity> / <gas/conductivity> (diffusion_coeff.hpp:84-136).  which: 0 viscosity, 1 conductivity;
// type: 1 viscosity_plaw (constant|powerlaw), 2 viscosity_alpha, 3 conductivity_plaw, 4 thermaldiff_plaw;
// p = {nu|alpha|cond|kappa, eta_bulk, r_exp, r0, Omega0, temp_exp, rho_exp, rho_ref, T_ref}
void oracle_set_diffusion(void *h, int which, int type, int avg, const double *p) {
  Sim &s = *static_cast<Sim *>(h);
  Sim::DiffCoeff &d = which ? s.cond : s.visc;
  d.type = type, d.avg = avg;
  d.nu_s = d.alpha = d.hcond_0 = d.kappa_0 = p[0];
  d.eta = p[1], d.r_exp = p[2], d.R0 = p[3], d.Omega0 = p[4];
  d.temp_exp = p[5], d.rho_exp = p[6], d.d0 = p[7], d.T0 = p[8];
}
void oracle_zero_diffusion_flux(void *h) { zero_diffusion_flux(*static_cast<Sim *>(h)); }
void oracle_viscous_flux(void *h) { viscous_flux(*static_cast<Sim *>(h)); }
void oracle_thermal_flux(void *h) { thermal_flux(*static_cast<Sim *>(h)); }
void oracle_diffusion_update(void *h, double dt) { diffusion_update(*static_cast<Sim *>(h), dt); }
double *oracle_qflux(void *h, int d) { return static_cast<Sim *>(h)->qflux[d].data(); }

// pgen/conduction.hpp:58-104: isothermal hydrostatic column under uniform gravity gx1 (mass at
// rest unless gas_vx* say otherwise); P = Gamma rho Cv T for the IdealGas (singularity-eos, recalled).
void oracle_pgen_conduction(void *h, double g_rho, double g_vx1, double g_vx2, double g_vx3,
                            double g_temp, double flux) {
  Sim &s = *static_cast<Sim *>(h);
  const int nsp = s.c.ns_gas;
  s.condbc.g_temp = g_temp, s.condbc.flux = flux;
  const Real gx1 = (s.grav.type == 1) ? s.grav.g[0] : 0.0;
  const Real x1min = s.gx1min;
  const Real gm1 = s.c.gamma - 1.0;
  for (int k = 0; k < s.nk; ++k)
    for (int j = 0; j < s.nj; ++j)
      for (int i = 0; i < s.ni; ++i) {
        const Coords coords(s, k, j, i);
        const Real xv0 = coords.x1v();
        const Real P0 = std::max(0.0, gm1 * g_rho * s.cv * g_temp);
        const Real Rgas = P0 / (g_rho * g_temp);
        const Real P = P0 * std::exp(gx1 * g_rho / P0 * (xv0 - x1min));
        const Real dens = P / (Rgas * g_temp);
        const size_t c = IDX(s, k, j, i);
        s.gprim[0 * s.N + c] = dens;
        s.gprim[(nsp + 0) * s.N + c] = g_vx1;
        s.gprim[(nsp + 1) * s.N + c] = g_vx2;
        s.gprim[(nsp + 2) * s.N + c] = g_vx3;
        s.gprim[(5 * nsp) * s.N + c] = std::max(0.0, s.cv * g_temp);
      }
  prim_to_cons(s);
}

// pgen/gaussian_bump.hpp:46-196 with problem/system = cartesian on a Cartesian mesh
void oracle_pgen_gaussian_bump(void *h, const double *xc_bump, double sigma, double dfac, double tfac,
                               double ufac, double vfac, double wfac, double g_rho, double g_vx1,
                               double g_vx2, double g_vx3, double g_pres) {
  Sim &s = *static_cast<Sim *>(h);
  const int nsp = s.c.ns_gas;
  const bool multi_d = (s.ndim >= 2), three_d = (s.ndim == 3);
  const Real gamma = s.c.gamma;
  const Real ex1[3] = {1.0, 0.0, 0.0}, ex2[3] = {0.0, 1.0, 0.0}, ex3[3] = {0.0, 0.0, 1.0};
  for (int k = 0; k < s.nk; ++k)
    for (int j = 0; j < s.nj; ++j)
      for (int i = 0; i < s.ni; ++i) {
        const BBox b = bbox(s, k, j, i);
        const Real xc[3] = {x1v(b), x2v(b), x3v(b)};
        const Real dx2 = SQR(xc[0] - xc_bump[0]) + SQR(xc[1] - xc_bump[1]) * multi_d +
                         SQR(xc[2] - xc_bump[2]) * three_d;
        const Real bump = std::exp(-dx2 / (2.0 * SQR(sigma)));
        const size_t c = IDX(s, k, j, i);
        const Real vx1 = (g_vx1 * ex1[0] + g_vx2 * ex1[1] + g_vx3 * ex1[2]);
        const Real vx2 = (g_vx1 * ex2[0] + g_vx2 * ex2[1] + g_vx3 * ex2[2]);
        const Real vx3 = (g_vx1 * ex3[0] + g_vx2 * ex3[1] + g_vx3 * ex3[2]);
        s.gprim[(nsp + 0) * s.N + c] = vx1 + ufac * bump;
        s.gprim[(nsp + 1) * s.N + c] = vx2 + vfac * bump;
        s.gprim[(nsp + 2) * s.N + c] = vx3 + wfac * bump;
        if (tfac > 0.0) {
          const Real sie0 = g_pres / (g_rho * (gamma - 1.0));
          const Real sie = sie0 * (1. + tfac * bump);
          s.gprim[0 * s.N + c] = g_pres / (sie * (gamma - 1.0));
          s.gprim[(5 * nsp) * s.N + c] = sie;
        } else {
          const Real dens = g_rho * (1. + dfac * bump);
          s.gprim[0 * s.N + c] = dens;
          s.gprim[(5 * nsp) * s.N + c] = g_pres / ((gamma - 1.0) * dens);
        }
      }
  prim_to_cons(s);
}

// pgen/constant.hpp:58-166 with problem/system = cartesian on a Cartesian mesh (the basis
// conversion is the identity); sie = Cv*T with Cv = kB/((gamma-1) amu mu) = 1/(gamma-1) in
// scale-free units (gas.cpp:106-116, units.cpp:68-76; singularity-eos IdealGas, recalled).
void oracle_pgen_constant(void *h, double g_rho, double g_vx1, double g_vx2, double g_vx3,
                          double g_temp, double d_rho, double d_vx1, double d_vx2, double d_vx3) {
  Sim &s = *static_cast<Sim *>(h);
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const Real cv = 1.0 / ((s.c.gamma - 1.) * 1.0 * 1.0);
  const Real ex1[3] = {1.0, 0.0, 0.0}, ex2[3] = {0.0, 1.0, 0.0}, ex3[3] = {0.0, 0.0, 1.0};
  for (size_t c = 0; c < s.N; ++c) {
    if (ng_) {
      s.gprim[0 * s.N + c] = g_rho;
      s.gprim[(ng_ + 0) * s.N + c] = (g_vx1 * ex1[0] + g_vx2 * ex1[1] + g_vx3 * ex1[2]);
      s.gprim[(ng_ + 1) * s.N + c] = (g_vx1 * ex2[0] + g_vx2 * ex2[1] + g_vx3 * ex2[2]);
      s.gprim[(ng_ + 2) * s.N + c] = (g_vx1 * ex3[0] + g_vx2 * ex3[1] + g_vx3 * ex3[2]);
      s.gprim[(5 * ng_) * s.N + c] = std::max(0.0, cv * g_temp);
    }
    for (int n = 0; n < nd_; ++n) {
      s.dprim[n * s.N + c] = d_rho;
      s.dprim[(nd_ + 3 * n + 0) * s.N + c] = (d_vx1 * ex1[0] + d_vx2 * ex1[1] + d_vx3 * ex1[2]);
      s.dprim[(nd_ + 3 * n + 1) * s.N + c] = (d_vx1 * ex2[0] + d_vx2 * ex2[1] + d_vx3 * ex2[2]);
      s.dprim[(nd_ + 3 * n + 2) * s.N + c] = (d_vx1 * ex3[0] + d_vx2 * ex3[1] + d_vx3 * ex3[2]);
    }
  }
  prim_to_cons(s);
}

// pgen/disk.hpp:253-323 InitDiskParams + :356-413 ProblemGenerator.  par = {r0, rho0, dslope,
// h0, polytropic_index, dens_min, pres_min, rexp, rcav, l0, dust_to_gas, temp_soft, tslope,
// flare, quiet_start, mdot (< 0: not given)}; tslope / flare: exactly one is > -1e300.
// Gravity (gm), the rotating frame (omf) and the viscosity must have been set before.
int oracle_pgen_disk(void *h, const double *par) {
  Sim &s = *static_cast<Sim *>(h);
  Sim::DiskParams &d = s.disk;
  d.gm = s.grav.gm;
  d.r0 = par[0];
  d.Omega0 = std::sqrt(d.gm / (d.r0 * d.r0 * d.r0));
  d.rho0 = par[1], d.p = par[2], d.h0 = par[3];
  d.gamma_gas = s.c.gamma;
  d.Gamma = par[4];
  if (!(d.Gamma >= 1)) return 1;
  d.dens_min = par[5], d.pres_min = par[6], d.rexp = par[7], d.rcav = par[8], d.l0 = par[9];
  d.dust_to_gas = par[10], d.temp_soft2 = par[11];
  Real q = par[12], flare = par[13];
  const Real big = -1e300;
  if (!(flare > big) && !(q > big)) return 2;
  if (!(flare > big)) flare = 0.5 * (1.0 + q);
  else if (!(q > big)) q = 2.0 * flare - 1.;
  else return 3;
  d.flare = flare, d.q = q;
  d.alpha = 0.0, d.nu0 = 0.0, d.nu_indx = 0.0, d.mdot = 0.0;
  d.quiet_start = (par[14] != 0.0);
  d.omf = s.rframe.on ? s.rframe.omega : 0.0;
  if (s.visc.type != 0) {
    if (s.visc.type == 2) {
      d.alpha = s.visc.alpha;
      d.nu0 = d.alpha * d.gamma_gas * SQR(d.h0 * d.r0 * d.Omega0);
      d.nu_indx = 1.5 + d.q;
    } else {
      d.nu0 = s.visc.nu_s;
      d.nu_indx = s.visc.r_exp;
    }
    if (par[15] >= 0.0) {
      d.mdot = par[15];
      d.rho0 = d.mdot / (3.0 * M_PI * d.nu0);
    } else {
      d.mdot = 3.0 * M_PI * d.nu0 * d.rho0;
    }
  }
  for (int k = 0; k < s.nk; ++k)
    for (int j = 0; j < s.nj; ++j)
      for (int i = 0; i < s.ni; ++i) disk_ic_cell(s, k, j, i);
  prim_to_cons(s);
  return 0;
}

// pgen/strat.hpp:55-150: isothermal shearing sheet, v2 = -q Om0 x, T0 = (h Om0)^2, Gaussian
// vertical profile in 3-D; dust at dust_to_gas of the gas density with the gas velocity.
void oracle_pgen_strat(void *h, double rho0, double dens_min, double hscale, double d2g) {
  Sim &s = *static_cast<Sim *>(h);
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const bool three_d = (s.ndim == 3);
  const Real q = s.strat.q, Om0 = s.strat.Om0;
  const Real temp0 = SQR(hscale * Om0);
  const Real cv = 1.0 / ((s.c.gamma - 1.) * 1.0 * 1.0);
  for (int k = 0; k < s.nk; ++k)
    for (int j = 0; j < s.nj; ++j)
      for (int i = 0; i < s.ni; ++i) {
        const BBox b = bbox(s, k, j, i);
        const Real x = x1v(b);
        const Real z = x3v(b);
        const Real vx1 = 0.0;
        const Real vx2 = -q * Om0 * x;
        const Real vx3 = 0.0;
        const Real temp = temp0;
        const Real efac = (three_d) ? std::exp(-SQR(z) / (2.0 * SQR(hscale))) : 1.0;
        const Real dens = std::max(dens_min, efac * rho0);
        const Real sie = std::max(0.0, cv * temp);
        const size_t c = IDX(s, k, j, i);
        s.gprim[0 * s.N + c] = dens;
        s.gprim[(ng_ + 0) * s.N + c] = vx1;
        s.gprim[(ng_ + 1) * s.N + c] = vx2;
        s.gprim[(ng_ + 2) * s.N + c] = vx3;
        s.gprim[(5 * ng_) * s.N + c] = sie;
        const Real ddens = dens * d2g;
        for (int n = 0; n < nd_; ++n) {
          s.dprim[n * s.N + c] = ddens;
          s.dprim[(nd_ + 3 * n + 0) * s.N + c] = vx1;
          s.dprim[(nd_ + 3 * n + 1) * s.N + c] = vx2;
          s.dprim[(nd_ + 3 * n + 2) * s.N + c] = vx3;
        }
      }
  prim_to_cons(s);
}

// pgen/linear_wave.hpp:58-111 HydroEigensystem + :117-259 ProblemGenerator.  Returns tlim.
static void lw_setup(Sim &s, int wave_flag, double amp, double vflow, int along_x1, int along_x2,
                     int along_x3, bool eigen) {
  const bool multi_d = (s.ndim > 1), three_d = (s.ndim > 2);
  Real x1size = s.gx1max - s.gx1min, x2size = s.gx2max - s.gx2min, x3size = s.gx3max - s.gx3min;
  s.lw_wave_flag = wave_flag, s.lw_amp = amp, s.lw_vflow = vflow;
  s.lw_cos_a3 = 1.0, s.lw_sin_a3 = 0.0, s.lw_cos_a2 = 1.0, s.lw_sin_a2 = 0.0;
  if (multi_d && !(along_x1)) {
    Real ang_3 = std::atan(x1size / x2size);
    s.lw_sin_a3 = std::sin(ang_3);
    s.lw_cos_a3 = std::cos(ang_3);
  }
  if (three_d && !(along_x1)) {
    Real ang_2 = std::atan(0.5 * (x1size * s.lw_cos_a3 + x2size * s.lw_sin_a3) / x3size);
    s.lw_sin_a2 = std::sin(ang_2);
    s.lw_cos_a2 = std::cos(ang_2);
  }
  if (along_x2) s.lw_cos_a3 = 0.0, s.lw_sin_a3 = 1.0, s.lw_cos_a2 = 1.0, s.lw_sin_a2 = 0.0;
  if (along_x3) s.lw_cos_a3 = 0.0, s.lw_sin_a3 = 1.0, s.lw_cos_a2 = 0.0, s.lw_sin_a2 = 1.0;
  s.lw_lambda = std::numeric_limits<float>::max();
  if (s.lw_cos_a2 * s.lw_cos_a3 > 0.0)
    s.lw_lambda = std::min(s.lw_lambda, x1size * s.lw_cos_a2 * s.lw_cos_a3);
  if (s.lw_cos_a2 * s.lw_sin_a3 > 0.0)
    s.lw_lambda = std::min(s.lw_lambda, x2size * s.lw_cos_a2 * s.lw_sin_a3);
  if (s.lw_sin_a2 > 0.0) s.lw_lambda = std::min(s.lw_lambda, x3size * s.lw_sin_a2);
  s.lw_k_par = 2.0 * (M_PI) / s.lw_lambda;
  s.lw_d0 = 1.0;
  s.lw_v1_0 = vflow;
  s.lw_gamma = s.c.gamma;
  s.lw_gm1 = s.lw_gamma - 1.0;
  s.lw_p0 = 1.0 / s.lw_gamma;
  if (eigen) {
    const Real d = s.lw_d0, v1 = s.lw_v1_0, v2 = 0.0, v3 = 0.0, p = s.lw_p0, gamma = s.lw_gamma;
    Real vsq = v1 * v1 + v2 * v2 + v3 * v3;
    Real hh = (p / (gamma - 1.0) + 0.5 * d * vsq + p) / d;
    Real a = std::sqrt(gamma * p / d);
    Real(&rem)[5][5] = s.lw_rem;
    s.lw_ev[0] = v1 - a, s.lw_ev[1] = v1, s.lw_ev[2] = v1, s.lw_ev[3] = v1, s.lw_ev[4] = v1 + a;
    rem[0][0] = 1.0, rem[1][0] = v1 - a, rem[2][0] = v2, rem[3][0] = v3, rem[4][0] = hh - v1 * a;
    rem[0][1] = 0.0, rem[1][1] = 0.0, rem[2][1] = 1.0, rem[3][1] = 0.0, rem[4][1] = v2;
    rem[0][2] = 0.0, rem[1][2] = 0.0, rem[2][2] = 0.0, rem[3][2] = 1.0, rem[4][2] = v3;
    rem[0][3] = 1.0, rem[1][3] = v1, rem[2][3] = v2, rem[3][3] = v3, rem[4][3] = 0.5 * vsq;
    rem[0][4] = 1.0, rem[1][4] = v1 + a, rem[2][4] = v2, rem[3][4] = v3, rem[4][4] = hh + v1 * a;
  }
}

double oracle_pgen_linear_wave(void *h, int wave_flag, double amp, double vflow, int along_x1,
                               int along_x2, int along_x3, double nperiod) {
  Sim &s = *static_cast<Sim *>(h);
  lw_setup(s, wave_flag, amp, vflow, along_x1, along_x2, along_x3, true);
  const int nsp = s.c.ns_gas;
  for (int k = 0; k < s.nk; ++k)
    for (int j = 0; j < s.nj; ++j)
      for (int i = 0; i < s.ni; ++i) {
        const BBox b = bbox(s, k, j, i);
        const Real x1 = x1v(b), x2 = x2v(b), x3 = x3v(b);
        Real x = s.lw_cos_a2 * (x1 * s.lw_cos_a3 + x2 * s.lw_sin_a3) + x3 * s.lw_sin_a2;
        Real sn = std::sin(s.lw_k_par * x);
        Real mx = s.lw_d0 * s.lw_vflow + s.lw_amp * sn * s.lw_rem[1][wave_flag];
        Real my = s.lw_amp * sn * s.lw_rem[2][wave_flag];
        Real mz = s.lw_amp * sn * s.lw_rem[3][wave_flag];
        const Real cd = s.lw_d0 + s.lw_amp * sn * s.lw_rem[0][wave_flag];
        const Real cm1 =
            mx * s.lw_cos_a2 * s.lw_cos_a3 - my * s.lw_sin_a3 - mz * s.lw_sin_a2 * s.lw_cos_a3;
        const Real cm2 =
            mx * s.lw_cos_a2 * s.lw_sin_a3 + my * s.lw_cos_a3 - mz * s.lw_sin_a2 * s.lw_sin_a3;
        const Real cm3 = mx * s.lw_sin_a2 + mz * s.lw_cos_a2;
        const Real ce = s.lw_p0 / s.lw_gm1 + 0.5 * s.lw_d0 * (s.lw_v1_0) * (s.lw_v1_0) +
                        s.lw_amp * sn * s.lw_rem[4][wave_flag];
        const Real cu = ce - 0.5 * (SQR(cm1) + SQR(cm2) + SQR(cm3)) / cd;
        const size_t c = IDX(s, k, j, i);
        s.gprim[0 * s.N + c] = cd;
        s.gprim[(nsp + 0) * s.N + c] = cm1 / cd;
        s.gprim[(nsp + 1) * s.N + c] = cm2 / cd;
        s.gprim[(nsp + 2) * s.N + c] = cm3 / cd;
        s.gprim[(5 * nsp) * s.N + c] = cu / cd;
      }
  prim_to_cons(s);
  return nperiod * (std::abs(s.lw_lambda / s.lw_ev[wave_flag])); // linear_wave.hpp:214-215
}

// pgen/linear_wave.hpp:267-377 UserWorkAfterLoop: out[0] = rms, out[1..5] = L1 of d, M1..3, E
// (this block's contribution already divided by the GLOBAL volume; sum blocks' L1 before rms
// when running decomposed: pass do_rms = 0 and finish on the caller's side).
void oracle_linear_wave_errors(void *h, double *out, int do_rms) {
  Sim &s = *static_cast<Sim *>(h);
  const int nsp = s.c.ns_gas;
  const int wf = s.lw_wave_flag;
  Real l1[5] = {0, 0, 0, 0, 0};
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const BBox b = bbox(s, k, j, i);
        const Real x1 = x1v(b), x2 = x2v(b), x3 = x3v(b);
        Real vol = volume(b);
        Real x = s.lw_cos_a2 * (x1 * s.lw_cos_a3 + x2 * s.lw_sin_a3) + x3 * s.lw_sin_a2;
        Real sn = std::sin(s.lw_k_par * x);
        Real mx = s.lw_d0 * s.lw_vflow + s.lw_amp * sn * s.lw_rem[1][wf];
        Real my = s.lw_amp * sn * s.lw_rem[2][wf];
        Real mz = s.lw_amp * sn * s.lw_rem[3][wf];
        Real ca = s.lw_d0 + s.lw_amp * sn * s.lw_rem[0][wf];
        Real cm1 =
            mx * s.lw_cos_a2 * s.lw_cos_a3 - my * s.lw_sin_a3 - mz * s.lw_sin_a2 * s.lw_cos_a3;
        Real cm2 =
            mx * s.lw_cos_a2 * s.lw_sin_a3 + my * s.lw_cos_a3 - mz * s.lw_sin_a2 * s.lw_sin_a3;
        Real cm3 = mx * s.lw_sin_a2 + mz * s.lw_cos_a2;
        Real ce = s.lw_p0 / s.lw_gm1 + 0.5 * s.lw_d0 * (s.lw_v1_0) * (s.lw_v1_0) +
                  s.lw_amp * sn * s.lw_rem[4][wf];
        const size_t c = IDX(s, k, j, i);
        l1[0] += vol * std::abs(s.gu0[0 * s.N + c] - ca);
        l1[1] += vol * std::abs(s.gu0[(nsp + 0) * s.N + c] - cm1);
        l1[2] += vol * std::abs(s.gu0[(nsp + 1) * s.N + c] - cm2);
        l1[3] += vol * std::abs(s.gu0[(nsp + 2) * s.N + c] - cm3);
        l1[4] += vol * std::abs(s.gu0[(4 * nsp) * s.N + c] - ce);
      }
  Real vol = (s.gx1max - s.gx1min) * (s.gx2max - s.gx2min) * (s.gx3max - s.gx3min);
  Real rms = 0.0;
  for (int i = 0; i < 5; ++i) {
    l1[i] = l1[i] / vol;
    out[1 + i] = l1[i];
    rms += SQR(l1[i]);
  }
  out[0] = do_rms ? std::sqrt(rms) : 0.0;
}

// pgen/advection.hpp:62-217 ProblemGenerator (gas + two counter-streaming dust species).
double oracle_pgen_advection(void *h, double amp, double vflow, int along_x1, int along_x2,
                             int along_x3, double nperiod) {
  Sim &s = *static_cast<Sim *>(h);
  lw_setup(s, 0, amp, vflow, along_x1, along_x2, along_x3, false);
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  for (int k = 0; k < s.nk; ++k)
    for (int j = 0; j < s.nj; ++j)
      for (int i = 0; i < s.ni; ++i) {
        const BBox b = bbox(s, k, j, i);
        const Real x1 = x1v(b), x2 = x2v(b), x3 = x3v(b);
        Real x = s.lw_cos_a2 * (x1 * s.lw_cos_a3 + x2 * s.lw_sin_a3) + x3 * s.lw_sin_a2;
        Real sn = std::sin(s.lw_k_par * x);
        Real mx = s.lw_d0 * s.lw_vflow + s.lw_amp * sn * s.lw_v1_0;
        const Real cd = s.lw_d0 + s.lw_amp * sn;
        const Real cm1 = mx * s.lw_cos_a2 * s.lw_cos_a3;
        const Real cm2 = mx * s.lw_cos_a2 * s.lw_sin_a3;
        const Real cm3 = mx * s.lw_sin_a2;
        const Real ce = s.lw_p0 / s.lw_gm1 + 0.5 * s.lw_d0 * SQR(s.lw_v1_0) +
                        0.5 * s.lw_d0 * s.lw_amp * sn * SQR(s.lw_v1_0);
        const Real cu = ce - 0.5 * (SQR(cm1) + SQR(cm2) + SQR(cm3)) / cd;
        const size_t c = IDX(s, k, j, i);
        if (ng_) {
          s.gprim[0 * s.N + c] = cd;
          s.gprim[(ng_ + 0) * s.N + c] = cm1 / cd;
          s.gprim[(ng_ + 1) * s.N + c] = cm2 / cd;
          s.gprim[(ng_ + 2) * s.N + c] = cm3 / cd;
          s.gprim[(5 * ng_) * s.N + c] = cu / cd;
        }
        if (nd_ == 2) {
          s.dprim[0 * s.N + c] = cd;
          s.dprim[(nd_ + 0) * s.N + c] = cm1 / cd;
          s.dprim[(nd_ + 1) * s.N + c] = cm2 / cd;
          s.dprim[(nd_ + 2) * s.N + c] = cm3 / cd;
          s.dprim[1 * s.N + c] = cd;
          s.dprim[(nd_ + 3 + 0) * s.N + c] = -cm1 / cd;
          s.dprim[(nd_ + 3 + 1) * s.N + c] = -cm2 / cd;
          s.dprim[(nd_ + 3 + 2) * s.N + c] = -cm3 / cd;
        }
      }
  prim_to_cons(s);
  return nperiod * (std::abs(s.lw_lambda / s.lw_v1_0)); // advection.hpp:167-168
}

// pgen/advection.hpp:224-405: out[0..2] = rms gas, dust1, dust2; out[3..15] = 13 L1 columns.
void oracle_advection_errors(void *h, double *out) {
  Sim &s = *static_cast<Sim *>(h);
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  Real l1[13];
  for (int i = 0; i < 13; ++i) l1[i] = 0.0;
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const BBox b = bbox(s, k, j, i);
        const Real x1 = x1v(b), x2 = x2v(b), x3 = x3v(b);
        Real vol = volume(b);
        Real x = s.lw_cos_a2 * (x1 * s.lw_cos_a3 + x2 * s.lw_sin_a3) + x3 * s.lw_sin_a2;
        Real sn = std::sin(s.lw_k_par * x);
        Real mx = s.lw_d0 * s.lw_vflow + s.lw_amp * sn * s.lw_v1_0;
        Real cd = s.lw_d0 + s.lw_amp * sn;
        Real cm1 = mx * s.lw_cos_a2 * s.lw_cos_a3;
        Real cm2 = mx * s.lw_cos_a2 * s.lw_sin_a3;
        Real cm3 = mx * s.lw_sin_a2;
        Real ce = s.lw_p0 / s.lw_gm1 + 0.5 * s.lw_d0 * SQR(s.lw_v1_0) +
                  0.5 * s.lw_d0 * s.lw_amp * sn * SQR(s.lw_v1_0);
        const size_t c = IDX(s, k, j, i);
        if (ng_) {
          l1[0] += vol * std::abs(s.gu0[0 * s.N + c] - cd);
          l1[1] += vol * std::abs(s.gu0[(ng_ + 0) * s.N + c] - cm1);
          l1[2] += vol * std::abs(s.gu0[(ng_ + 1) * s.N + c] - cm2);
          l1[3] += vol * std::abs(s.gu0[(ng_ + 2) * s.N + c] - cm3);
          l1[4] += vol * std::abs(s.gu0[(4 * ng_) * s.N + c] - ce);
        }
        if (nd_ == 2) {
          l1[5] += vol * std::abs(s.du0[0 * s.N + c] - cd);
          l1[6] += vol * std::abs(s.du0[(nd_ + 0) * s.N + c] - cm1);
          l1[7] += vol * std::abs(s.du0[(nd_ + 1) * s.N + c] - cm2);
          l1[8] += vol * std::abs(s.du0[(nd_ + 2) * s.N + c] - cm3);
          l1[9] += vol * std::abs(s.du0[1 * s.N + c] - cd);
          l1[10] += vol * std::abs(s.du0[(nd_ + 3 + 0) * s.N + c] + cm1);
          l1[11] += vol * std::abs(s.du0[(nd_ + 3 + 1) * s.N + c] + cm2);
          l1[12] += vol * std::abs(s.du0[(nd_ + 3 + 2) * s.N + c] + cm3);
        }
      }
  Real vol = (s.gx1max - s.gx1min) * (s.gx2max - s.gx2min) * (s.gx3max - s.gx3min);
  for (int i = 0; i < 13; ++i) l1[i] = l1[i] / vol;
  Real rg = 0, r1 = 0, r2 = 0;
  for (int i = 0; i < 5; ++i) rg += SQR(l1[i]);
  for (int i = 5; i < 9; ++i) r1 += SQR(l1[i]);
  for (int i = 9; i < 13; ++i) r2 += SQR(l1[i]);
  out[0] = std::sqrt(rg), out[1] = std::sqrt(r1), out[2] = std::sqrt(r2);
  for (int i = 0; i < 13; ++i) out[3 + i] = l1[i];
}

// utils/history.hpp:29-100 volume integrals registered at gas.cpp:648-676 / dust.cpp:332-352:
// out = [gas mass, mom1, mom2, mom3, energy, internal energy] for gas species 0, then
// [mass, mom1, mom2, mom3] per dust species.
void oracle_history(void *h, double *out) {
  Sim &s = *static_cast<Sim *>(h);
  const int ng_ = s.c.ns_gas, nd_ = s.c.ns_dust;
  const int nout = 6 + 4 * nd_;
  for (int i = 0; i < nout; ++i) out[i] = 0.0;
  for (int k = s.ks; k <= s.ke; ++k)
    for (int j = s.js; j <= s.je; ++j)
      for (int i = s.is; i <= s.ie; ++i) {
        const Real vv = Coords(s, k, j, i).Volume(); // history.hpp:49-50
        const size_t c = IDX(s, k, j, i);
        if (ng_) {
          out[0] += s.gu0[0 * s.N + c] * vv;
          out[1] += s.gu0[(ng_ + 0) * s.N + c] * vv;
          out[2] += s.gu0[(ng_ + 1) * s.N + c] * vv;
          out[3] += s.gu0[(ng_ + 2) * s.N + c] * vv;
          out[4] += s.gu0[(4 * ng_) * s.N + c] * vv;
          out[5] += s.gu0[(5 * ng_) * s.N + c] * vv;
        }
        for (int n = 0; n < nd_; ++n) {
          out[6 + 4 * n + 0] += s.du0[n * s.N + c] * vv;
          for (int d = 0; d < 3; ++d)
            out[6 + 4 * n + 1 + d] += s.du0[(nd_ + 3 * n + d) * s.N + c] * vv;
        }
      }
}

// Leaf functions exposed for table tests.
void oracle_plm(double qm, double q, double qp, double *ql_ip1, double *qr_i) {
  PLM(qm, q, qp, *ql_ip1, *qr_i);
}
void oracle_ppm4(double qmm, double qm, double q, double qp, double qpp, double *ql_ip1,
                 double *qr_i) {
  PPM4(qmm, qm, q, qp, qpp, *ql_ip1, *qr_i);
}
// wl/wr = [rho, vx, vy, vz, P, sie] (dust: first four); out = FaceOut as 8 doubles.
void oracle_riemann(int fluid, int solver, double gm1, const double *wl, const double *wr,
                    double *out) {
  FaceOut o = {0, 0, 0, 0, 0, 0, 0, 0};
  if (fluid == FL_GAS) {
    if (solver == RS_HLLC)
      hllc_gas(gm1, wl[0], wl[1], wl[2], wl[3], wl[4], wl[5], wr[0], wr[1], wr[2], wr[3], wr[4],
               wr[5], o);
    else if (solver == RS_HLLE)
      hlle_gas(gm1, wl[0], wl[1], wl[2], wl[3], wl[4], wl[5], wr[0], wr[1], wr[2], wr[3], wr[4],
               wr[5], o);
    else
      llf_gas(gm1, wl[0], wl[1], wl[2], wl[3], wl[4], wl[5], wr[0], wr[1], wr[2], wr[3], wr[4],
              wr[5], o);
  } else {
    if (solver == RS_HLLE)
      hlle_dust(wl[0], wl[1], wl[2], wl[3], wr[0], wr[1], wr[2], wr[3], o);
    else
      llf_dust(wl[0], wl[1], wl[2], wl[3], wr[0], wr[1], wr[2], wr[3], o);
  }
  out[0] = o.fd, out[1] = o.fmx, out[2] = o.fmy, out[3] = o.fmz, out[4] = o.fe, out[5] = o.feg;
  out[6] = o.pf, out[7] = o.vf;
}
// The same leaves over tables of n inputs (tests/test_reference_leaves.py holds them against the reference's
// own headers, oracle/ref/ref_leaves.cpp); rows of wl / wr / out as in oracle_riemann.
void oracle_plm_n(long n, const double *qm, const double *q, const double *qp, double *ql_ip1, double *qr_i) {
  for (long t = 0; t < n; ++t) PLM(qm[t], q[t], qp[t], ql_ip1[t], qr_i[t]);
}
void oracle_ppm4_n(long n, const double *qmm, const double *qm, const double *q, const double *qp,
                   const double *qpp, double *ql_ip1, double *qr_i) {
  for (long t = 0; t < n; ++t) PPM4(qmm[t], qm[t], q[t], qp[t], qpp[t], ql_ip1[t], qr_i[t]);
}
void oracle_plm_g(long n, const double *qm, const double *q, const double *qp, const double *xm,
                  const double *xc, const double *xp, const double *xf0, const double *xf1, const double *dx,
                  double *ql_ip1, double *qr_i) {
  for (long t = 0; t < n; ++t) {
    const Real xf[2] = {xf0[t], xf1[t]};
    PLM_G(qm[t], q[t], qp[t], ql_ip1[t], qr_i[t], xm[t], xc[t], xp[t], xf, dx[t]);
  }
}
void oracle_riemann_n(int fluid, int solver, double gm1, long n, const double *wl, const double *wr,
                      double *out) {
  const int nv = (fluid == FL_GAS) ? 6 : 4;
  for (long t = 0; t < n; ++t) oracle_riemann(fluid, solver, gm1, wl + t * nv, wr + t * nv, out + t * 8);
}
// {x1 of face 0, dx1, x2 of face 0, dx2, x3 of face 0, dx3}: the block's logical coordinates, Xf(d, i) = f0 + i * dx
void oracle_geom(void *h, double *out) {
  Sim &s = *static_cast<Sim *>(h);
  for (int d = 0; d < 3; ++d) out[2 * d] = s.f0[d], out[2 * d + 1] = s.dx[d];
}
// What the hot path reads of Coords at n cells, 31 doubles a cell, in ref_coords' order: Volume, lower AreaX1..3,
// x1v..x3v, hx1v..hx3v, dh{1,2,3}dx1, dh{1,2,3}dx2, dh{1,2,3}dx3, cell widths X1..X3, hx1..3 at the lower X1, X2
// and X3 face centres.
void oracle_coords(void *h, const int *k, const int *j, const int *i, long n, double *out) {
  Sim &s = *static_cast<Sim *>(h);
  for (long t = 0; t < n; ++t) {
    double *o = out + t * 31;
    const Coords c(s, k[t], j[t], i[t]);
    Real a[2], w[3], hv[3], c1[3], c2[3];
    o[0] = c.Volume();
    c.GetFaceAreaX1(a), o[1] = a[0];
    c.GetFaceAreaX2(a), o[2] = a[0];
    c.GetFaceAreaX3(a), o[3] = a[0];
    o[4] = c.x1v(), o[5] = c.x2v(), o[6] = c.x3v();
    c.GetScaleFactors(hv), o[7] = hv[0], o[8] = hv[1], o[9] = hv[2];
    c.GetConnX1(c1), c.GetConnX2(c2);
    o[10] = c1[0], o[11] = c1[1], o[12] = c1[2];
    o[13] = c2[0], o[14] = c2[1], o[15] = c2[2];
    o[16] = 0.0, o[17] = 0.0, o[18] = 0.0; // x3dep() is false for every system (geometry.hpp:110-113)
    c.GetCellWidths(w), o[19] = w[0], o[20] = w[1], o[21] = w[2];
    Real xf[3][3];
    c.FaceCenX1(0, xf[0]), c.FaceCenX2(0, xf[1]), c.FaceCenX3(0, xf[2]);
    for (int d = 0; d < 3; ++d) {
      o[22 + 3 * d + 0] = c.hx1(xf[d][0], xf[d][1], xf[d][2]);
      o[22 + 3 * d + 1] = c.hx2(xf[d][0], xf[d][1], xf[d][2]);
      o[22 + 3 * d + 2] = c.hx3(xf[d][0], xf[d][1], xf[d][2]);
    }
  }
}

} // extern "C"
