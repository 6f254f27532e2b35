// One HIP kernel per Parthenon task of the reference's stage (artemis_driver.cpp:182-261).
// These back the per-task C-ABI entry points (drop-in granularity); the fast path is the
// fused stage kernel in kernels_fused.hip, which must agree with this chain bit for bit.
//
// Thread mapping everywhere: threadIdx.x walks i (contiguous, coalesced 8-byte lanes),
// blockIdx.y/threadIdx.y walk j, blockIdx.z walks (block, k).
#include <cfloat>
#include <map>
#include <vector>

#include "device_math.hpp"
#include "geometry.hpp"
#include "kernels.hpp"
#include "options.hpp"
#include "task_device.hpp"
#include "pack_view.hpp"

namespace artemis {

namespace {
constexpr int TX = 64, TY = 4;

struct Range3 {
  int il, iu, jl, ju, kl, ku;
};
// Thread shape of the one-thread-per-zone kernels: 64 x 4 by default; for narrow mesh blocks (refined meshes
// run 16^3 blocks) the x1 extent of the workgroup shrinks to the next power of two >= nx and the rows it
// frees fold along x2, so that a wave's 64 lanes stay on real zones (a 16-zone row filled a quarter of them).
inline dim3 tile_threads(int nx) {
  int tx = TX;
  while (tx > 8 && tx / 2 >= nx) tx >>= 1;
  return dim3(tx, TX * TY / tx);
}
struct Shape {
  dim3 grid, block;
};
// Ranges the tiles cover badly -- the 17 x 17 x 9 face range of a 16 x 16 x 8 block of a
// refined mesh fills 38 % of the lanes of 32 x 8 tiles; below 60 % a range is walked FLAT instead: 256 consecutive zones of
// the range per workgroup (block shape (256, 1, 1), which no tile has, is how the kernels tell).
inline Shape shape_for(const Range3 &r, int nb) {
  const int nx = r.iu - r.il + 1, ny = r.ju - r.jl + 1, nz = r.ku - r.kl + 1;
  Shape s;
  s.block = tile_threads(nx);
  const int tx = s.block.x, ty = s.block.y;
  s.grid = dim3((nx + tx - 1) / tx, (ny + ty - 1) / ty, nz * nb);
  const long covered = static_cast<long>(s.grid.x) * tx * s.grid.y * ty, used = static_cast<long>(nx) * ny;
  if (used * 10 < covered * 6 && !opt(OPT_NO_FLAT_RANGES)) {
    s.block = dim3(TX * TY, 1, 1);
    s.grid = dim3(static_cast<unsigned>((used * nz + TX * TY - 1) / (TX * TY)), 1, nb);
  }
  return s;
}
struct CellIdx {
  int i, j, k, b;
  bool ok;
};
__device__ __forceinline__ CellIdx cell_from_grid(const Range3 &r) {
  CellIdx q;
  if (blockDim.y == 1) { // flat walk
    const int nx = r.iu - r.il + 1, ny = r.ju - r.jl + 1;
    const int p = blockIdx.x * blockDim.x + threadIdx.x, row = p / nx;
    q.i = r.il + (p - row * nx), q.j = r.jl + row % ny, q.k = r.kl + row / ny, q.b = blockIdx.z;
    q.ok = q.k <= r.ku;
  } else {
    const int nkr = r.ku - r.kl + 1;
    q.i = r.il + blockIdx.x * blockDim.x + threadIdx.x, q.j = r.jl + blockIdx.y * blockDim.y + threadIdx.y;
    q.b = blockIdx.z / nkr, q.k = r.kl + blockIdx.z % nkr;
    q.ok = q.i <= r.iu && q.j <= r.ju;
  }
  return q;
}
#define CELL_FROM_GRID(r)                                                                  \
  const CellIdx ci_ = cell_from_grid(r);                                                   \
  if (!ci_.ok) return;                                                                     \
  const int i = ci_.i, j = ci_.j, k = ci_.k, b = ci_.b;                                    \
  const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;

// ---------------------------------------------------------------------------------------
// CalculateFluxesImpl (fluid_fluxes.hpp:78-213): one thread per FACE.  The thread
// reconstructs the upper face value of the cell below the face and the lower face value of
// the cell above it straight from global memory (neighbouring threads share those lines in
// L1/L2), then solves the Riemann problem and writes the 8 (gas) / 4 (dust) face outputs.
// One face: the reconstruction and the Riemann problem of species n at the lower `dir` face of cell (k,j,i).
template <int FLUID, int RIEMANN, int RECON, bool CURV, bool TAB = false>
__device__ __forceinline__ FaceFlux flux_face(const PackView &P, int b, int k, int j, int i, long c, const int dir, const int n) {
  PlmGeo gl{}, gr{};
  double hs[3] = {1.0, 1.0, 1.0}; // ScaleMomentumFlux factors (fluid_fluxes.hpp:33-70)
  if constexpr (CURV) {
    if constexpr (RECON == 1) {
      if constexpr (TAB) { // PLM_G's weights from the per-mesh table (artemis_hip_plm_table_fill)
        gl = plm_geo_tab(P, b, dir, k - (dir == 3), j - (dir == 2), i - (dir == 1));
        gr = plm_geo_tab(P, b, dir, k, j, i);
      } else {
        gl = plm_geo(P, b, dir, k - (dir == 3), j - (dir == 2), i - (dir == 1));
        gr = plm_geo(P, b, dir, k, j, i);
      }
    }
    make_coords(P, b, k, j, i).face_scale(dir, hs);
  }
  const FluidView &f = (FLUID == 0) ? P.gas : P.dust;
  const int ns = f.ns;
  const int nv = (FLUID == 0) ? 6 * ns : 4 * ns;
  const long st = (dir == 1) ? 1 : ((dir == 2) ? P.sj : P.sk);
  const int d = dir - 1;
  const int IDN = n;
  const int ivx = ns + 3 * n + d;
  const int ivy = ns + 3 * n + (d + 1) % 3;
  const int ivz = ns + 3 * n + (d + 2) % 3;
  const int IPR = 4 * ns + n, ISE = 5 * ns + n;
  FaceFlux F;
  if constexpr (FLUID == 0) {
    Prim6 L, R;
    const double *q;
    q = f.prim[b * nv + IDN] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.d, R.d);
    q = f.prim[b * nv + ivx] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.vx, R.vx);
    q = f.prim[b * nv + ivy] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.vy, R.vy);
    q = f.prim[b * nv + ivz] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.vz, R.vz);
    q = f.prim[b * nv + IPR] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.p, R.p);
    q = f.prim[b * nv + ISE] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.e, R.e);
    riemann_gas<RIEMANN>(P.gm1, L, R, F);
  } else {
    Prim4 L, R;
    const double *q;
    q = f.prim[b * nv + IDN] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.d, R.d);
    q = f.prim[b * nv + ivx] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.vx, R.vx);
    q = f.prim[b * nv + ivy] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.vy, R.vy);
    q = f.prim[b * nv + ivz] + c;
    face_states<RECON, CURV>(q, st, gl, gr, L.vz, R.vz);
    riemann_dust<RIEMANN>(L, R, F);
  }
  if constexpr (CURV) F.fmx *= hs[d], F.fmy *= hs[(d + 1) % 3], F.fmz *= hs[(d + 2) % 3];
  return F;
}
template <int FLUID>
__device__ __forceinline__ void store_face(const PackView &P, int b, long c, const int dir, const int n, const FaceFlux &F) {
  const FluidView &f = (FLUID == 0) ? P.gas : P.dust;
  const int ns = f.ns, nv = (FLUID == 0) ? 6 * ns : 4 * ns, d = dir - 1;
  const int ivx = ns + 3 * n + d, ivy = ns + 3 * n + (d + 1) % 3, ivz = ns + 3 * n + (d + 2) % 3;
  f.flux[d][b * nv + n][c] = F.fd;
  f.flux[d][b * nv + ivx][c] = F.fmx;
  f.flux[d][b * nv + ivy][c] = F.fmy;
  f.flux[d][b * nv + ivz][c] = F.fmz;
  if constexpr (FLUID == 0) {
    f.flux[d][b * nv + 4 * ns + n][c] = F.fe;  // IEN shares the IPR slot (hllc.hpp:72)
    f.flux[d][b * nv + 5 * ns + n][c] = F.feg; // IEG shares the ISE slot (hllc.hpp:73)
    f.pflux[d][b * ns + n][c] = F.pf;
    f.vface[d][b * ns + n][c] = F.vf;
  }
}

// One launch for every active direction: the thread of cell (k,j,i) solves the lower x1, x2 and x3 faces
// it stores (the face of direction d exists where the other two indices are active), so the centre
// stencil values are fetched once and stay in L1 for the three sweeps.  The three faces of a species are solved
// first and stored afterwards: a store through the pointer tables may alias anything as far as the compiler knows,
// so stores between the sweeps kept the next sweep's loads from being issued early (three load -> solve -> store
// chains per thread, latency-bound at 3-4 waves per SIMD).
template <int FLUID, int RIEMANN, int RECON, bool CURV, bool TAB = false>
__global__ __launch_bounds__(TX *TY) void flux_kernel(const PackView P, const Range3 r) {
  CELL_FROM_GRID(r)
  const int ns = (FLUID == 0) ? P.gas.ns : P.dust.ns;
  const bool has1 = (j <= P.je && k <= P.ke), has2 = P.ndim > 1 && (i <= P.ie && k <= P.ke), has3 = P.ndim > 2 && (i <= P.ie && j <= P.je);
  if constexpr (TAB) {
    // with the geometry table a face is cheap in registers only while its two records are the only ones alive: one
    // face at a time (solve, store), which also keeps the next face's table loads behind this face's stores
    // (direction outermost: the records do not depend on the species, and hoisted out of a species loop all six
    // would be alive at once)
    if (has1)
      for (int n = 0; n < ns; ++n) store_face<FLUID>(P, b, c, 1, n, flux_face<FLUID, RIEMANN, RECON, CURV, true>(P, b, k, j, i, c, 1, n));
    if (has2)
      for (int n = 0; n < ns; ++n) store_face<FLUID>(P, b, c, 2, n, flux_face<FLUID, RIEMANN, RECON, CURV, true>(P, b, k, j, i, c, 2, n));
    if (has3)
      for (int n = 0; n < ns; ++n) store_face<FLUID>(P, b, c, 3, n, flux_face<FLUID, RIEMANN, RECON, CURV, true>(P, b, k, j, i, c, 3, n));
    return;
  }
  for (int n = 0; n < ns; ++n) {
    FaceFlux F1{}, F2{}, F3{};
    if (has1) F1 = flux_face<FLUID, RIEMANN, RECON, CURV>(P, b, k, j, i, c, 1, n);
    if (has2) F2 = flux_face<FLUID, RIEMANN, RECON, CURV>(P, b, k, j, i, c, 2, n);
    if (has3) F3 = flux_face<FLUID, RIEMANN, RECON, CURV>(P, b, k, j, i, c, 3, n);
    if (has1) store_face<FLUID>(P, b, c, 1, n, F1);
    if (has2) store_face<FLUID>(P, b, c, 2, n, F2);
    if (has3) store_face<FLUID>(P, b, c, 3, n, F3);
  }
}

template <int FLUID, int RIEMANN, int RECON>
void launch_flux_dirs(const PackView &P, hipStream_t s) {
  // faces [s, e+1] of each active direction (fluid_fluxes.hpp:105, :130, :172): the union of the three ranges
  Range3 r{P.is, P.ie + 1, P.js, P.je + (P.ndim > 1 ? 1 : 0), P.ks, P.ke + (P.ndim > 2 ? 1 : 0)};
  if (P.coords == ARTEMIS_CARTESIAN)
    hipLaunchKernelGGL((flux_kernel<FLUID, RIEMANN, RECON, false>), shape_for(r, P.nb).grid, shape_for(r, P.nb).block, 0, s, P, r);
  else if (RECON == 1 && P.plm_tab != nullptr)
    hipLaunchKernelGGL((flux_kernel<FLUID, RIEMANN, RECON, true, true>), shape_for(r, P.nb).grid, shape_for(r, P.nb).block, 0, s, P, r);
  else
    hipLaunchKernelGGL((flux_kernel<FLUID, RIEMANN, RECON, true>), shape_for(r, P.nb).grid, shape_for(r, P.nb).block, 0, s, P, r);
}
template <int FLUID, int RIEMANN>
void launch_flux_recon(const PackView &P, int recon, hipStream_t s) {
  if (recon == ARTEMIS_PCM) launch_flux_dirs<FLUID, RIEMANN, 0>(P, s);
  else if (recon == ARTEMIS_PLM) launch_flux_dirs<FLUID, RIEMANN, 1>(P, s);
  else launch_flux_dirs<FLUID, RIEMANN, 2>(P, s);
}

// ---------------------------------------------------------------------------------------
// ApplyUpdate (artemis_integrator.hpp:79-108)
template <int FLUID>
__device__ __forceinline__ void update_fluid(const PackView &P, const FluidView &f, int b, long c,
                                             const CellMetric &g, double gam0, double gam1,
                                             double beta_dt) {
  const int nv = (FLUID == 0 ? 6 : 4) * f.ns;
  const bool multi_d = P.ndim > 1, three_d = P.ndim > 2;
  for (int n = 0; n < nv; ++n) {
    const double *f1 = f.flux[0][b * nv + n];
    double divf = (g.ax1[0] * f1[c] - g.ax1[1] * f1[c + 1]);
    if (multi_d) {
      const double *f2 = f.flux[1][b * nv + n];
      divf += (g.ax2[0] * f2[c] - g.ax2[1] * f2[c + P.sj]);
    }
    if (three_d) {
      const double *f3 = f.flux[2][b * nv + n];
      divf += (g.ax3[0] * f3[c] - g.ax3[1] * f3[c + P.sk]);
    }
    double *v0 = f.cons0[b * nv + n];
    const double *v1 = f.cons1[b * nv + n];
    v0[c] = gam0 * v0[c] + gam1 * v1[c] + divf * beta_dt / g.vol;
  }
}
template <bool CURV>
__global__ __launch_bounds__(TX *TY) void apply_update_kernel(const PackView P, const Range3 r,
                                                              double gam0, double gam1,
                                                              double beta_dt) {
  CELL_FROM_GRID(r)
  const CellMetric g = cell_metric<CURV>(P, b, k, j, i);
  if (P.gas.ns) update_fluid<0>(P, P.gas, b, c, g, gam0, gam1, beta_dt);
  if (P.dust.ns) update_fluid<1>(P, P.dust, b, c, g, gam0, gam1, beta_dt);
}

// ---------------------------------------------------------------------------------------
// FluxSourceImpl (fluid_fluxes.hpp:323-418), interior cells only.  Gas: pressure gradient
// and P div(v) work (:361-393).  Metric-dependent systems, both fluids: coordinate source
// rho*dt*sum_d dh_d/dx_a*v_d^2 on momentum a (:395-415; the rotating-frame velocity is zero
// without <rotating_frame>).
template <int FLUID, bool CURV>
__global__ __launch_bounds__(TX *TY) void flux_source_kernel(const PackView P, const Range3 r,
                                                             double dt) {
  CELL_FROM_GRID(r)
  const FluidView &f = (FLUID == 0) ? P.gas : P.dust;
  const int ns = f.ns, nv = (FLUID == 0 ? 6 : 4) * ns;
  const bool multi_d = P.ndim >= 2, three_d = P.ndim == 3;
  const CellMetric g = cell_metric<CURV>(P, b, k, j, i);
  for (int n = 0; n < ns; ++n) {
    double *mx = f.cons0[b * nv + ns + 3 * n + 0];
    double *my = f.cons0[b * nv + ns + 3 * n + 1];
    double *mz = f.cons0[b * nv + ns + 3 * n + 2];
    double m1 = mx[c], m2 = multi_d || CURV ? my[c] : 0.0;
    if constexpr (FLUID == 0) {
      double *eg = f.cons0[b * nv + 5 * ns + n];
      const double *p1 = f.pflux[0][b * ns + n], *v1 = f.vface[0][b * ns + n];
      double e = eg[c];
      m1 += dt / g.dx[0] * (p1[c] - p1[c + 1]);
      e -= dt / g.vol * 0.5 * (p1[c] + p1[c + 1]) * (g.ax1[1] * v1[c + 1] - g.ax1[0] * v1[c]);
      if (multi_d) {
        const double *p2 = f.pflux[1][b * ns + n], *v2 = f.vface[1][b * ns + n];
        m2 += dt / g.dx[1] * (p2[c] - p2[c + P.sj]);
        e -= dt / g.vol * 0.5 * (p2[c] + p2[c + P.sj]) *
             (g.ax2[1] * v2[c + P.sj] - g.ax2[0] * v2[c]);
      }
      if (three_d) {
        const double *p3 = f.pflux[2][b * ns + n], *v3 = f.vface[2][b * ns + n];
        double m3 = mz[c];
        m3 += dt / g.dx[2] * (p3[c] - p3[c + P.sk]);
        e -= dt / g.vol * 0.5 * (p3[c] + p3[c + P.sk]) *
             (g.ax3[1] * v3[c + P.sk] - g.ax3[0] * v3[c]);
        mz[c] = m3;
      }
      eg[c] = e;
    }
    if constexpr (CURV) {
      const DCoords co = make_coords(P, b, k, j, i);
      const double rdt = f.prim[b * nv + n][c] * dt;
      const double vx = f.prim[b * nv + ns + 3 * n + 0][c];
      const double vy = f.prim[b * nv + ns + 3 * n + 1][c];
      const double vz = f.prim[b * nv + ns + 3 * n + 2][c];
      double vf[3];
      rotation_velocity(co, P.omf, vf);
      if (co.x1dep())
        m1 += rdt * (0.0 * sqr(vx + vf[0]) + co.dh2dx1() * sqr(vy + vf[1]) + co.dh3dx1() * sqr(vz + vf[2]));
      if (co.x2dep() && multi_d) {
        m2 += rdt * (0.0 * sqr(vx + vf[0]) + 0.0 * sqr(vy + vf[1]) + co.dh3dx2() * sqr(vz + vf[2]));
      }
    }
    mx[c] = m1;
    if (multi_d || CURV) my[c] = m2;
  }
}

// ---------------------------------------------------------------------------------------
// SetAuxillaryFields (fill_derived.cpp:54-73) + GetSpecificInternalEnergy
// (artemis_utils.hpp:43-62); Cartesian scale factors are 1.
template <bool CURV>
__global__ __launch_bounds__(TX *TY) void set_aux_kernel(const PackView P, const Range3 r) {
  CELL_FROM_GRID(r)
  const FluidView &f = P.gas;
  const int ns = f.ns, nv = 6 * ns;
  double hx[3];
  scale_factors<CURV>(P, b, k, j, i, hx);
  for (int n = 0; n < ns; ++n) {
    const double D = f.cons0[b * nv + n][c];
    const double u_d = (D > f.dfloor) ? D : f.dfloor;
    const double u_d2 = amax(D, f.dfloor);
    const double rv1 = f.cons0[b * nv + ns + 3 * n + 0][c] / hx[0];
    const double rv2 = f.cons0[b * nv + ns + 3 * n + 1][c] / hx[1];
    const double rv3 = f.cons0[b * nv + ns + 3 * n + 2][c] / hx[2];
    const double ke = 0.5 * (sqr(rv1) + sqr(rv2) + sqr(rv3)) / u_d2;
    const double e_cons = f.cons0[b * nv + 4 * ns + n][c];
    const double ue_cons = e_cons - ke;
    double *eg = f.cons0[b * nv + 5 * ns + n];
    double sie = (ue_cons > f.de_switch * e_cons) ? ue_cons / u_d2 : eg[c] / u_d2;
    sie = amax(sie, f.siefloor);
    double u_u = sie * u_d;
    const double uflr = f.siefloor * u_d;
    u_u = (u_u > uflr) ? u_u : uflr;
    eg[c] = u_u;
  }
}

// ConsToPrim (fill_derived.cpp:120-166), interior
template <bool CURV>
__global__ __launch_bounds__(TX *TY) void cons_to_prim_kernel(const PackView P, const Range3 r) {
  CELL_FROM_GRID(r)
  double hx[3];
  scale_factors<CURV>(P, b, k, j, i, hx);
  {
    const FluidView &f = P.gas;
    const int ns = f.ns, nv = 6 * ns;
    for (int n = 0; n < ns; ++n) {
      const double u_d = f.cons0[b * nv + n][c];
      const double w_d = (u_d > f.dfloor) ? u_d : f.dfloor;
      f.prim[b * nv + n][c] = w_d;
      for (int d = 0; d < 3; ++d)
        f.prim[b * nv + ns + 3 * n + d][c] = f.cons0[b * nv + ns + 3 * n + d][c] / (w_d * hx[d]);
      const double w_s = f.cons0[b * nv + 5 * ns + n][c] / w_d;
      f.prim[b * nv + 5 * ns + n][c] = (w_s > f.siefloor) ? w_s : f.siefloor;
    }
  }
  {
    const FluidView &f = P.dust;
    const int ns = f.ns, nv = 4 * ns;
    for (int n = 0; n < ns; ++n) {
      const double u_d = f.cons0[b * nv + n][c];
      const double w_d = (u_d > f.dfloor) ? u_d : f.dfloor;
      f.prim[b * nv + n][c] = w_d;
      for (int d = 0; d < 3; ++d)
        f.prim[b * nv + ns + 3 * n + d][c] = f.cons0[b * nv + ns + 3 * n + d][c] / (w_d * hx[d]);
    }
  }
}

// PrimToCons (fill_derived.cpp:212-276), entire block.  P = IdealGas (gm1*rho)*sie clamped
// at 0 (singularity-eos, recalled).
// ghosts_only: the active zones are skipped (a fused stage that stores the conserved state of the zones it updates
// leaves only the ghost zones, filled by the exchange and the physical conditions, to convert)
// (GHOSTS is a template argument so that the two forms are separate kernels in a profile)
template <bool CURV, bool GHOSTS = false>
__global__ __launch_bounds__(TX *TY) void prim_to_cons_kernel(const PackView P, const Range3 r) {
  CELL_FROM_GRID(r)
  if (GHOSTS && i >= P.is && i <= P.ie && j >= P.js && j <= P.je && k >= P.ks && k <= P.ke) return;
  double hx[3];
  scale_factors<CURV>(P, b, k, j, i, hx);
  {
    const FluidView &f = P.gas;
    const int ns = f.ns, nv = 6 * ns;
    for (int n = 0; n < ns; ++n) {
      double w_d = f.prim[b * nv + n][c];
      w_d = (w_d > f.dfloor) ? w_d : f.dfloor;
      f.prim[b * nv + n][c] = w_d;
      f.cons0[b * nv + n][c] = w_d;
      const double vel1 = f.prim[b * nv + ns + 3 * n + 0][c];
      const double vel2 = f.prim[b * nv + ns + 3 * n + 1][c];
      const double vel3 = f.prim[b * nv + ns + 3 * n + 2][c];
      f.cons0[b * nv + ns + 3 * n + 0][c] = w_d * vel1 * hx[0];
      f.cons0[b * nv + ns + 3 * n + 1][c] = w_d * vel2 * hx[1];
      f.cons0[b * nv + ns + 3 * n + 2][c] = w_d * vel3 * hx[2];
      double w_s = f.prim[b * nv + 5 * ns + n][c];
      w_s = (w_s > f.siefloor) ? w_s : f.siefloor;
      f.prim[b * nv + 5 * ns + n][c] = w_s;
      const double u_u = w_s * w_d;
      f.cons0[b * nv + 5 * ns + n][c] = u_u;
      f.prim[b * nv + 4 * ns + n][c] = amax(0.0, P.gm1 * w_d * w_s);
      const double ke = 0.5 * w_d * (sqr(vel1) + sqr(vel2) + sqr(vel3));
      f.cons0[b * nv + 4 * ns + n][c] = u_u + ke;
    }
  }
  {
    const FluidView &f = P.dust;
    const int ns = f.ns, nv = 4 * ns;
    for (int n = 0; n < ns; ++n) {
      double w_d = f.prim[b * nv + n][c];
      w_d = (w_d > f.dfloor) ? w_d : f.dfloor;
      f.prim[b * nv + n][c] = w_d;
      f.cons0[b * nv + n][c] = w_d;
      for (int d = 0; d < 3; ++d)
        f.cons0[b * nv + ns + 3 * n + d][c] = w_d * f.prim[b * nv + ns + 3 * n + d][c] * hx[d];
    }
  }
}

// DeepCopyConservedData (artemis_integrator.hpp:42-49), entire block
__global__ __launch_bounds__(TX *TY) void deep_copy_kernel(const PackView P, const Range3 r) {
  CELL_FROM_GRID(r)
  for (int n = 0; n < 6 * P.gas.ns; ++n)
    P.gas.cons1[b * 6 * P.gas.ns + n][c] = P.gas.cons0[b * 6 * P.gas.ns + n][c];
  for (int n = 0; n < 4 * P.dust.ns; ++n)
    P.dust.cons1[b * 4 * P.dust.ns + n][c] = P.dust.cons0[b * 4 * P.dust.ns + n][c];
}

// ---------------------------------------------------------------------------------------
// EstimateTimestepMesh (gas.cpp:411-433, dust.cpp:256-272): wave64 shuffle min -> LDS min over
// the 4 waves -> one atomicMin per workgroup on the bit pattern (positive doubles order like
// unsigned integers).
template <int FLUID, bool CURV>
__global__ __launch_bounds__(TX *TY) void estimate_dt_kernel(const PackView P, const Range3 r,
                                                             double cfl,
                                                             unsigned long long *dt_bits) {
  // grid-stride over the 64x4 cell tiles: a bounded number of workgroups, hence a bounded number
  // of atomics on the single result word (one atomic per tile serialises in L2 on large meshes)
  const int gx = (r.iu - r.il + TX) / TX, gy = (r.ju - r.jl + TY) / TY;
  const int nkr = r.ku - r.kl + 1;
  const long ntile = static_cast<long>(gx) * gy * nkr * P.nb;
  double ldt = DBL_MAX;
  for (long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int i = r.il + static_cast<int>(tile % gx) * TX + threadIdx.x;
    const int j = r.jl + static_cast<int>((tile / gx) % gy) * TY + threadIdx.y;
    const int bz = static_cast<int>(tile / (static_cast<long>(gx) * gy));
    const int b = bz / nkr;
    const int k = r.kl + bz % nkr;
    if (i > r.iu || j > r.ju) continue;
    const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;
    double dx[3]; // GetCellWidths (geometry.hpp:352-361)
    if constexpr (CURV) {
      const DCoords co = make_coords(P, b, k, j, i);
      dx[0] = co.width1(), dx[1] = co.width2(), dx[2] = co.width3();
    } else {
      const CellGeom g = cell_geom(P.geom + 6 * b, k, j, i);
      dx[0] = 1.0 * g.dx1, dx[1] = 1.0 * g.dx2, dx[2] = 1.0 * g.dx3;
    }
    const FluidView &f = (FLUID == 0) ? P.gas : P.dust;
    const int ns = f.ns, nv = (FLUID == 0 ? 6 : 4) * ns;
    for (int n = 0; n < ns; ++n) {
      double denom = 0.0;
      if constexpr (FLUID == 0) {
        const double dens = f.prim[b * nv + n][c];
        const double sie = f.prim[b * nv + 5 * ns + n][c];
        const double bulk = (P.gm1 + 1.0) * P.gm1 * dens * sie; // IdealGas bulk modulus
        const double cs = sqrt(bulk / dens);
        for (int d = 0; d < P.ndim; d++) {
          const double ss = fabs(f.prim[b * nv + ns + 3 * n + d][c]) + cs;
          denom += ss / dx[d];
        }
      } else {
        for (int d = 0; d < P.ndim; d++) denom += fabs(f.prim[b * nv + ns + 3 * n + d][c]) / dx[d];
      }
      ldt = amin(ldt, 1.0 / denom);
    }
  }
  for (int off = 32; off > 0; off >>= 1) ldt = fmin(ldt, __shfl_down(ldt, off, 64));
  __shared__ double wmin[TY];
  const int lane = threadIdx.x, wave = threadIdx.y;
  if (lane == 0) wmin[wave] = ldt;
  __syncthreads();
  if (wave == 0 && lane == 0) {
    double m = wmin[0];
    for (int w = 1; w < TY; ++w) m = fmin(m, wmin[w]);
    atomicMin(dt_bits, static_cast<unsigned long long>(__double_as_longlong(cfl * m)));
  }
}

// ---------------------------------------------------------------------------------------
// Ghost fill of one face of one block (see artemis_hip_apply_bc).  The slab spans the ENTIRE
// extent of the other two dimensions.  `table` holds nfill pointers chosen by the host:
// gas rho, v, sie and dust rho, v (pressure is not FillGhost).
struct BcArgs {
  int d, side, bc;    // direction 0..2, 0 inner / 1 outer, artemis_bc
  int nfill;          // entries used in ptrs/normal
  int n_act;          // interior cells along d
  int st, en;         // interior bounds along d
  int ng;
};
// FillGhost variables are enumerated on the device straight from the pack's pointer tables
// (no host copy of the tables, hence no synchronisation and nothing to go stale).
struct FillTabs {
  double *const *gas;  // [nb][6*nsg]
  double *const *dust; // [nb][4*nsd]
  int nsg, nsd, b;
};
// The blocks one launch of a per-face condition kernel serves (blockIdx.y picks the block): a refined disk has
// hundreds of boundary blocks per face, and one 5 us launch per block and face was 14 % of its GPU time.
constexpr int FACE_BATCH = 240;
struct BlockList {
  int n; // 0: the block is FillTabs::b (single-block launch)
  int b[FACE_BATCH];
};
__device__ __forceinline__ FillTabs tabs_of(const FillTabs &t, const BlockList &l) {
  FillTabs o = t;
  if (l.n > 0) o.b = l.b[blockIdx.y];
  return o;
}
// v-th FillGhost variable of block b and whether it is the velocity component along d
__device__ __forceinline__ double *fill_var(const FillTabs &t, int v, int d, bool &normal) {
  const int ngas = 5 * t.nsg;
  if (v < ngas) {
    // gas order with the pressure block [4ns,5ns) skipped (gas.cpp:251-252)
    const int slot = (v < 4 * t.nsg) ? v : v + t.nsg;
    normal = (slot >= t.nsg && slot < 4 * t.nsg && ((slot - t.nsg) % 3) == d);
    return t.gas[t.b * 6 * t.nsg + slot];
  }
  const int w = v - ngas;
  normal = (w >= t.nsd && ((w - t.nsd) % 3) == d);
  return t.dust[t.b * 4 * t.nsd + w];
}

__global__ __launch_bounds__(256) void bc_kernel(const BcArgs a, const FillTabs t_in, int ni, int nj,
                                                 int nk, const BlockList bl) {
  const FillTabs t = tabs_of(t_in, bl);
  // slab extents: ng along d, full extent along the others
  int ext[3] = {ni, nj, nk};
  ext[a.d] = a.ng;
  const long ncell = static_cast<long>(ext[0]) * ext[1] * ext[2];
  const long tid = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= ncell) return;
  int idx[3];
  idx[0] = tid % ext[0];
  idx[1] = (tid / ext[0]) % ext[1];
  idx[2] = tid / (static_cast<long>(ext[0]) * ext[1]);
  const int g = idx[a.d];
  int gi, si;
  if (a.side == 0) {
    gi = a.st - 1 - g;
    si = (a.bc == ARTEMIS_BC_PERIODIC) ? gi + a.n_act
                                       : ((a.bc == ARTEMIS_BC_OUTFLOW) ? a.st : 2 * a.st - 1 - gi);
  } else {
    gi = a.en + 1 + g;
    si = (a.bc == ARTEMIS_BC_PERIODIC) ? gi - a.n_act
                                       : ((a.bc == ARTEMIS_BC_OUTFLOW) ? a.en : 2 * a.en + 1 - gi);
  }
  int dst[3] = {idx[0], idx[1], idx[2]}, src[3] = {idx[0], idx[1], idx[2]};
  dst[a.d] = gi, src[a.d] = si;
  const long cd = (static_cast<long>(dst[2]) * nj + dst[1]) * ni + dst[0];
  const long cs = (static_cast<long>(src[2]) * nj + src[1]) * ni + src[0];
  for (int v = 0; v < a.nfill; ++v) {
    bool normal;
    double *q = fill_var(t, v, a.d, normal);
    const double sgn = (a.bc == ARTEMIS_BC_REFLECT && normal) ? -1.0 : 1.0;
    q[cd] = sgn * q[cs];
  }
}

// The `strat` problem's user conditions (pgen/strat.hpp:158-466).  One thread per ghost zone of
// the (d, side) slab.  x1 `extrap` (:188-226, :262-299): density, sie and v3 copied from the first
// active zone, v1 copied unless it points into the domain, v2 extrapolated linearly in x1v.
// x2 `inflow` (:352-392, :437-466): copy, with v2 = -q Om0 x1v where the shear carries material
// into the box (lower face: x1f >= 0, upper face: x1f < 0) and one-way outflow elsewhere.
// Gas species 0 and every dust species, like the reference's loops.
struct StratBcArgs {
  int d, side, ng, st, en;
  int both; // one launch fills the inner and the outer slab (disjoint zones, both read active zones only)
  double q, om0, x1f0, dx1;
};
__global__ __launch_bounds__(256) void strat_bc_kernel(const StratBcArgs a_in, const FillTabs t_in,
                                                       const double *geom, int ni, int nj, int nk, const BlockList bl) {
  const FillTabs t = tabs_of(t_in, bl);
  StratBcArgs a = a_in;
  int ext[3] = {ni, nj, nk};
  ext[a.d] = a.ng;
  const long ncell = static_cast<long>(ext[0]) * ext[1] * ext[2];
  long tid = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (a.both) {
    a.side = (tid >= ncell) ? 1 : 0;
    tid -= a.side * ncell;
  }
  if (tid >= ncell) return;
  int idx[3];
  idx[0] = tid % ext[0];
  idx[1] = (tid / ext[0]) % ext[1];
  idx[2] = tid / (static_cast<long>(ext[0]) * ext[1]);
  idx[a.d] = (a.side == 0) ? a.st - 1 - idx[a.d] : a.en + 1 + idx[a.d];
  const int i = idx[0], j = idx[1], k = idx[2];
  const long c = (static_cast<long>(k) * nj + j) * ni + i;
  const double *g = geom + 6 * t.b;
  auto x1v = [&](int ii) { return 0.5 * ((g[0] + ii * g[1]) + (g[0] + (ii + 1) * g[1])); };
  const int nsg = t.nsg, nsd = t.nsd;
  if (a.d == 0) {
    const int ia = (a.side == 0) ? a.st : a.en, ib = (a.side == 0) ? a.st + 1 : a.en - 1;
    const long ca = c - i + ia, cb = c - i + ib;
    const double x0 = x1v(ia), x1 = x1v(ib);
    const double dx = (a.side == 0) ? (x1 - x0) : (x0 - x1);
    const double x = x1v(i);
    auto fill = [&](double *const *tab, int base, int ns, int n) {
      double *q1 = tab[base + ns + 3 * n + 0], *q2 = tab[base + ns + 3 * n + 1];
      double *q3 = tab[base + ns + 3 * n + 2], *qd = tab[base + n];
      const double v1 = q1[ca], v2 = q2[ca], v3 = q3[ca], v2n = q2[cb];
      const double vx1 = (a.side == 0) ? ((v1 > 0.0) ? 0.0 : v1) : ((v1 < 0.0) ? 0.0 : v1);
      const double vx2 = (a.side == 0) ? (v2 + (v2n - v2) * (x - x0) / dx) : (v2 + (v2 - v2n) * (x - x0) / dx);
      q1[c] = vx1, q2[c] = vx2, q3[c] = v3, qd[c] = qd[ca];
    };
    if (nsg) {
      fill(t.gas, t.b * 6 * nsg, nsg, 0);
      double *se = t.gas[t.b * 6 * nsg + 5 * nsg];
      se[c] = se[ca];
    }
    for (int n = 0; n < nsd; ++n) fill(t.dust, t.b * 4 * nsd, nsd, n);
  } else if (a.d == 2) { // x3 `extrap` (strat.hpp:476-640): copy, no inflow in v3, density continued as a power
    // law in z through the first two active zones -- std::pow of a STATE ratio in the reference, pow()
    // on the device here: agreement with a host libm is to rounding, not bitwise
    const int ka = (a.side == 0) ? a.st : a.en, kb = (a.side == 0) ? a.st + 1 : a.en - 1;
    const long ca = c + static_cast<long>(ka - k) * ni * nj, cb = c + static_cast<long>(kb - k) * ni * nj;
    auto x3v = [&](int kk) { return 0.5 * ((g[4] + kk * g[5]) + (g[4] + (kk + 1) * g[5])); };
    const double z = x3v(k), z0 = x3v(ka), z1 = x3v(kb);
    const double dz = (a.side == 0) ? (z1 - z0) : (z0 - z1);
    auto fill = [&](double *const *tab, int base, int ns, int n) {
      double *q1 = tab[base + ns + 3 * n + 0], *q2 = tab[base + ns + 3 * n + 1];
      double *q3 = tab[base + ns + 3 * n + 2], *qd = tab[base + n];
      const double v1 = q1[ca], v2 = q2[ca], v3 = q3[ca];
      const double vx3 = (a.side == 0) ? ((v3 > 0.0) ? 0.0 : v3) : ((v3 < 0.0) ? 0.0 : v3);
      const double dd = qd[ca], dn = qd[cb];
      const double drho = (a.side == 0) ? dn / dd : dd / dn;
      q1[c] = v1, q2[c] = v2, q3[c] = vx3, qd[c] = dd * pow(drho, (z - z0) / dz);
    };
    if (nsg) {
      fill(t.gas, t.b * 6 * nsg, nsg, 0);
      double *se = t.gas[t.b * 6 * nsg + 5 * nsg];
      se[c] = se[ca];
    }
    for (int n = 0; n < nsd; ++n) fill(t.dust, t.b * 4 * nsd, nsd, n);
  } else {
    const int ja = (a.side == 0) ? a.st : a.en;
    const long ca = c + static_cast<long>(ja - j) * ni;
    const double x = x1v(i);
    const double xf = g[0] + i * g[1];
    const double vy0 = -a.q * a.om0 * x;
    auto fill = [&](double *const *tab, int base, int ns, int n) {
      double *q1 = tab[base + ns + 3 * n + 0], *q2 = tab[base + ns + 3 * n + 1];
      double *q3 = tab[base + ns + 3 * n + 2], *qd = tab[base + n];
      const double v1 = q1[ca], v2 = q2[ca], v3 = q3[ca];
      const double vx2 = (a.side == 0) ? ((xf >= 0) ? ((v2 > 0.) ? 0.0 : v2) : vy0)
                                       : ((xf < 0) ? ((v2 < 0.0) ? 0.0 : v2) : vy0);
      q1[c] = v1, q2[c] = vx2, q3[c] = v3, qd[c] = qd[ca];
    };
    if (nsg) {
      fill(t.gas, t.b * 6 * nsg, nsg, 0);
      double *se = t.gas[t.b * 6 * nsg + 5 * nsg];
      se[c] = se[ca];
    }
    for (int n = 0; n < nsd; ++n) fill(t.dust, t.b * 4 * nsd, nsd, n);
  }
}

// The `conduction` problem's user condition (pgen/conduction.hpp:105-232), Cartesian, gas species 0:
// ghost temperature from a fixed heat flux (inner faces) or a fixed value (outer faces), density
// from hydrostatic balance, velocities copied from the first active zone `ia` along d.
struct CondBcArgs {
  int d, side, ng, st, en;
  double g_temp, flux, gx, coeff, cv, gm1, temp_exp, rho_exp, T_ref, rho_ref;
  int type;
};
__global__ __launch_bounds__(256) void conductive_bc_kernel(const CondBcArgs a, const FillTabs t_in,
                                                            const PackView P, const BlockList bl) {
  const FillTabs t = tabs_of(t_in, bl);
  const int ni = P.ni, nj = P.nj, nk = P.nk;
  int ext[3] = {ni, nj, nk};
  ext[a.d] = a.ng;
  const long ncell = static_cast<long>(ext[0]) * ext[1] * ext[2];
  const long tid = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= ncell || t.nsg == 0) return;
  int idx[3];
  idx[0] = tid % ext[0];
  idx[1] = (tid / ext[0]) % ext[1];
  idx[2] = tid / (static_cast<long>(ext[0]) * ext[1]);
  idx[a.d] = (a.side == 0) ? a.st - 1 - idx[a.d] : a.en + 1 + idx[a.d];
  int ia[3] = {idx[0], idx[1], idx[2]};
  ia[a.d] = (a.side == 0) ? a.st : a.en;
  const long c = (static_cast<long>(idx[2]) * nj + idx[1]) * ni + idx[0];
  const long cA = (static_cast<long>(ia[2]) * nj + ia[1]) * ni + ia[0];
  // Coords::Distance between the two cell centres (geometry.hpp:407-412)
  double xg[3], xa[3];
  make_coords(P, t.b, idx[2], idx[1], idx[0]).centre_to_cart(xg);
  make_coords(P, t.b, ia[2], ia[1], ia[0]).centre_to_cart(xa);
  const double dist = sqrt(sqr(xg[0] - xa[0]) + sqr(xg[1] - xa[1]) + sqr(xg[2] - xa[2]));
  const bool INNER = (a.side == 0);
  const double xma = (INNER ? -1. : 1.) * dist;
  const int nsg = t.nsg;
  double *rho = t.gas[t.b * 6 * nsg + 0], *se = t.gas[t.b * 6 * nsg + 5 * nsg];
  const double da = rho[cA], siea = se[cA];
  const double Ta = amax(0.0, siea / a.cv);
  double ft = 1.0, fr = 1.0; // DiffusionCoeff::Get (diffusion_coeff.hpp:312-316, :353-359); pow() only for non-zero exponents
  if (a.temp_exp != 0.0) ft = pow(Ta / a.T_ref, a.temp_exp);
  if (a.rho_exp != 0.0) fr = pow(da / a.rho_ref, a.rho_exp);
  const double ka = (a.type == ARTEMIS_CONDUCTIVITY_PLAW) ? a.coeff * ft * fr : a.coeff * ft * fr * da * a.cv;
  double Tg = a.g_temp;
  if (INNER) Tg = Ta - a.flux * xma / ka;
  const double densg = da * (Ta - 0.5 * a.gx * xma) / (Tg + 0.5 * a.gx * xma);
  const double sieg = amax(0.0, a.cv * Tg);
  rho[c] = densg, se[c] = sieg;
  for (int q = 0; q < 3; ++q) {
    double *v = t.gas[t.b * 6 * nsg + nsg + q];
    v[c] = v[cA];
  }
}

// The `disk` problem's user conditions.  `ic` (disk.hpp:597-632): ghost zones keep the initial
// condition -- the reference re-evaluates the disk profile (std::pow / std::exp of the zone's
// position) on every call; the profile does not depend on time, so the adapter hands over the
// initial primitives once (ic_gas / ic_dust, laid out like prim) and the kernel copies the ghost
// zones from there: the same numbers bit for bit.  Gas species 0 and every dust species, like
// DiskICImpl (:325-354).
// `extrap` (disk.hpp:634-825): power-law extrapolation in ln(x) (x for Cartesian) of density,
// sie and the inertial azimuthal velocity along the fill direction, from the first two active
// zones; R and z velocities copied.  `viscous` (disk.hpp:415-595, x1 faces): the same, except that the
// gas density and radial velocity follow the steady viscous-accretion solution with the disk's
// nu(R) = nu0 (R/r0)^nu_indx and mdot.  These two evaluate log / exp / pow on the device:
// agreement with a host libm is to rounding (a few ulp), not bitwise.
struct DiskBcArgs {
  int d, side, ng, st, en, extrap, visc;
  int both; // `ic` on both faces of d: one launch, the second half of the threads takes the upper face (pure copies)
  double omf, nu0, nu_indx, r0, mdot;
  double *const *ic_gas, *const *ic_dust;
};
__global__ __launch_bounds__(256) void disk_bc_kernel(const DiskBcArgs a, const FillTabs t_in, const PackView P,
                                                      const BlockList bl) {
  const FillTabs t = tabs_of(t_in, bl);
  const int ni = P.ni, nj = P.nj, nk = P.nk;
  int ext[3] = {ni, nj, nk};
  ext[a.d] = a.ng;
  const long ncell = static_cast<long>(ext[0]) * ext[1] * ext[2];
  long tid = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  int side = a.side;
  if (a.both && tid >= ncell) tid -= ncell, side = 1;
  if (tid >= ncell) return;
  int idx[3];
  idx[0] = tid % ext[0];
  idx[1] = (tid / ext[0]) % ext[1];
  idx[2] = tid / (static_cast<long>(ext[0]) * ext[1]);
  idx[a.d] = (side == 0) ? a.st - 1 - idx[a.d] : a.en + 1 + idx[a.d];
  const long c = (static_cast<long>(idx[2]) * nj + idx[1]) * ni + idx[0];
  const int nsg = t.nsg, nsd = t.nsd;
  if (!a.extrap) {
    if (nsg) {
      const int vars[5] = {0, nsg + 0, nsg + 1, nsg + 2, 5 * nsg};
      for (int q = 0; q < 5; ++q) t.gas[t.b * 6 * nsg + vars[q]][c] = a.ic_gas[t.b * 6 * nsg + vars[q]][c];
    }
    for (int v = 0; v < 4 * nsd; ++v) t.dust[t.b * 4 * nsd + v][c] = a.ic_dust[t.b * 4 * nsd + v][c];
    return;
  }
  const bool INNER = (a.side == 0);
  int ia[3] = {idx[0], idx[1], idx[2]}, ip1[3] = {idx[0], idx[1], idx[2]}, im1[3] = {idx[0], idx[1], idx[2]};
  ia[a.d] = INNER ? a.st : a.en;
  ip1[a.d] = INNER ? a.st + 1 : a.en;
  im1[a.d] = INNER ? a.st : a.en - 1;
  const int ix1 = a.d, ix2 = (a.d + 1) % 3, ix3 = (a.d + 2) % 3;
  auto cell = [&](const int q[3]) { return (static_cast<long>(q[2]) * nj + q[1]) * ni + q[0]; };
  const long cA = cell(ia), cP = cell(ip1), cM = cell(im1);
  const DCoords co = make_coords(P, t.b, idx[2], idx[1], idx[0]), ca = make_coords(P, t.b, ia[2], ia[1], ia[0]);
  const DCoords cp1 = make_coords(P, t.b, ip1[2], ip1[1], ip1[0]), cm1 = make_coords(P, t.b, im1[2], im1[1], im1[0]);
  double xv[3], xva[3], xvp1[3], xvm1[3];
  co.centre(xv), ca.centre(xva), cp1.centre(xvp1), cm1.centre(xvm1);
  const Frame fr = cyl_frame(co.sys, xv, co.cv, co.sv), fa = cyl_frame(ca.sys, xva, ca.cv, ca.sv);
  const Frame fp1 = cyl_frame(cp1.sys, xvp1, cp1.cv, cp1.sv), fm1 = cyl_frame(cm1.sys, xvm1, cm1.cv, cm1.sv);
  const double eRa[3] = {fa.e1[0], fa.e2[0], fa.e3[0]};
  const double epa[3] = {fa.e1[1], fa.e2[1], fa.e3[1]};
  const double eza[3] = {fa.e1[2], fa.e2[2], fa.e3[2]};
  const double epp1[3] = {fp1.e1[1], fp1.e2[1], fp1.e3[1]};
  const double epm1[3] = {fm1.e1[1], fm1.e2[1], fm1.e3[1]};
  const bool lnx = (P.coords != ARTEMIS_CARTESIAN);
  const double xma = lnx ? log(xv[ix1] / xva[ix1]) : xv[ix1] - xva[ix1];
  const double dx = lnx ? log(xvp1[ix1] / xvm1[ix1]) : xvp1[ix1] - xvm1[ix1];
  const double xmadx = xma / dx;
  auto vdot = [](const double u[3], const double w[3]) { return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]; };
  double dgvp = 0.0;
  if (nsg) {
    double *rho = t.gas[t.b * 6 * nsg], *sie = t.gas[t.b * 6 * nsg + 5 * nsg];
    double *v[3] = {t.gas[t.b * 6 * nsg + nsg], t.gas[t.b * 6 * nsg + nsg + 1], t.gas[t.b * 6 * nsg + nsg + 2]};
    const double dgrho = a.visc ? 0.0 : log(rho[cP] / rho[cM]);
    const double dgsie = log(sie[cP] / sie[cM]);
    double rhog = rho[cA] * exp(dgrho * xmadx);
    const double sieg = sie[cA] * exp(dgsie * xmadx);
    const double gva[3] = {v[0][cA], v[1][cA], v[2][cA]};
    const double gvp1[3] = {v[0][cP], v[1][cP], v[2][cP]};
    const double gvm1[3] = {v[0][cM], v[1][cM], v[2][cM]};
    const double gvp = vdot(gva, epa) + a.omf * fa.x[0];
    double gvR = vdot(gva, eRa);
    const double gvz = vdot(gva, eza);
    const double gvp1p = vdot(gvp1, epp1) + a.omf * fp1.x[0];
    const double gvm1p = vdot(gvm1, epm1) + a.omf * fm1.x[0];
    dgvp = log(gvp1p / gvm1p);
    if (a.visc) { // DiskBoundaryVisc (disk.hpp:415-595): steady viscous accretion sets rho and v_R
      const double nua = a.nu0 * pow(fa.x[0] / a.r0, a.nu_indx);
      const double nug = a.nu0 * pow(fr.x[0] / a.r0, a.nu_indx);
      const double vpg = gvp * exp(dgvp * xmadx);
      const double rhoa = rho[cA];
      if (INNER) {
        rhog = rhoa * nua / nug;
        gvR = -1.5 * nug / fr.x[0];
      } else { // dFnu/dl = Mdot
        const double lg = fr.x[0] * vpg;
        const double la = fa.x[0] * gvp;
        rhog = (3.0 * M_PI * rhoa * nua * la + a.mdot * (lg - la)) / (3.0 * M_PI * nug * lg);
        gvR = -a.mdot / (2 * M_PI * fr.x[0] * rhog);
      }
    }
    const double gvcyl[3] = {gvR, gvp * exp(dgvp * xmadx) - a.omf * fr.x[0], gvz};
    const double gvel[3] = {vdot(gvcyl, fr.e1), vdot(gvcyl, fr.e2), vdot(gvcyl, fr.e3)};
    rho[c] = rhog, sie[c] = sieg;
    v[ix1][c] = gvel[ix1], v[ix2][c] = gvel[ix2], v[ix3][c] = gvel[ix3];
  }
  for (int n = 0; n < nsd; ++n) {
    double *dr = t.dust[t.b * 4 * nsd + n];
    double *v[3] = {t.dust[t.b * 4 * nsd + nsd + 3 * n], t.dust[t.b * 4 * nsd + nsd + 3 * n + 1],
                    t.dust[t.b * 4 * nsd + nsd + 3 * n + 2]};
    const double ddrho = log(dr[cP] / dr[cM]);
    const double rhod = dr[cA] * exp(ddrho * xmadx);
    const double dva[3] = {v[0][cA], v[1][cA], v[2][cA]};
    const double dvp = vdot(dva, epa) + a.omf * fa.x[0];
    const double dvR = vdot(dva, eRa);
    const double dvz = vdot(dva, eza);
    // the dust azimuthal velocity is scaled with the GAS exponent (disk.hpp:795-797)
    const double dvcyl[3] = {dvR, dvp * exp(dgvp * xmadx) - a.omf * fr.x[0], dvz};
    const double dvel[3] = {vdot(dvcyl, fr.e1), vdot(dvcyl, fr.e2), vdot(dvcyl, fr.e3)};
    dr[c] = rhod;
    v[ix1][c] = dvel[ix1], v[ix2][c] = dvel[ix2], v[ix3][c] = dvel[ix3];
  }
}

// All ghost cells of one block in ONE launch.  Parthenon applies periodic images, then x1, x2, x3
// physical conditions, each pass over the entire extent of the other dimensions; every pass
// remaps one index (and flips the sign of the normal velocity for reflecting walls), so the
// passes compose into independent per-dimension index maps: ghost cell (i,j,k) receives
// sgn * q[map3(k)][map2(j)][map1(i)].  Faces flagged `none` keep their index (their slabs were
// filled by the neighbour exchange).  Destinations are ghost in >= 1 mapped dimension, sources
// are interior in every mapped dimension: no cell is both, so the fill is race-free in place.
struct ShellArgs {
  int bc[6];
  int lo[3], hi[3], ext[3]; // interior bounds and array extents
  int ng, ndim, nfill;
  long nA, nB, nC;          // cells in the x3-, x2-, x1-ghost regions
  // `ic` faces (ARTEMIS_BC_IC: the ghost zone takes the initial state's value AT ITS OWN PLACE, pgen/disk.hpp) ride the same
  // launch: a zone whose LAST covering pass is an `ic` pass reads the initial-state tables instead of the state.  Passes
  // run periodic images first, then x1, x2, x3 physical conditions: the last one is the highest physical direction in
  // which the zone is a ghost zone; copy conditions of higher directions have remapped their own index by then, lower
  // directions and periodic images were overwritten.  The primitive floors PrimToCons would apply behind a value
  // condition (fill_derived.cpp:227-262) are applied to those zones here (floor_ghost_kernel's test).
  double *const *ic_gas, *const *ic_dust;
  double g_dfloor, g_siefloor, d_dfloor;
  int floor_ic;
};
// Up to BC_BATCH blocks per launch (blockIdx.y): block ids and their six flags travel in the kernel arguments
// (a refined mesh has hundreds of small blocks on the domain boundary; one launch per block was 30 % of the
// GPU time of inputs/disk/disk_cart.in, profiles/r02_smr_disk_cart_kernel_stats.csv).
constexpr int BC_BATCH = 256;
struct ShellBatch {
  int blk[BC_BATCH];
  unsigned char bc[BC_BATCH][6];
};
// ghost zone `tid` of the shell (regions A, B, C in turn) -> its array offset `cd`, the offset `cs` of the active zone
// it copies and the reflecting walls crossed; false where nothing is to be done
__device__ __forceinline__ bool shell_zone(const ShellArgs &a, unsigned tid, long &cd, long &cs, int &refl, bool &from_ic) {
  const unsigned nA = static_cast<unsigned>(a.nA), nB = static_cast<unsigned>(a.nB), nC = static_cast<unsigned>(a.nC);
  const unsigned e0 = a.ext[0], e1 = a.ext[1];
  int idx[3];
  const unsigned g2 = 2 * a.ng;
  if (tid < nA) { // k in ghost planes, all j, all i
    const unsigned row = tid / e0, kk = row / e1;
    idx[0] = tid - row * e0;
    idx[1] = row - kk * e1;
    idx[2] = (static_cast<int>(kk) < a.ng) ? kk : a.hi[2] + 1 + (kk - a.ng);
  } else if (tid < nA + nB) { // k interior, j in ghost rows
    tid -= nA;
    const unsigned row = tid / e0, kk = row / g2, jj = row - kk * g2;
    idx[0] = tid - row * e0;
    idx[1] = (static_cast<int>(jj) < a.ng) ? jj : a.hi[1] + 1 + (jj - a.ng);
    idx[2] = a.lo[2] + kk;
  } else if (tid < nA + nB + nC) { // k, j interior, i in ghost columns
    tid -= nA + nB;
    const unsigned ny = a.hi[1] - a.lo[1] + 1;
    const unsigned row = tid / g2, ii = tid - row * g2, kk = row / ny;
    idx[0] = (static_cast<int>(ii) < a.ng) ? ii : a.hi[0] + 1 + (ii - a.ng);
    idx[1] = a.lo[1] + (row - kk * ny);
    idx[2] = a.lo[2] + kk;
  } else {
    return false;
  }
  int src[3] = {idx[0], idx[1], idx[2]};
  refl = 0; // bit d set: reflecting wall crossed along d
  bool moved = false;
  // the highest direction whose `ic` pass covers the zone (none: -1)
  int icd = -1;
  for (int d = 0; d < a.ndim; ++d) {
    const int flag = (idx[d] < a.lo[d]) ? a.bc[2 * d] : ((idx[d] > a.hi[d]) ? a.bc[2 * d + 1] : static_cast<int>(ARTEMIS_BC_NONE));
    if (flag == ARTEMIS_BC_IC) icd = d;
  }
  from_ic = icd >= 0;
  for (int d = 0; d < a.ndim; ++d) {
    const int n_act = a.hi[d] - a.lo[d] + 1;
    int flag = ARTEMIS_BC_NONE;
    if (idx[d] < a.lo[d]) flag = a.bc[2 * d];
    else if (idx[d] > a.hi[d]) flag = a.bc[2 * d + 1];
    else continue;
    if (flag == ARTEMIS_BC_NONE) continue;
    if (flag == ARTEMIS_BC_IC) {
      moved = true;
      continue;
    }
    // (behind an `ic` pass only the copy conditions of HIGHER directions still act; periodic images came first of all)
    if (from_ic && (d < icd || flag == ARTEMIS_BC_PERIODIC)) continue;
    const bool inner = idx[d] < a.lo[d];
    if (flag == ARTEMIS_BC_PERIODIC) src[d] = inner ? idx[d] + n_act : idx[d] - n_act;
    else if (flag == ARTEMIS_BC_OUTFLOW) src[d] = inner ? a.lo[d] : a.hi[d];
    else src[d] = inner ? 2 * a.lo[d] - 1 - idx[d] : 2 * a.hi[d] + 1 - idx[d], refl |= (1 << d);
    moved = true;
  }
  cd = (static_cast<long>(idx[2]) * a.ext[1] + idx[1]) * a.ext[0] + idx[0];
  cs = (static_cast<long>(src[2]) * a.ext[1] + src[1]) * a.ext[0] + src[0];
  return moved;
}
// SHELL_ZONES zones per thread, a workgroup stride apart (coalesced): their loads of five variables are all in
// flight before the first store -- the kernel is a chain of dependent memory round trips, not bandwidth
constexpr int SHELL_ZONES = 4;
__global__ __launch_bounds__(256) void bc_shell_kernel(ShellArgs a, FillTabs t, const ShellBatch batch) {
  {
    const int q = blockIdx.y; // wave-uniform: scalar loads from the kernel-argument segment
    t.b = batch.blk[q];
    for (int f = 0; f < 6; ++f) a.bc[f] = batch.bc[q][f];
  }
  // (the three regions of one block hold < 2^31 zones: the launcher checks; 32-bit divisions)
  long cd[SHELL_ZONES], cs[SHELL_ZONES];
  int refl[SHELL_ZONES];
  bool on[SHELL_ZONES], ic[SHELL_ZONES];
#pragma unroll
  for (int z = 0; z < SHELL_ZONES; ++z) {
    const unsigned tid = (blockIdx.x * SHELL_ZONES + z) * blockDim.x + threadIdx.x;
    cd[z] = cs[z] = 0, refl[z] = 0, ic[z] = false;
    on[z] = shell_zone(a, tid, cd[z], cs[z], refl[z], ic[z]);
  }
  FillTabs ti = t; // the initial state's tables, same layout (only read where a zone comes from an `ic` pass)
  if (a.ic_gas) ti.gas = a.ic_gas;
  if (a.ic_dust) ti.dust = a.ic_dust;
  constexpr int NV = 5;
  for (int v0 = 0; v0 < a.nfill; v0 += NV) {
    double *q[NV];
    bool nrm[NV][3];
    double val[NV][SHELL_ZONES];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int v = (v0 + u < a.nfill) ? v0 + u : v0;
      q[u] = fill_var(t, v, 0, nrm[u][0]);
      fill_var(t, v, 1, nrm[u][1]);
      fill_var(t, v, 2, nrm[u][2]);
      bool unused_;
      const double *qi = fill_var(ti, v, 0, unused_);
#pragma unroll
      for (int z = 0; z < SHELL_ZONES; ++z) val[u][z] = on[z] ? (ic[z] ? qi[cs[z]] : q[u][cs[z]]) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      if (v0 + u >= a.nfill) continue;
#pragma unroll
      for (int z = 0; z < SHELL_ZONES; ++z) {
        if (!on[z]) continue;
        // sequential passes multiply by -1.0 once per reflecting wall crossed along the component's own direction
        double w = val[u][z];
        if ((refl[z] & 1) && nrm[u][0]) w = -1.0 * w;
        if ((refl[z] & 2) && nrm[u][1]) w = -1.0 * w;
        if ((refl[z] & 4) && nrm[u][2]) w = -1.0 * w;
        if (a.floor_ic && ic[z]) { // floor_ghost_kernel's test on the floored variables: gas rho, gas sie, dust rho
          const int v = v0 + u, ngas = 5 * t.nsg;
          if (v < t.nsg) w = (w > a.g_dfloor) ? w : a.g_dfloor;
          else if (v >= 4 * t.nsg && v < ngas) w = (w > a.g_siefloor) ? w : a.g_siefloor;
          else if (v >= ngas && v < ngas + t.nsd) w = (w > a.d_dfloor) ? w : a.d_dfloor;
        }
        q[u][cd[z]] = w;
      }
    }
  }
}

// Halo slab pack/unpack: slab spans the INTERIOR extent of the other dimensions.
struct HaloArgs {
  int d, side, ng, nfill;
  int lo[3], n[3]; // slab origin and extents (in cells)
};
__global__ __launch_bounds__(256) void halo_kernel(const HaloArgs a, const FillTabs t, int ni, int nj,
                                                   double *buf, int unpack) {
  const long ncell = static_cast<long>(a.n[0]) * a.n[1] * a.n[2];
  const long tid = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= ncell) return;
  const int i = a.lo[0] + tid % a.n[0];
  const int j = a.lo[1] + (tid / a.n[0]) % a.n[1];
  const int k = a.lo[2] + tid / (static_cast<long>(a.n[0]) * a.n[1]);
  const long c = (static_cast<long>(k) * nj + j) * ni + i;
  for (int v = 0; v < a.nfill; ++v) {
    bool normal;
    double *q = fill_var(t, v, a.d, normal);
    if (unpack) q[c] = buf[v * ncell + tid];
    else buf[v * ncell + tid] = q[c];
  }
}

} // namespace

// =======================================================================================
// Host launchers (declared in kernels.hpp)
#define DISPATCH_GAS(RS)                                                                   \
  case RS: launch_flux_recon<0, RS>(P, recon, s); break;

void launch_calculate_fluxes(const PackView &P, int fluid, int riemann, int recon, hipStream_t s) {
  if (fluid == ARTEMIS_GAS) {
    switch (riemann) {
      DISPATCH_GAS(0)
      DISPATCH_GAS(1)
      DISPATCH_GAS(2)
    }
  } else {
    if (riemann == ARTEMIS_HLLE) launch_flux_recon<1, 1>(P, recon, s);
    else launch_flux_recon<1, 2>(P, recon, s);
  }
}

static Range3 interior(const PackView &P) { return Range3{P.is, P.ie, P.js, P.je, P.ks, P.ke}; }
static Range3 entire(const PackView &P) { return Range3{0, P.ni - 1, 0, P.nj - 1, 0, P.nk - 1}; }

// CURV = any non-Cartesian system; the Cartesian instantiations are the ones the fused kernel
// is checked against and keep their constant-folded unit scale factors.
#define LAUNCH_GEOM(kern, r, ...)                                                               \
  do {                                                                                          \
    if (P.coords == ARTEMIS_CARTESIAN)                                                          \
      hipLaunchKernelGGL((kern<false>), shape_for(r, P.nb).grid, shape_for(r, P.nb).block, 0, s, P, r,            \
                         ##__VA_ARGS__);                                                        \
    else                                                                                        \
      hipLaunchKernelGGL((kern<true>), shape_for(r, P.nb).grid, shape_for(r, P.nb).block, 0, s, P, r,             \
                         ##__VA_ARGS__);                                                        \
  } while (0)

void launch_apply_update(const PackView &P, double gam0, double gam1, double beta_dt, hipStream_t s) {
  const Range3 r = interior(P);
  LAUNCH_GEOM(apply_update_kernel, r, gam0, gam1, beta_dt);
}
void launch_flux_source(const PackView &P, int fluid, double dt, hipStream_t s) {
  const Range3 r = interior(P);
  const dim3 g = shape_for(r, P.nb).grid, t = shape_for(r, P.nb).block;
  const bool curv = P.coords != ARTEMIS_CARTESIAN;
  if (fluid == ARTEMIS_GAS) {
    if (curv) hipLaunchKernelGGL((flux_source_kernel<0, true>), g, t, 0, s, P, r, dt);
    else hipLaunchKernelGGL((flux_source_kernel<0, false>), g, t, 0, s, P, r, dt);
  } else if (curv) { // Dust::FluxSource skips metric-free systems (dust.cpp:310-311)
    hipLaunchKernelGGL((flux_source_kernel<1, true>), g, t, 0, s, P, r, dt);
  }
}
void launch_set_aux(const PackView &P, hipStream_t s) {
  const Range3 r = interior(P);
  LAUNCH_GEOM(set_aux_kernel, r);
}
void launch_cons_to_prim(const PackView &P, hipStream_t s) {
  const Range3 r = interior(P);
  LAUNCH_GEOM(cons_to_prim_kernel, r);
}
void launch_prim_to_cons(const PackView &P, hipStream_t s, bool ghosts_only) {
  const Range3 r = entire(P);
  if (!ghosts_only) {
    LAUNCH_GEOM(prim_to_cons_kernel, r);
    return;
  }
  const Shape sh = shape_for(r, P.nb);
  if (P.coords == ARTEMIS_CARTESIAN) hipLaunchKernelGGL((prim_to_cons_kernel<false, true>), sh.grid, sh.block, 0, s, P, r);
  else hipLaunchKernelGGL((prim_to_cons_kernel<true, true>), sh.grid, sh.block, 0, s, P, r);
}
void launch_deep_copy(const PackView &P, hipStream_t s) {
  const Range3 r = entire(P);
  hipLaunchKernelGGL(deep_copy_kernel, shape_for(r, P.nb).grid, shape_for(r, P.nb).block, 0, s, P, r);
}
void launch_estimate_dt(const PackView &P, int fluid, double cfl, double *dt_dev, hipStream_t s) {
  const Range3 r = interior(P);
  auto *bits = reinterpret_cast<unsigned long long *>(dt_dev);
  const dim3 t(TX, TY); // fixed 64 x 4 tiles: grid-stride kernel with a wave reduction
  const dim3 g3((r.iu - r.il + TX) / TX, (r.ju - r.jl + TY) / TY, (r.ku - r.kl + 1) * P.nb);
  const long ntile = static_cast<long>(g3.x) * g3.y * g3.z;
  const dim3 g(static_cast<unsigned>(grid_capped(ntile < 4096 ? ntile : 4096)));
  const bool curv = P.coords != ARTEMIS_CARTESIAN;
  if (fluid == ARTEMIS_GAS) {
    if (curv) hipLaunchKernelGGL((estimate_dt_kernel<0, true>), g, t, 0, s, P, r, cfl, bits);
    else hipLaunchKernelGGL((estimate_dt_kernel<0, false>), g, t, 0, s, P, r, cfl, bits);
  } else {
    if (curv) hipLaunchKernelGGL((estimate_dt_kernel<1, true>), g, t, 0, s, P, r, cfl, bits);
    else hipLaunchKernelGGL((estimate_dt_kernel<1, false>), g, t, 0, s, P, r, cfl, bits);
  }
}

void invalidate_table_cache() {} // nothing is cached on the host any more

static FillTabs fill_tabs(const PackView &P, int b) {
  FillTabs t;
  t.gas = P.gas.prim, t.dust = P.dust.prim, t.nsg = P.gas.ns, t.nsd = P.dust.ns, t.b = b;
  return t;
}

// Sequential fallback used when a block carries a user (strat / disk / conductive) condition: those read
// neighbouring zones of the fill direction and limit velocities, so they do not compose into
// index maps.  Order as parthenon applies it: periodic images of every direction, then x1,
// x2, x3 physical / user conditions, each over the entire extent of the other dimensions.  The order only binds
// within a block, so the blocks that carry the same condition on the same face share a launch (blockIdx.y).
static void launch_bc_sequential(const PackView &P, const std::vector<int> &blocks, const int *bc,
                                 const artemis_bc_params_t *par, hipStream_t s) {
  if (blocks.empty()) return;
  const int st[3] = {P.is, P.js, P.ks}, en[3] = {P.ie, P.je, P.ke}, ext[3] = {P.ni, P.nj, P.nk};
  auto flag_of = [&](int b, int f) { return (f / 2 < P.ndim) ? bc[b * 6 + f] : static_cast<int>(ARTEMIS_BC_NONE); };
  for (int pass = 0; pass < 2; ++pass)
    for (int d = 0; d < P.ndim; ++d)
      for (int side = 0; side < 2; ++side) {
        long ncell = P.ng;
        for (int q = 0; q < 3; ++q)
          if (q != d) ncell *= ext[q];
        // group the blocks by (condition, same-on-both-faces)
        std::map<std::pair<int, int>, std::vector<int>> groups;
        for (int b : blocks) {
          const int flag = flag_of(b, 2 * d + side);
          if (flag == ARTEMIS_BC_NONE || (pass == 0) != (flag == ARTEMIS_BC_PERIODIC)) continue;
          // (`ic` copies ghost zones from the initial state: nothing it reads is written by a fill, so its two faces share a launch too)
          const bool strat = (flag == ARTEMIS_BC_STRAT_EXTRAP || flag == ARTEMIS_BC_STRAT_INFLOW || flag == ARTEMIS_BC_IC);
          const int pair = (strat && flag_of(b, 2 * d) == flag_of(b, 2 * d + 1)) ? 1 : 0; // one launch fills both faces
          if (pair && side == 1) continue;
          groups[std::make_pair(flag, pair)].push_back(b);
        }
        for (auto &kv : groups) {
          const int flag = kv.first.first, pair = kv.first.second;
          const std::vector<int> &bs = kv.second;
          for (size_t q0 = 0; q0 < bs.size(); q0 += FACE_BATCH) {
            BlockList bl;
            bl.n = static_cast<int>(std::min<size_t>(FACE_BATCH, bs.size() - q0));
            for (int q = 0; q < bl.n; ++q) bl.b[q] = bs[q0 + q];
            const FillTabs t = fill_tabs(P, bl.b[0]);
            const unsigned ny = static_cast<unsigned>(bl.n);
            if (flag == ARTEMIS_BC_CONDUCTIVE) {
              CondBcArgs a;
              a.d = d, a.side = side, a.ng = P.ng, a.st = st[d], a.en = en[d];
              a.g_temp = par->cond_temp, a.flux = par->cond_flux, a.gx = par->cond_g[d];
              a.coeff = par->cond_coeff, a.cv = par->cond_cv, a.gm1 = P.gm1, a.type = par->cond_type;
              a.temp_exp = par->cond_temp_exp, a.rho_exp = par->cond_rho_exp, a.T_ref = par->cond_T_ref;
              a.rho_ref = par->cond_rho_ref;
              hipLaunchKernelGGL(conductive_bc_kernel, dim3((ncell + 255) / 256, ny), dim3(256), 0, s, a, t, P, bl);
            } else if (flag == ARTEMIS_BC_IC || flag == ARTEMIS_BC_DISK_EXTRAP || flag == ARTEMIS_BC_DISK_VISC) {
              DiskBcArgs a;
              a.d = d, a.side = side, a.ng = P.ng, a.st = st[d], a.en = en[d];
              a.extrap = (flag != ARTEMIS_BC_IC), a.visc = (flag == ARTEMIS_BC_DISK_VISC), a.omf = par->disk_omf;
              a.nu0 = par->disk_nu0, a.nu_indx = par->disk_nu_indx, a.r0 = par->disk_r0, a.mdot = par->disk_mdot;
              a.ic_gas = par->ic_gas, a.ic_dust = par->ic_dust, a.both = pair ? 1 : 0;
              const long nthr = pair ? 2 * ncell : ncell;
              hipLaunchKernelGGL(disk_bc_kernel, dim3((nthr + 255) / 256, ny), dim3(256), 0, s, a, t, P, bl);
            } else if (flag == ARTEMIS_BC_STRAT_EXTRAP || flag == ARTEMIS_BC_STRAT_INFLOW) {
              StratBcArgs a;
              a.d = d, a.side = side, a.ng = P.ng, a.st = st[d], a.en = en[d], a.both = pair ? 1 : 0;
              a.q = par->qshear, a.om0 = par->omega, a.x1f0 = 0.0, a.dx1 = 0.0;
              const long nthr = pair ? 2 * ncell : ncell;
              hipLaunchKernelGGL(strat_bc_kernel, dim3((nthr + 255) / 256, ny), dim3(256), 0, s, a, t, P.geom,
                                 P.ni, P.nj, P.nk, bl);
            } else {
              BcArgs a;
              a.d = d, a.side = side, a.bc = flag, a.nfill = 5 * P.gas.ns + 4 * P.dust.ns;
              a.n_act = en[d] - st[d] + 1, a.st = st[d], a.en = en[d], a.ng = P.ng;
              hipLaunchKernelGGL(bc_kernel, dim3((ncell + 255) / 256, ny), dim3(256), 0, s, a, t, P.ni, P.nj,
                                 P.nk, bl);
            }
          }
        }
      }
}

// PrimToCons's primitive floors (fill_derived.cpp:227, :245, :262) on the ghost zones of block t.b
__global__ __launch_bounds__(256) void floor_ghost_kernel(const FillTabs t_in, const PackView P, const BlockList bl) {
  const FillTabs t = tabs_of(t_in, bl);
  const long n = static_cast<long>(P.ni) * P.nj * P.nk;
  const long c = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const int i = c % P.ni, j = (c / P.ni) % P.nj, k = c / (static_cast<long>(P.ni) * P.nj);
  if (i >= P.is && i <= P.ie && j >= P.js && j <= P.je && k >= P.ks && k <= P.ke) return;
  const int nsg = t.nsg, nsd = t.nsd;
  for (int m = 0; m < nsg; ++m) {
    double *rho = t.gas[t.b * 6 * nsg + m], *se = t.gas[t.b * 6 * nsg + 5 * nsg + m];
    const double w_d = rho[c], w_s = se[c];
    // (stored only where the floor acts -- almost nowhere: the pass is then reads alone; `!(w > floor)` is the
    //  reference's `(w > floor) ? w : floor` with NaN going to the floor as well)
    if (!(w_d > P.gas.dfloor)) rho[c] = P.gas.dfloor;
    if (!(w_s > P.gas.siefloor)) se[c] = P.gas.siefloor;
  }
  for (int m = 0; m < nsd; ++m) {
    double *rho = t.dust[t.b * 4 * nsd + m];
    const double w_d = rho[c];
    if (!(w_d > P.dust.dfloor)) rho[c] = P.dust.dfloor;
  }
}

int launch_apply_bc(const PackView &P, const int *bc, const artemis_bc_params_t *par, hipStream_t s) {
  // `ic` faces on the one-launch fill (the initial-state tables of every fluid present are at hand)
  const bool ic_in_shell = par && (!P.gas.ns || par->ic_gas) && (!P.dust.ns || par->ic_dust) && !opt(OPT_NO_IC_IN_SHELL);
  struct FloorAfter { // runs when the function returns
    const PackView &P;
    const artemis_bc_params_t *par;
    hipStream_t s;
    const int *bc;
    const bool ic_in_shell;
    ~FloorAfter() {
      if (!par || !par->floor_ghosts) return;
      // only a condition that computes values can leave something below a floor, and only in the block it fills
      // (copies, restrictions and limited prolongations of floored zones are floored): those blocks, batched
      const long n = static_cast<long>(P.ni) * P.nj * P.nk;
      BlockList bl;
      bl.n = 0;
      auto flush = [&]() {
        if (bl.n == 0) return;
        hipLaunchKernelGGL(floor_ghost_kernel, dim3((n + 255) / 256, bl.n), dim3(256), 0, s, fill_tabs(P, bl.b[0]), P, bl);
        bl.n = 0;
      };
      for (int b = 0; b < P.nb; ++b) {
        bool value = false;
        for (int f = 0; f < 2 * P.ndim; ++f) // (`ic` zones are floored where the one-launch fill writes them)
          value = value || (bc[b * 6 + f] >= ARTEMIS_BC_CONDUCTIVE && !(ic_in_shell && bc[b * 6 + f] == ARTEMIS_BC_IC)) ||
                  bc[b * 6 + f] == ARTEMIS_BC_STRAT_EXTRAP;
        if (!value) continue;
        bl.b[bl.n++] = b;
        if (bl.n == FACE_BATCH) flush();
      }
      flush();
    }
  } floor_after{P, par, s, bc, ic_in_shell};
  ShellArgs a;
  a.lo[0] = P.is, a.lo[1] = P.js, a.lo[2] = P.ks, a.hi[0] = P.ie, a.hi[1] = P.je, a.hi[2] = P.ke;
  a.ext[0] = P.ni, a.ext[1] = P.nj, a.ext[2] = P.nk;
  a.ng = P.ng, a.ndim = P.ndim, a.nfill = 5 * P.gas.ns + 4 * P.dust.ns;
  a.ic_gas = ic_in_shell ? par->ic_gas : nullptr, a.ic_dust = ic_in_shell ? par->ic_dust : nullptr;
  a.g_dfloor = P.gas.dfloor, a.g_siefloor = P.gas.siefloor, a.d_dfloor = P.dust.dfloor;
  a.floor_ic = (par && par->floor_ghosts) ? 1 : 0;
  const long nz = P.ke - P.ks + 1, ny = P.je - P.js + 1;
  a.nA = (P.ndim > 2) ? 2L * P.ng * P.nj * P.ni : 0;
  a.nB = (P.ndim > 1) ? nz * 2L * P.ng * P.ni : 0;
  a.nC = nz * ny * 2L * P.ng;
  if (par && (par->x1_interior_done & 3) == 3) { // the caller's stage kernel does not read the x1 ghost columns of active rows
    bool user = false;
    for (int b = 0; b < P.nb && !user; ++b)
      for (int f = 0; f < 2 * P.ndim; ++f) user = user || bc[b * 6 + f] >= ARTEMIS_BC_STRAT_EXTRAP;
    if (!user) a.nC = 0;
  }
  const long n = a.nA + a.nB + a.nC;
  if (n >= (1L << 31)) return 3; // (a block with 2^31 shell zones)
  ShellBatch batch;
  int nq = 0;
  std::vector<int> user_blocks; // blocks with a user condition: per-face launches, batched over the blocks
  auto flush = [&]() {
    if (nq == 0) return;
    if (n == 0) { // (1-D blocks whose only shell region was left to the caller)
      nq = 0;
      return;
    }
    for (int f = 0; f < 6; ++f) a.bc[f] = ARTEMIS_BC_NONE; // (the kernel takes the flags from the batch)
    hipLaunchKernelGGL(bc_shell_kernel, dim3((n + 256 * SHELL_ZONES - 1) / (256 * SHELL_ZONES), nq), dim3(256), 0, s, a, fill_tabs(P, 0), batch);
    nq = 0;
  };
  for (int b = 0; b < P.nb; ++b) {
    int fl[6];
    bool any = false, user = false;
    for (int f = 0; f < 6; ++f) {
      fl[f] = (f / 2 < P.ndim) ? bc[b * 6 + f] : ARTEMIS_BC_NONE;
      any = any || (fl[f] != ARTEMIS_BC_NONE);
      user = user || fl[f] == ARTEMIS_BC_STRAT_EXTRAP || fl[f] == ARTEMIS_BC_STRAT_INFLOW ||
             fl[f] == ARTEMIS_BC_CONDUCTIVE || (fl[f] == ARTEMIS_BC_IC && !ic_in_shell) || fl[f] == ARTEMIS_BC_DISK_EXTRAP ||
             fl[f] == ARTEMIS_BC_DISK_VISC;
    }
    if (!any) continue;
    if (user) {
      user_blocks.push_back(b);
      continue;
    }
    batch.blk[nq] = b;
    for (int f = 0; f < 6; ++f) batch.bc[nq][f] = static_cast<unsigned char>(fl[f]);
    if (++nq == BC_BATCH) flush();
  }
  flush();
  launch_bc_sequential(P, user_blocks, bc, par, s);
  return 0;
}

// extended: the slab spans the ENTIRE extent (ghosts included) of the dimensions below d, so that
// exchanging x1, then x2, then x3 slabs carries edge and corner zones along (needed by the
// viscous cross-derivatives, momentum_diffusion.hpp:95-141)
static void halo_args(const PackView &P, int face, int unpack, HaloArgs &a, int extended = 0) {
  const int d = face / 2, side = face % 2;
  a.d = d, a.side = side, a.ng = P.ng;
  const int st[3] = {P.is, P.js, P.ks}, en[3] = {P.ie, P.je, P.ke}, ext[3] = {P.ni, P.nj, P.nk};
  for (int q = 0; q < 3; ++q) {
    a.lo[q] = st[q], a.n[q] = en[q] - st[q] + 1;
    if (extended && q < d) a.lo[q] = 0, a.n[q] = ext[q];
  }
  a.n[d] = P.ng;
  if (!unpack) a.lo[d] = (side == 0) ? st[d] : en[d] - P.ng + 1; // interior slab next to the face
  else a.lo[d] = (side == 0) ? st[d] - P.ng : en[d] + 1;         // ghost slab behind the face
}
long halo_count(const PackView &P, int face, int extended) {
  HaloArgs a;
  halo_args(P, face, 0, a, extended);
  return static_cast<long>(a.n[0]) * a.n[1] * a.n[2] * (5 * P.gas.ns + 4 * P.dust.ns);
}
int launch_halo(const PackView &P, int block, int face, double *buf, int unpack, int extended,
                hipStream_t s) {
  HaloArgs a;
  halo_args(P, face, unpack, a, extended);
  const FillTabs t = fill_tabs(P, block);
  a.nfill = 5 * P.gas.ns + 4 * P.dust.ns;
  const long ncell = static_cast<long>(a.n[0]) * a.n[1] * a.n[2];
  hipLaunchKernelGGL(halo_kernel, dim3((ncell + 255) / 256), dim3(256), 0, s, a, t, P.ni, P.nj, buf,
                     unpack);
  return 0;
}

// ---- PLM_G geometry table (artemis_hip_plm_table_fill; layout: pack_view.hpp, geometry.hpp plm_geo_tab) ---------
namespace {
__global__ __launch_bounds__(256) void plm_table_kernel(const PackView P, double *tab) {
  const int L = P.plm_len;
  const long t = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<long>(P.nb) * 3 * L) return;
  const int idx = static_cast<int>(t % L), d = static_cast<int>((t / L) % 3), b = static_cast<int>(t / (3L * L));
  const int n = (d == 0) ? P.ni : ((d == 1) ? P.nj : P.nk);
  double *row = tab + (static_cast<long>(b) * 3 + d) * PLM_TAB_ROWS * L + idx;
  double v[PLM_TAB_ROWS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (d < P.ndim && idx >= 1 && idx <= n - 2) { // (the record reads the centroids of idx - 1 and idx + 1)
    const PlmGeo g = plm_geo(P, b, d + 1, (d == 2) ? idx : 0, (d == 1) ? idx : 0, (d == 0) ? idx : 0);
    v[0] = g.cr, v[1] = g.cl, v[2] = g.up, v[3] = g.lo, v[4] = g.ra.b, v[5] = g.ra.y, v[6] = g.rb.b, v[7] = g.rb.y;
  }
  if (d == 0 && idx < n) v[8] = make_coords(P, b, 0, 0, idx).x1v();
  for (int q = 0; q < PLM_TAB_ROWS; ++q) row[q * L] = v[q];
}
} // namespace
long plm_table_count(const PackView &P) { return static_cast<long>(P.nb) * 3 * PLM_TAB_ROWS * P.plm_len; }
void launch_plm_table_fill(const PackView &P, double *tab, hipStream_t s) {
  PackView Q = P;
  Q.plm_tab = nullptr; // (the fill evaluates the functions themselves)
  const long n = static_cast<long>(P.nb) * 3 * P.plm_len;
  hipLaunchKernelGGL(plm_table_kernel, dim3((n + 255) / 256), dim3(256), 0, s, Q, tab);
}

} // namespace artemis
