// Fused RK stage for gas (one species) on CARTESIAN 3-D blocks with PPM4 reconstruction, HLLC / HLLE / LLF:
//   CalculateFluxes (ppm.hpp:33-66) -> ApplyUpdate -> FluxSource -> SetAuxillaryFields -> ConsToPrim
//   (-> EstimateTimestepMesh)
// (artemis_driver.cpp:182-255 with every optional package off) in ONE pass: variant 4 of artemis_hip_stage_general.
// The caller has filled every ghost zone (the general stage's plain contract); the pressure slot of the output is not
// written, exactly like the cell-centred kernel (variant 0) this march replaces for such packs.
//
// Shape: the 2.5-D tile march of kernels_fused.hip / kernels_curv.hip with the stencil radius of PPM; what the marches
// have in common is in march_device.hpp.
//   * a 256-thread workgroup owns a 32 x 8 column of zones and marches along x3 through a chunk of planes;
//   * x3 in registers: a thread keeps its own column's planes k-1 .. k+2, fetches plane k+3 at the top of a trip, forms
//     the two x3 face values of zone k+1 from those five and carries the upper one to the next trip, so every x3 face
//     is reconstructed and solved once;
//   * x1 / x2 through an LDS tile of plane k with HALO 3 (face i0 needs the upper value of zone i0-1, whose stencil
//     reaches i0-3; face i0+32 the lower value of zone i0+32, whose stencil reaches i0+34).  No corner zones: the halo is
//     2*3*8 + 2*3*32 = 240 zones, one per thread.  x1 neighbours exchange their face value and their face flux with DPP
//     wave shifts (fused_device.hpp lane_below / lane_above); only the tile's edge columns go through small LDS
//     arrays.  That is what makes halo 3 fit at two workgroups per CU: 79.75 KB of LDS with the two register parks
//     (S.ZL, S.WM) that keep the kernel at 256 registers without scratch;
//   * every face value and every Riemann problem inside a tile is computed once; the tile's perimeter (the halo zones'
//     face values, one extra face per row and column) is spare-wave duty, rotating over the waves with k;
//   * two barriers per plane: face values | Riemann problems + staging of the next plane.
// The divisions by 12 of PPM4 share one refined reciprocal (device_math.hpp ppm4_fast); that form and the solvers'
// hand-scheduled divisions give the bits of `/` only while no tiny-but-nonzero velocity is in reach (DESIGN.md
// section 4), so a staged plane that holds one (halo included) takes ppm4 and the IEEE solvers for its x1 / x2 sweeps --
// workgroup-uniform, per plane, in this kernel -- and the x3 sweep does the same, per wave, when one of the six planes
// k-2 .. k+3 of the wave's own columns holds one.  Same expression trees as the cell-centred kernel, fluxes summed in
// ApplyUpdate's order: bit-identical (tests/test_parity_ppm_march.py).
#include <algorithm>
#include <cfloat>
#include <type_traits>

#include "device_math.hpp"
#include "fused_device.hpp"
#include "geometry.hpp"
#include "kernels.hpp"
#include "march_device.hpp"
#include "options.hpp"
#include "pack_view.hpp"
#include "sources_device.hpp"

namespace artemis {
namespace {
using namespace fused;

constexpr int FTX = 32, FTY = 8, FH = 3; // tile and halo
constexpr int QX = FTX + 2 * FH, QY = FTY + 2 * FH;
constexpr int PKMAX = 64; // planes per chunk at most

struct PpmK {
  double gam0, gam1, beta_dt, bdt, cfl;
  const double *bdt_ptr; // optional device scalar beta*dt (replaces beta_dt and bdt)
  double *const *prim_in, *const *prim_u1, *const *prim_out;
  unsigned long long *dt_bits;
  int has_u1;
  int nti, ntj, nchunk, kchunk;
};

// Workgroup constants the update reads on every plane: in LDS rather than in scalar registers for the whole march
// (kernels_curv.hip CurvConst)
struct PpmConst {
  double gam0, gam1, beta_dt, bdt, cfl;
  double dfloor, siefloor, de_switch;
  double *out[6];
  const double *u1[5]; // rho, v1, v2, v3, sie of the start-of-step state
};

struct PpmTile {
  double Q[6][QY][QX];         // staged primitives of plane k (rho, v1, v2, v3, P, sie), halo 3 (no corners)
  double UPY[6][FTY + 1][FTX]; // upper x2-face value of rows j0-1 .. j0+FTY-1
  double LOY[6][FTX];          // lower x2-face value of row j0+FTY
  double UPX0[6][FTY];         // upper x1-face value of column i0-1      (perimeter duty -> lanes tx == 0)
  double UPXE[6][FTY];         // upper x1-face value of column i0+FTX-1  (lanes tx == FTX-1 -> perimeter duty)
  double LOXE[6][FTY];         // lower x1-face value of column i0+FTX    (perimeter duty)
  double FY[8][FTY][FTX];      // x2 faces j0+1 .. j0+FTY (upper faces of the tile's rows)
  double FXE[8][FTY];          // x1 face i0+FTX (perimeter duty -> lanes tx == FTX-1)
  double ZL[6][256];           // the zone's upper x3 face value, parked between two x3 sweeps (12 VGPRs less through a plane)
  double WM[5][256];           // the own column's plane k-1 (the x3 sweep alone reads it), parked through the plane's phases
  double wmin[4];
  int tiny[2];                 // plane (k & 1) holds a tiny-but-nonzero velocity: its sweeps take the IEEE divisions
  PpmConst C;
};
static_assert(sizeof(PpmTile) <= 80 * 1024, "two workgroups per CU (160 KiB of LDS)");

// the two face values of a zone from its five-zone stencil: shared-reciprocal PPM4 (FAST) or ppm4 as it stands
template <bool FAST>
ADEV void faces5(double qmm, double qm, double q, double qp, double qpp, const Recip &r12, double &up, double &lo) {
  if constexpr (FAST) ppm4_fast(qmm, qm, q, qp, qpp, r12, up, lo);
  else ppm4(qmm, qm, q, qp, qpp, up, lo);
}

template <int RIEMANN>
__global__ __launch_bounds__(256, 2) void stage_ppm_kernel(const PackView P, const PpmK a) {
  __shared__ PpmTile S;
  const int t = threadIdx.x, tx = t % FTX, ty = t / FTX;
  int id = xcd_dealt_id();
  const int ti = id % a.nti;
  id /= a.nti;
  const int tj = id % a.ntj;
  id /= a.ntj;
  const int chunk = id % a.nchunk, b = id / a.nchunk;
  const int i0 = P.is + ti * FTX, j0 = P.js + tj * FTY;
  const int i = i0 + tx, j = j0 + ty;
  const bool active = (i <= P.ie) && (j <= P.je);
  const int il = min(i, P.ni - 1), jl = min(j, P.nj - 1);
  const int k0 = P.ks + chunk * a.kchunk;
  const int k1 = min(P.ke, k0 + a.kchunk - 1);
  const double gm1 = P.gm1;
  const GasK gk = gas_constants(gm1);
  const Recip r12 = recip(12.0);
  if (t == 0) { // (read back after the barrier below)
    PpmConst c;
    c.gam0 = a.gam0, c.gam1 = a.gam1, c.beta_dt = a.beta_dt, c.bdt = a.bdt, c.cfl = a.cfl;
    if (a.bdt_ptr) c.beta_dt = c.bdt = *a.bdt_ptr;
    c.dfloor = P.gas.dfloor, c.siefloor = P.gas.siefloor, c.de_switch = P.gas.de_switch;
    for (int q = 0; q < 6; ++q) c.out[q] = a.prim_out[b * 6 + q];
    for (int q = 0; q < 4; ++q) c.u1[q] = a.prim_u1[b * 6 + q];
    c.u1[4] = a.prim_u1[b * 6 + 5];
    S.C = c;
    S.tiny[0] = S.tiny[1] = 0;
  }
  const double *g = P.geom + 6 * b;
  const double *in_r = a.prim_in[b * 6 + 0], *in_1 = a.prim_in[b * 6 + 1], *in_2 = a.prim_in[b * 6 + 2];
  const double *in_3 = a.prim_in[b * 6 + 3], *in_e = a.prim_in[b * 6 + 5];
  const unsigned sj = static_cast<unsigned>(P.sj), sk = static_cast<unsigned>(P.sk);
  const unsigned col = static_cast<unsigned>(jl) * sj + static_cast<unsigned>(il);
  // halo duty: threads 0 .. 6 FTX - 1 stage the x2 halo rows (Q rows 0 .. 2, FTY+3 .. FTY+5), the next 6 FTY threads the
  // x1 halo columns (Q columns 0 .. 2, FTX+3 .. FTX+5); each owns one halo column for the whole march.  Indices beyond
  // the array (ragged tiles) are clamped: such zones feed only faces of zones outside the block, which store nothing.
  int hr = -1, hc = -1;
  if (t < 2 * FH * FTX) {
    const int rr = t / FTX;
    hr = (rr < FH) ? rr : FTY + rr, hc = (t % FTX) + FH;
  } else if (t < 2 * FH * FTX + 2 * FH * FTY) {
    const int u = t - 2 * FH * FTX, cc = u % (2 * FH);
    hr = u / (2 * FH) + FH, hc = (cc < FH) ? cc : FTX + cc;
  }
  const unsigned hcol = halo_column<FH>(hr, hc, i0, j0, P.ni, P.nj, sj, col);
  // cell widths (device_math.hpp cell_geom: the reference's BBox arithmetic); x1 / x2 are constants of the march
  const double dx1 = (g[0] + (i + 1) * g[1]) - (g[0] + i * g[1]);
  const double dx2 = (g[2] + (j + 1) * g[3]) - (g[2] + j * g[3]);
  const double g4 = g[4], g5 = g[5];
  __syncthreads();

  auto stage_plane = [&](const Cell6 &q, const Raw5 &hal, int par) {
    S.Q[0][ty + FH][tx + FH] = q.d, S.Q[1][ty + FH][tx + FH] = q.v1, S.Q[2][ty + FH][tx + FH] = q.v2;
    S.Q[3][ty + FH][tx + FH] = q.v3, S.Q[4][ty + FH][tx + FH] = q.p, S.Q[5][ty + FH][tx + FH] = q.e;
    bool tn = tiny_vel3(q.v1, q.v2, q.v3);
    if (hr >= 0) {
      const Cell6 h = finish_cell(hal, gm1);
      S.Q[0][hr][hc] = h.d, S.Q[1][hr][hc] = h.v1, S.Q[2][hr][hc] = h.v2;
      S.Q[3][hr][hc] = h.v3, S.Q[4][hr][hc] = h.p, S.Q[5][hr][hc] = h.e;
      tn = tn || tiny_vel3(h.v1, h.v2, h.v3);
    }
    if (__any(tn) && (t & 63) == 0) S.tiny[par] = 1;
  };

  // ---- one plane, phases 1 and 2: the x1 / x2 sweeps (two barriers).  Plane k's primitives are staged; leaves the fluxes
  // through the zone's lower x1 / x2 faces in fx_lo / fy_lo and the tile's other face fluxes in S.FY / S.FXE.
  // FT: the plane holds no tiny-but-nonzero velocity (workgroup-uniform).
  auto phase12 = [&](auto FT, const int k, const bool stage_next, const Cell6 &qn, const Raw5 &hal_next, Flux8 &fx_lo,
                     Flux8 &fy_lo) {
    constexpr bool fastp = decltype(FT)::value;
    const int duty = (t + 64 * (k & 3)) & 255; // wave roles rotate with k
    if (duty >= 64) __builtin_amdgcn_s_setprio(2); // the duty waves first (kernels_fused.hip)
    // ---- P1: face values of the own zone; the tile's edge columns and rows on the duty waves
    Cell6 lox, loy, L;
#define SLX(m, n)                                                                                               \
  {                                                                                                             \
    const double *row_ = &S.Q[n][ty + FH][tx + FH];                                                             \
    double up_;                                                                                                 \
    faces5<fastp>(row_[-2], row_[-1], row_[0], row_[1], row_[2], r12, up_, lox.m);                              \
    L.m = lane_below(up_);                                                                                      \
    if (tx == FTX - 1) S.UPXE[n][ty] = up_;                                                                     \
  }
    FOR6_33(SLX)
#undef SLX
    __builtin_amdgcn_sched_barrier(0);
#define SLY(m, n)                                                                                               \
  {                                                                                                             \
    double up_;                                                                                                 \
    faces5<fastp>(S.Q[n][ty + FH - 2][tx + FH], S.Q[n][ty + FH - 1][tx + FH], S.Q[n][ty + FH][tx + FH],         \
                  S.Q[n][ty + FH + 1][tx + FH], S.Q[n][ty + FH + 2][tx + FH], r12, up_, loy.m);                 \
    S.UPY[n][ty + 1][tx] = up_;                                                                                 \
  }
    FOR6_33(SLY)
#undef SLY
    if (duty >= 128 && duty < 128 + 2 * FTY) { // columns i0-1 (upper value) and i0+FTX (lower value)
      const int u = duty - 128, row = u >> 1, side = u & 1;
      const int cx = side ? FTX + FH : FH - 1;
#pragma unroll
      for (int n = 0; n < 6; ++n) {
        const double *row_ = &S.Q[n][row + FH][cx];
        double up_, lo_;
        faces5<fastp>(row_[-2], row_[-1], row_[0], row_[1], row_[2], r12, up_, lo_);
        if (side) S.LOXE[n][row] = lo_;
        else S.UPX0[n][row] = up_;
      }
    }
    if (duty >= 192) { // rows j0-1 (upper value) and j0+FTY (lower value)
      const int u = duty - 192, cx = u % FTX, side = u / FTX;
      const int ry = side ? FTY + FH : FH - 1;
#pragma unroll
      for (int n = 0; n < 6; ++n) {
        double up_, lo_;
        faces5<fastp>(S.Q[n][ry - 2][cx + FH], S.Q[n][ry - 1][cx + FH], S.Q[n][ry][cx + FH], S.Q[n][ry + 1][cx + FH],
                      S.Q[n][ry + 2][cx + FH], r12, up_, lo_);
        if (side) S.LOY[n][cx] = lo_;
        else S.UPY[n][0][cx] = up_;
      }
    }
    __syncthreads();
    // ---- P2: S.Q is dead now: the next plane is staged into it first (its halo zone's registers are free before the
    // solvers need them); then the tile's upper perimeter on one duty wave -- ahead of the wave's own faces, whose two
    // results would otherwise sit in registers through a third solver pass (measured: scratch with HLLC) -- and the
    // Riemann problems at the own lower faces
    if (stage_next) stage_plane(qn, hal_next, (k + 1) & 1);
    __builtin_amdgcn_sched_barrier(0);
    if (duty >= 64 && duty < 128) { // lanes 0 .. FTY-1: x1 face i0+FTX per row; lanes 32 .. 63: x2 face j0+FTY
      // ONE Riemann pass for both kinds of face (kernels_fused.hip): the x2 lanes rotate their velocity components
      const int u = duty - 64;
      const bool isx = (u < FTY), isy = (u >= 32);
      if (isx || isy) {
        const int cx = u - 32;
        Cell6 l, r;
        if (isx) {
          GET6(6, l, S.UPXE, [u]);
          GET6(6, r, S.LOXE, [u]);
        } else {
          GET6(6, l, S.UPY, [FTY][cx]);
          GET6(6, r, S.LOY, [cx]);
          rotate_x2_in(l), rotate_x2_in(r);
        }
        Flux8 fe_ = solve_face<RIEMANN, 1>(gk, l, r, fastp);
        if (isx) {
          PUT8(6, S.FXE, fe_, [u]);
        } else {
          rotate_x2_out(fe_);
          PUT8(6, S.FY, fe_, [FTY - 1][cx]);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (tx == 0) { GET6(6, L, S.UPX0, [ty]); }
    fx_lo = solve_face<RIEMANN, 1>(gk, L, lox, fastp);
    GET6(6, L, S.UPY, [ty][tx]);
    fy_lo = solve_face<RIEMANN, 2>(gk, L, loy, fastp);
    if (ty > 0) { PUT8(6, S.FY, fy_lo, [ty - 1][tx]); }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  };
  auto plane12 = [&](const int k, const bool stage_next, const Cell6 &qn, const Raw5 &hal_next, Flux8 &fx_lo, Flux8 &fy_lo) {
    const bool fastp = (S.tiny[k & 1] == 0);
    if (t == 0) S.tiny[(k + 1) & 1] = 0; // set again when the next plane is staged (after the first barrier)
    if (fastp) phase12(std::true_type{}, k, stage_next, qn, hal_next, fx_lo, fy_lo);
    else phase12(std::false_type{}, k, stage_next, qn, hal_next, fx_lo, fy_lo);
  };
  // after the second barrier: the upper x1 / x2 faces from the neighbours
  auto upper12 = [&](const Flux8 &fx_lo, Flux8 &fx_hi, Flux8 &fy_hi) {
    flux_from_lane_above<6>(fx_lo, fx_hi);
    if (tx == FTX - 1) { GET8(6, fx_hi, S.FXE, [ty]); }
    GET8(6, fy_hi, S.FY, [ty][tx]);
  };

  // ---- the update of zone (k, j, i) from the folded sums (kernels_stage_cell.hip's gas branch on a Cartesian block)
  struct Sums {          // what ApplyUpdate and FluxSource sum over the faces, in their order of additions
    double dv[6];        // sum_d (A_d F_d- - A_d F_d+) of D, M1, M2, M3, E, e_int
    double tm[3], te[3]; // FluxSource: pressure-gradient term of M_d, P div v term of e_int, per direction
  };
  auto fold = [&](auto DTAG, Sums &s, const Flux8 &lo, const Flux8 &hi, double A, double dtdx, double dt_vol) {
    constexpr int D = decltype(DTAG)::value;
    const double t0 = (A * lo.d - A * hi.d), t1 = (A * lo.m1 - A * hi.m1), t2 = (A * lo.m2 - A * hi.m2);
    const double t3 = (A * lo.m3 - A * hi.m3), t4 = (A * lo.e - A * hi.e), t5 = (A * lo.eg - A * hi.eg);
    if constexpr (D == 1) s.dv[0] = t0, s.dv[1] = t1, s.dv[2] = t2, s.dv[3] = t3, s.dv[4] = t4, s.dv[5] = t5;
    else s.dv[0] += t0, s.dv[1] += t1, s.dv[2] += t2, s.dv[3] += t3, s.dv[4] += t4, s.dv[5] += t5;
    s.tm[D - 1] = dtdx * (lo.pf - hi.pf);
    s.te[D - 1] = dt_vol * 0.5 * (lo.pf + hi.pf) * (A * hi.vf - A * lo.vf);
  };
  double ldt = DBL_MAX;
  auto update = [&](const int k, const double vol, const double dx3, const Cell6 &qc, const Sums &s, const Raw5 &u1raw) {
    if (!active) return;
    const PpmConst &KC = S.C; // (LDS: every read below is a broadcast ds_read at its use)
    const unsigned c = col + static_cast<unsigned>(k) * sk;
    const double hx[3] = {1.0, 1.0, 1.0};
    GasCons u0 = prim_to_cons_gas(KC, qc.d, qc.v1, qc.v2, qc.v3, qc.e, hx);
    GasCons u1 = u0;
    if (a.has_u1) u1 = prim_to_cons_gas(KC, u1raw.d, u1raw.v1, u1raw.v2, u1raw.v3, u1raw.e, hx);
    // ---- ApplyUpdate (artemis_integrator.hpp:88-106)
    const Recip rvol = recip(vol);
    const double nd = s.dv[0] * KC.beta_dt, n1m = s.dv[1] * KC.beta_dt, n2m = s.dv[2] * KC.beta_dt, n3m = s.dv[3] * KC.beta_dt;
    const double ne = s.dv[4] * KC.beta_dt, neg = s.dv[5] * KC.beta_dt;
    // momenta can be tiny-but-nonzero ahead of a shock, where only IEEE division is right: wave-uniform choice
    double q1m, q2m, q3m;
    if (__any(tiny_nonzero(n1m) || tiny_nonzero(n2m) || tiny_nonzero(n3m))) {
      q1m = n1m / vol, q2m = n2m / vol, q3m = n3m / vol;
    } else {
      q1m = div(n1m, rvol), q2m = div(n2m, rvol), q3m = div(n3m, rvol);
    }
    u0.d = KC.gam0 * u0.d + KC.gam1 * u1.d + div(nd, rvol);
    u0.m1 = KC.gam0 * u0.m1 + KC.gam1 * u1.m1 + q1m;
    u0.m2 = KC.gam0 * u0.m2 + KC.gam1 * u1.m2 + q2m;
    u0.m3 = KC.gam0 * u0.m3 + KC.gam1 * u1.m3 + q3m;
    u0.e = KC.gam0 * u0.e + KC.gam1 * u1.e + div(ne, rvol);
    u0.eg = KC.gam0 * u0.eg + KC.gam1 * u1.eg + div(neg, rvol);
    // ---- FluxSource (fluid_fluxes.hpp:361-415)
    u0.m1 += s.tm[0];
    u0.eg -= s.te[0];
    u0.m2 += s.tm[1];
    u0.eg -= s.te[1];
    u0.m3 += s.tm[2];
    u0.eg -= s.te[2];
    // ---- SetAuxillaryFields (fill_derived.cpp:58-71) + ConsToPrim (:132-146); every scale factor is 1.  Not
    // the curvilinear marches' form (kernels_curv.hip update): with hx == 1 the two floored densities are one, so ONE
    // reciprocal serves all six divisions and there is no division by a scale factor -- another expression set
    const double w_d = (u0.d > KC.dfloor) ? u0.d : KC.dfloor;
    const Recip rwd = recip(w_d);
    const bool tiny_m = __any(tiny_nonzero(u0.m1) || tiny_nonzero(u0.m2) || tiny_nonzero(u0.m3));
    const double ke = div(0.5 * (sqr(u0.m1) + sqr(u0.m2) + sqr(u0.m3)), rwd);
    const double ue_cons = u0.e - ke;
    double sie = (ue_cons > KC.de_switch * u0.e) ? div(ue_cons, rwd) : div(u0.eg, rwd);
    sie = amax(sie, KC.siefloor);
    double u_u = sie * w_d;
    const double uflr = KC.siefloor * w_d;
    u_u = (u_u > uflr) ? u_u : uflr;
    double n1, n2, n3;
    if (tiny_m) n1 = u0.m1 / w_d, n2 = u0.m2 / w_d, n3 = u0.m3 / w_d;
    else n1 = div(u0.m1, rwd), n2 = div(u0.m2, rwd), n3 = div(u0.m3, rwd);
    double w_s = div(u_u, rwd);
    w_s = (w_s > KC.siefloor) ? w_s : KC.siefloor;
    gst(KC.out[0], c, w_d);
    gst(KC.out[1], c, n1);
    gst(KC.out[2], c, n2);
    gst(KC.out[3], c, n3);
    gst(KC.out[5], c, w_s); // (the pressure slot is not written: consumers recompute it, and variant 0 leaves it alone)
    if (a.dt_bits) { // Gas::EstimateTimestepMesh on the new state (gas.cpp:411-433)
      const double bulk = (gm1 + 1.0) * gm1 * w_d * w_s;
      const double cs = sqrt_pos(div(bulk, rwd));
      double denom = div(fabs(n1) + cs, dx1);
      denom += div(fabs(n2) + cs, dx2);
      denom += div(fabs(n3) + cs, dx3);
      ldt = amin(ldt, div(1.0, denom));
    }
  };

  // ---- the march ------------------------------------------------------------------------------------------------------
  auto ldraw = [&](unsigned c_) { return load_raw(in_r, in_1, in_2, in_3, in_e, c_); };
  auto tiny_r = [&](const Raw5 &q) { return tiny_vel3(q.v1, q.v2, q.v3); };
  // own column: planes k-1 .. k+2 of trip k in w0 (parked in S.WM) .. w3 (the first trip is k0-1: it only primes the x3 face k0)
  Raw5 w0 = ldraw(col + static_cast<unsigned>(k0 - 2) * sk), w1 = ldraw(col + static_cast<unsigned>(k0 - 1) * sk);
  Raw5 w2 = ldraw(col + static_cast<unsigned>(k0) * sk), w3 = ldraw(col + static_cast<unsigned>(k0 + 1) * sk);
  unsigned tb; // bit q: the own column's plane (newest staged) - q holds a tiny-but-nonzero velocity
  {            // upper x3 face value of zone k (ql of face k+1), carried from trip to trip in S.ZL
    Cell6 zl;
    const Raw5 wm = ldraw(col + static_cast<unsigned>(k0 - 3) * sk);
    const Cell6 c0 = finish_cell(wm, gm1), c1 = finish_cell(w0, gm1), c2 = finish_cell(w1, gm1), c3 = finish_cell(w2, gm1);
    const Cell6 c4 = finish_cell(w3, gm1);
    double unused_;
#define ZL0(m, n) ppm4(c0.m, c1.m, c2.m, c3.m, c4.m, zl.m, unused_);
    FOR6(ZL0)
#undef ZL0
#define ZPUT(m, n) S.ZL[n][t] = zl.m;
    FOR6(ZPUT)
    S.WM[0][t] = w0.d, S.WM[1][t] = w0.v1, S.WM[2][t] = w0.v2, S.WM[3][t] = w0.v3, S.WM[4][t] = w0.e;
    tb = (tiny_r(wm) ? 16u : 0u) | (tiny_r(w0) ? 8u : 0u) | (tiny_r(w1) ? 4u : 0u) | (tiny_r(w2) ? 2u : 0u) | (tiny_r(w3) ? 1u : 0u);
  }
  Flux8 fz_lo;
  fz_lo.d = fz_lo.m1 = fz_lo.m2 = fz_lo.m3 = fz_lo.e = fz_lo.eg = fz_lo.pf = fz_lo.vf = 0.0;
  Raw5 u1raw = w1;
  for (int k = k0 - 1; k <= k1; ++k) {
    // this trip's HBM loads first (unconditional: kernels_curv.hip); consumed after the plane's LDS phases
    const Raw5 w4 = ldraw(col + static_cast<unsigned>(k + 3) * sk);
    const Raw5 hal = ldraw(hcol + static_cast<unsigned>(min(k + 1, P.nk - 1)) * sk); // halo zone of plane k+1
    const bool live = k >= k0;
    const unsigned ck = col + static_cast<unsigned>(k) * sk;
    const double dx3 = (g4 + (k + 1) * g5) - (g4 + k * g5);
    const double vol = dx1 * dx2 * dx3; // geometry.hpp:199-225
    const double bdt = S.C.bdt;
    const double dt_vol = div(bdt, recip(vol));
    const Cell6 qc = finish_cell(w1, gm1);
    Sums s;
    if (live) {
      Flux8 fx_lo, fy_lo, fx_hi, fy_hi;
      plane12(k, k < k1, finish_cell(w2, gm1), hal, fx_lo, fy_lo);
      upper12(fx_lo, fx_hi, fy_hi);
      fold(std::integral_constant<int, 1>{}, s, fx_lo, fx_hi, dx2 * dx3, div(bdt, dx1), dt_vol);
      fold(std::integral_constant<int, 2>{}, s, fy_lo, fy_hi, dx1 * dx3, div(bdt, dx2), dt_vol);
    } else { // priming trip: stage the first plane
      stage_plane(finish_cell(w2, gm1), hal, k0 & 1);
      __syncthreads();
    }
    // what only the update reads is fetched here: the x3 sweep covers its latency (kernels_curv.hip)
    if (a.has_u1 && live) u1raw = load_raw(S.C.u1[0], S.C.u1[1], S.C.u1[2], S.C.u1[3], S.C.u1[4], ck);
    // x3 sweep, registers only: the face values of zone k+1 from planes k-1 .. k+3, then face k+1
    tb = (tb << 1) | (tiny_r(w4) ? 1u : 0u);
    const bool fast3 = !__any((tb & 63u) != 0u); // planes k-2 .. k+3 (the carried value's stencil reached k-2)
    Cell6 zr, zl;
    {
      Cell6 zl_next;
      Raw5 w0; // (written by this thread in the previous trip: no barrier needed)
      w0.d = S.WM[0][t], w0.v1 = S.WM[1][t], w0.v2 = S.WM[2][t], w0.v3 = S.WM[3][t], w0.e = S.WM[4][t];
      const Cell6 c0 = finish_cell(w0, gm1), c2 = finish_cell(w2, gm1), c3 = finish_cell(w3, gm1), c4 = finish_cell(w4, gm1);
      if (fast3) {
#define ZSL(m, n) ppm4_fast(c0.m, qc.m, c2.m, c3.m, c4.m, r12, zl_next.m, zr.m);
        FOR6_33(ZSL)
#undef ZSL
      } else {
#define ZSL(m, n) ppm4(c0.m, qc.m, c2.m, c3.m, c4.m, zl_next.m, zr.m);
        FOR6_33(ZSL)
#undef ZSL
      }
#define ZGET(m, n) zl.m = S.ZL[n][t]; // (written by this thread in the previous trip: no barrier needed)
      FOR6(ZGET)
#undef ZGET
      S.ZL[0][t] = zl_next.d, S.ZL[1][t] = zl_next.v1, S.ZL[2][t] = zl_next.v2;
      S.ZL[3][t] = zl_next.v3, S.ZL[4][t] = zl_next.p, S.ZL[5][t] = zl_next.e;
    }
    __builtin_amdgcn_sched_barrier(0);
    const Flux8 fz_hi = solve_face<RIEMANN, 3>(gk, zl, zr, fast3);
    __builtin_amdgcn_sched_barrier(0);
    if (live) {
      fold(std::integral_constant<int, 3>{}, s, fz_lo, fz_hi, dx1 * dx2, div(bdt, dx3), dt_vol);
      update(k, vol, dx3, qc, s, u1raw);
    }
    fz_lo = fz_hi;
    S.WM[0][t] = w1.d, S.WM[1][t] = w1.v1, S.WM[2][t] = w1.v2, S.WM[3][t] = w1.v3, S.WM[4][t] = w1.e;
    w1 = w2, w2 = w3, w3 = w4;
  }
#undef ZPUT
  if (a.dt_bits) BLOCK_MIN_TO_DT(t, ldt, S.wmin, 4, S.C.cfl, a.dt_bits)
}
} // namespace

// Gas of a pack the stage plan sends here: the whole stage, timestep limit included
void launch_stage_ppm(const PackView &P, const artemis_stage_general_args_t &g, int riemann, hipStream_t s) {
  PpmK k;
  k.gam0 = g.gam0, k.gam1 = g.gam1, k.beta_dt = g.beta_dt, k.bdt = g.bdt, k.cfl = g.cfl_gas;
  k.bdt_ptr = g.beta_dt_dev;
  k.prim_in = g.gas_in, k.prim_u1 = g.gas_u1, k.prim_out = g.gas_out;
  k.dt_bits = reinterpret_cast<unsigned long long *>(g.dt_dev);
  k.has_u1 = (k.prim_u1 != k.prim_in) ? 1 : 0;
  const int nx = P.ie - P.is + 1, ny = P.je - P.js + 1, nz = P.ke - P.ks + 1;
  k.nti = (nx + FTX - 1) / FTX, k.ntj = (ny + FTY - 1) / FTY;
  const long tiles = static_cast<long>(k.nti) * k.ntj * P.nb;
  // chunks along x3 (one priming trip each): long ones, but enough workgroups for the chip's 512 slots (kernels.hpp)
  int nch = pick_march_chunks(nz, tiles, 512, PKMAX, 0.6);
  // tuning knob (1 .. PKMAX planes: a chunk of any length finds its stencil, planes k0 - 3 .. k1 + 3, inside the block's
  // nghost >= 3 planes)
  if (opt(OPT_PPM_KCHUNK) > 0) nch = (nz + knob_chunk(opt(OPT_PPM_KCHUNK), PKMAX) - 1) / knob_chunk(opt(OPT_PPM_KCHUNK), PKMAX);
  k.kchunk = (nz + nch - 1) / nch;
  k.nchunk = (nz + k.kchunk - 1) / k.kchunk;
  const unsigned grid = static_cast<unsigned>(tiles * k.nchunk);
  note_cut(ARTEMIS_CUT_STAGE_PPM, k.kchunk, k.nchunk, grid);
  if (riemann == ARTEMIS_HLLC) hipLaunchKernelGGL((stage_ppm_kernel<0>), dim3(grid), dim3(256), 0, s, P, k);
  else if (riemann == ARTEMIS_HLLE) hipLaunchKernelGGL((stage_ppm_kernel<1>), dim3(grid), dim3(256), 0, s, P, k);
  else hipLaunchKernelGGL((stage_ppm_kernel<2>), dim3(grid), dim3(256), 0, s, P, k);
}

} // namespace artemis
