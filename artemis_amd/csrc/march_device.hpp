// What the streaming tile marches share (kernels_fused.hip, kernels_curv.hip, kernels_ppm.hip; the viscous-source march
// of kernels_diffusion.hip takes the id remap): the field lists that move a cell's primitives and a face's fluxes in and
// out of LDS, the workgroup-id remap, the halo zone's column, the x2 rotation of the perimeter's Riemann pass, the
// timestep term of a finished zone and the workgroup's timestep reduction.  Functions are forced inline, and a piece is
// shared only where the march that calls it compiles to the assembly it had with the text in place.
#pragma once
#include <cfloat>

#include "device_math.hpp"
#include "fused_device.hpp"
#include "geometry.hpp"
#include "sources_device.hpp"

namespace artemis {
namespace fused {

// ---- field lists: X(member, index) over a Cell6; a Cell6 from / a Flux8 to and from arrays indexed [variable]<index...>.
// nv = 6: every field; nv = 4 (the dust march carries rho, v1, v2, v3): the pressure / energy slots of a cell and the
// energy / pressure-flux / face-velocity slots of a face flux are skipped.
#define FOR6(X) X(d, 0) X(v1, 1) X(v2, 2) X(v3, 3) X(p, 4) X(e, 5)
// ... with a scheduling fence after the third variable: three reconstruction chains interleave (six would need the
// registers of twelve more doubles)
#define FOR6_33(X) X(d, 0) X(v1, 1) X(v2, 2) __builtin_amdgcn_sched_barrier(0); X(v3, 3) X(p, 4) X(e, 5)
#define GET6(nv, dst, A, ...)                                                              \
  dst.d = A[0] __VA_ARGS__, dst.v1 = A[1] __VA_ARGS__, dst.v2 = A[2] __VA_ARGS__,          \
  dst.v3 = A[3] __VA_ARGS__;                                                               \
  if constexpr ((nv) > 4) dst.p = A[4] __VA_ARGS__, dst.e = A[5] __VA_ARGS__
#define PUT8(nv, A, fl, ...)                                                               \
  A[0] __VA_ARGS__ = fl.d, A[1] __VA_ARGS__ = fl.m1, A[2] __VA_ARGS__ = fl.m2,             \
  A[3] __VA_ARGS__ = fl.m3;                                                                \
  if constexpr ((nv) > 4)                                                                  \
  A[4] __VA_ARGS__ = fl.e, A[5] __VA_ARGS__ = fl.eg, A[6] __VA_ARGS__ = fl.pf, A[7] __VA_ARGS__ = fl.vf
#define GET8(nv, fl, A, ...)                                                               \
  fl.d = A[0] __VA_ARGS__, fl.m1 = A[1] __VA_ARGS__, fl.m2 = A[2] __VA_ARGS__,             \
  fl.m3 = A[3] __VA_ARGS__;                                                                \
  if constexpr ((nv) > 4)                                                                  \
  fl.e = A[4] __VA_ARGS__, fl.eg = A[5] __VA_ARGS__, fl.pf = A[6] __VA_ARGS__, fl.vf = A[7] __VA_ARGS__

// Workgroup ids are dealt round-robin over the 8 XCDs, each with its own L2: give every XCD one contiguous run of tiles
// (the halo columns and the 128-byte lines a row segment straddles are then fetched from HBM once, not once per XCD).
// A bijection of 0 .. gridDim.x - 1.  (The headline kernel keeps its own form: its shell workgroups keep the lowest ids.)
ADEV int xcd_dealt_id() {
  const int id = blockIdx.x;
  const int n = static_cast<int>(gridDim.x), q = n >> 3, rem = n & 7, xcd = id & 7;
  return xcd * q + min(xcd, rem) + (id >> 3);
}

// The column, as an offset within a plane, of the halo zone a thread stages for the whole march: (hr, hc) = the zone's row
// and column in the staged rectangle of a tile at (i0, j0) with halo FH, hr < 0: no duty, the thread's own column `col`.
// Indices beyond the array (ragged tiles) are clamped: such zones feed only faces of zones outside the block, which
// store nothing.  (Which thread stages which halo zone stays with each march: as a call, the assignment moved the
// assembly of the curvilinear march, and the headline kernel deals its x1 columns from thread 128.)
template <int FH>
ADEV unsigned halo_column(const int hr, const int hc, const int i0, const int j0, const int ni, const int nj,
                          const unsigned sj, const unsigned col) {
  unsigned hcol = col;
  if (hr >= 0) {
    const int gi = min(max(i0 - FH + hc, 0), ni - 1), gj = min(max(j0 - FH + hr, 0), nj - 1);
    hcol = static_cast<unsigned>(gj) * sj + static_cast<unsigned>(gi);
  }
  return hcol;
}

// A zone's upper x1 face flux: the lower face flux of the lane above (the tile's last column is overwritten by the caller)
template <int NV>
ADEV void flux_from_lane_above(const Flux8 &lo, Flux8 &hi) {
  hi.d = lane_above(lo.d), hi.m1 = lane_above(lo.m1), hi.m2 = lane_above(lo.m2);
  hi.m3 = lane_above(lo.m3);
  if constexpr (NV > 4) {
    hi.e = lane_above(lo.e), hi.eg = lane_above(lo.eg);
    hi.pf = lane_above(lo.pf), hi.vf = lane_above(lo.vf);
  }
}

// ONE Riemann pass for both kinds of perimeter face: the x2 lanes hand the direction-1 solver their states with the
// velocity components rotated (v2, v3, v1) -- what solve_face<.., 2> does internally (hllc.hpp:67-69) -- and rotate the
// momentum fluxes back: (normal, t1, t2) = (m2, m3, m1) of the block's frame.  Same bits.
ADEV void rotate_x2_in(Cell6 &q) {
  const double a_ = q.v1;
  q.v1 = q.v2, q.v2 = q.v3, q.v3 = a_;
}
ADEV void rotate_x2_out(Flux8 &f) {
  const double n_ = f.m1;
  f.m1 = f.m3, f.m3 = f.m2, f.m2 = n_;
}

// Gas::EstimateTimestepMesh on a finished zone (gas.cpp:411-433) of the marches that carry scale factors:
// 1 / sum_d (|v_d| + cs) / width_d over the active directions.  rwd: the reciprocal of w_d that ConsToPrim formed;
// CO: the zone's Coords (width1 .. width3).
template <class CO>
ADEV double zone_dt_term(const double w_d, const double n1, const double n2, const double n3, const double w_s, const Recip &rwd,
                         const double gm1, const CO &co, const bool multi_d, const bool three_d) {
  const double bulk = (gm1 + 1.0) * gm1 * w_d * w_s;
  const double cs = sqrt_pos(div(bulk, rwd));
  double denom = div(fabs(n1) + cs, co.width1());
  if (multi_d) denom += div(fabs(n2) + cs, co.width2());
  if (three_d) denom += div(fabs(n3) + cs, co.width3());
  return div(1.0, denom);
}

// The workgroup's smallest timestep term to the device's limit: *dt_bits = min(*dt_bits, cfl * min over the nw waves).
// A statement, not a function: inlined from a function the same text is laid out differently, and the assembly of the
// kernels around it moves.  t: the thread's index in the workgroup; wmin: nw doubles of LDS that nothing reads any more
// (the barrier in front makes that so); cfl and dt_bits are evaluated by the one lane that needs them.
#define BLOCK_MIN_TO_DT(t, ldt, wmin, nw, cfl, dt_bits)                                                            \
  {                                                                                                                \
    __syncthreads();                                                                                               \
    for (int off = 32; off > 0; off >>= 1) ldt = fmin(ldt, __shfl_down(ldt, off, 64));                             \
    if (((t) & 63) == 0) (wmin)[(t) >> 6] = ldt;                                                                   \
    __syncthreads();                                                                                               \
    if ((t) == 0) {                                                                                                \
      double m = (wmin)[0];                                                                                        \
      for (int w = 1; w < (nw); ++w) m = fmin(m, (wmin)[w]);                                                       \
      if (m < DBL_MAX) atomicMin(dt_bits, static_cast<unsigned long long>(__double_as_longlong((cfl) * m)));       \
    }                                                                                                              \
  }

} // namespace fused
} // namespace artemis
