// Point sampling (artemis_hip_locate_points, artemis_hip_sample_fields; include/artemis_hip_sample.h has the definition): the
// block and zone that hold each of a list of points, and the requested variables of those zones, formed from the PRIMITIVES by
// the functions artemis_hip_pack_fields forms them with (fields_device.hpp) -- the same doubles, stored as out[c * npoints + p].
//
// Both kernels: one point per lane, grid-stride, no LDS, no atomics, 64-bit offsets.
//   locate   the search of locate_table.hpp: a cell index, the containment tests of that cell's blocks (one on a tiling tree)
//            and a face search that starts from the quotient -- double compares only.  Reads 24 bytes and stores 16 a point.
//   sample   an element-granular gather: lane t serves point order[t] (the caller's sort by block and zone, so neighbouring
//            lanes read neighbouring zones and a slice reads whole rows) and stores to that point's place.  Bound by the
//            latency of its loads, not by bandwidth: nothing here is tiled.  A thread loads the primitives of one species once
//            and forms every requested component of that species, as put_zone of kernels_fields.hip does; the selection is
//            wave-uniform, the block is not (the pointer tables are read per lane).  The derived codes are the DERIVED = true
//            instantiations, launched only for a selection that names one: a request without them never pays for the stencil.
// A location outside the pack and an order entry outside the list are treated as not found / skipped, so a bad list cannot make
// a lane read or write outside the pack's arrays or the output.
#include <cmath>

#include "device_math.hpp"
#include "fields_device.hpp"
#include "geometry.hpp"
#include "kernels.hpp"
#include "kernels_sample.hpp"
#include "locate_table.hpp"
#include "pack_view.hpp"
#include "task_device.hpp"

namespace artemis {

namespace {
constexpr int STX = 256;
constexpr long SAMPLE_MAX_WG = 2048; // 256 CUs x 8 workgroups; the rest of the points by grid stride

struct LocateArgs {
  int nb, nx[3], ng;
  double closed_hi[3];
};

__global__ __launch_bounds__(STX) void locate_points_kernel(const void *table, const double *geom, const LocateArgs A, long npoints,
                                                           const double *points, int4 *loc) {
  for (long p = static_cast<long>(blockIdx.x) * STX + threadIdx.x; p < npoints; p += static_cast<long>(gridDim.x) * STX) {
    const double x[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
    int l[4];
    artemis_locate::locate_point(table, geom, A.nb, A.nx, A.ng, A.closed_hi, x, l);
    loc[p] = make_int4(l[0], l[1], l[2], l[3]);
  }
}

// every requested plain component of zone (k, j, i) of block b, component c at o[c * npoints]: put_zone of kernels_fields.hip
template <bool CURV, class OUT>
__device__ __forceinline__ void put_point(const PackView &P, const FieldSelection &S, int b, int k, int j, int i, OUT *o, long npoints) {
  const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;
  double hx[3];
  scale_factors<CURV>(P, b, k, j, i, hx);
  for (int n = 0; n < (S.want_gas ? P.gas.ns : 0); ++n) {
    const GasZone g = load_gas(P, b, n, c);
    for (int e = 0; e < S.nsel; ++e) {
      const long at = S.comp0[e] * npoints;
      gas_components(g, P.gm1, hx, S.code[e], [&](int w, int d, double v) { put(o, at + (w * n + d) * npoints, v); });
    }
  }
  for (int m = 0; m < (S.want_dust ? P.dust.ns : 0); ++m) {
    const DustZone g = load_dust(P, b, m, c);
    for (int e = 0; e < S.nsel; ++e) {
      const long at = S.comp0[e] * npoints;
      dust_components(g, hx, S.code[e], [&](int w, int d, double v) { put(o, at + (w * m + d) * npoints, v); });
    }
  }
}
// ... and its derived components: put_zone_derived
template <bool CURV, class OUT>
__device__ __forceinline__ void put_point_derived(const PackView &P, const FieldSelection &S, int b, int k, int j, int i, OUT *o, long npoints) {
  for (int n = 0; n < (S.want_gas ? P.gas.ns : 0); ++n) {
    const DerivedZone z = load_derived<CURV, true>(P, b, n, k, j, i);
    for (int e = 0; e < S.nsel; ++e) {
      const long at = S.comp0[e] * npoints;
      derived_components<true>(z, S.code[e], [&](int w, int d, double v) { put(o, at + (w * n + d) * npoints, v); });
    }
  }
  for (int m = 0; m < (S.want_dust ? P.dust.ns : 0); ++m) {
    const DerivedZone z = load_derived<CURV, false>(P, b, m, k, j, i);
    for (int e = 0; e < S.nsel; ++e) {
      const long at = S.comp0[e] * npoints;
      derived_components<false>(z, S.code[e], [&](int w, int d, double v) { put(o, at + (w * m + d) * npoints, v); });
    }
  }
}
// NaN in every component this pass owns: a point that is not found
template <bool DERIVED, class OUT>
__device__ __forceinline__ void put_missing(const PackView &P, const FieldSelection &S, OUT *o, long npoints) {
  for (int e = 0; e < S.nsel; ++e) {
    const int code = S.code[e];
    const bool derived = code >= ARTEMIS_VAR_DERIVED0;
    if (derived != DERIVED) continue;
    const bool dust = derived ? code >= ARTEMIS_VAR_DUST_DERIVED_DIVERGENCE : code >= ARTEMIS_VAR_DUST_PRIM_DENSITY;
    const bool vec = code == ARTEMIS_VAR_GAS_PRIM_VELOCITY || code == ARTEMIS_VAR_GAS_CONS_MOMENTUM || code == ARTEMIS_VAR_DUST_PRIM_VELOCITY ||
                     code == ARTEMIS_VAR_DUST_CONS_MOMENTUM || code == ARTEMIS_VAR_GAS_DERIVED_VORTICITY || code == ARTEMIS_VAR_DUST_DERIVED_VORTICITY;
    const int ncomp = (vec ? 3 : 1) * (dust ? P.dust.ns : P.gas.ns);
    for (int q = 0; q < ncomp; ++q) put(o, (S.comp0[e] + q) * npoints, __builtin_nan(""));
  }
}

// (DERIVED: the derived pass -- S.want_gas / S.want_dust then say which fluids' DERIVED codes the selection names)
template <bool CURV, class OUT, bool DERIVED>
__global__ __launch_bounds__(STX) void sample_fields_kernel(const PackView P, const FieldSelection S, long npoints, const int4 *loc,
                                                           const long *order, OUT *out) {
  const int nx1 = P.ie - P.is + 1, nx2 = P.je - P.js + 1, nx3 = P.ke - P.ks + 1;
  for (long t = static_cast<long>(blockIdx.x) * STX + threadIdx.x; t < npoints; t += static_cast<long>(gridDim.x) * STX) {
    const long p = order ? order[t] : t;
    if (p < 0 || p >= npoints) continue;
    const int4 l = loc[p]; // {block, k, j, i}
    OUT *o = out + p;
    const bool found = l.x >= 0 && l.x < P.nb && l.y >= 0 && l.y < nx3 && l.z >= 0 && l.z < nx2 && l.w >= 0 && l.w < nx1;
    if (!found) put_missing<DERIVED>(P, S, o, npoints);
    else if constexpr (DERIVED) put_point_derived<CURV>(P, S, l.x, P.ks + l.y, P.js + l.z, P.is + l.w, o, npoints);
    else put_point<CURV>(P, S, l.x, P.ks + l.y, P.js + l.z, P.is + l.w, o, npoints);
  }
}

unsigned sample_grid(long npoints) {
  const long own = (npoints + STX - 1) / STX;
  return static_cast<unsigned>(grid_capped(own < SAMPLE_MAX_WG ? own : SAMPLE_MAX_WG));
}

template <class OUT>
void launch_sample_passes(const PackView &P, long npoints, const int4 *loc, const long *order, const FieldPasses &X, OUT *o, hipStream_t s) {
  const dim3 t(STX), g(sample_grid(npoints));
  const bool curv = P.coords != ARTEMIS_CARTESIAN;
  if (X.has_plain) {
    if (curv) hipLaunchKernelGGL((sample_fields_kernel<true, OUT, false>), g, t, 0, s, P, X.plain, npoints, loc, order, o);
    else hipLaunchKernelGGL((sample_fields_kernel<false, OUT, false>), g, t, 0, s, P, X.plain, npoints, loc, order, o);
  }
  if (X.has_derived) {
    if (curv) hipLaunchKernelGGL((sample_fields_kernel<true, OUT, true>), g, t, 0, s, P, X.derived, npoints, loc, order, o);
    else hipLaunchKernelGGL((sample_fields_kernel<false, OUT, true>), g, t, 0, s, P, X.derived, npoints, loc, order, o);
  }
}
} // namespace

void launch_locate_points(const PackView &P, const void *table_dev, const double *closed_hi, long npoints, const double *points, int *loc,
                          hipStream_t s) {
  if (npoints <= 0) return;
  LocateArgs A;
  A.nb = P.nb, A.ng = P.ng;
  A.nx[0] = P.ie - P.is + 1, A.nx[1] = P.je - P.js + 1, A.nx[2] = P.ke - P.ks + 1;
  for (int d = 0; d < 3; ++d) A.closed_hi[d] = closed_hi[d];
  hipLaunchKernelGGL(locate_points_kernel, dim3(sample_grid(npoints)), dim3(STX), 0, s, table_dev, P.geom, A, npoints, points,
                     reinterpret_cast<int4 *>(loc));
}

void launch_sample_fields(const PackView &P, long npoints, const int *loc, const long *order, const FieldSelection &S, bool single, void *out,
                          hipStream_t s) {
  if (npoints <= 0 || S.ncomp == 0) return;
  const FieldPasses X = field_passes(S);
  const int4 *l = reinterpret_cast<const int4 *>(loc);
  if (single) launch_sample_passes(P, npoints, l, order, X, static_cast<float *>(out), s);
  else launch_sample_passes(P, npoints, l, order, X, static_cast<double *>(out), s);
}

// ---- recording inside the time loop (artemis_hip_record_tick, artemis_hip_record_samples) -------------------------------------
// What a replayed graph cannot take by value lives in the control block on the device: the tick (one thread) counts the cycle,
// decides whether it is due and opens the row; the sample kernels read the row index there -- a load from a kernel-argument
// address, the same for every lane: one scalar load per wave -- and are sample_fields_kernel otherwise, with the same
// put_point / put_point_derived / put_missing, so a row holds the bits artemis_hip_sample_fields stores.  Only the tick
// writes the control block; plain stores everywhere.
namespace {
__global__ __launch_bounds__(64) void record_tick_kernel(artemis_record_ctl_t *ctl, artemis_record_head_t *head, const double *tstate,
                                                        double time, double dt, long every, long capacity) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long seen = ++ctl->seen, cycle = ++ctl->cycle;
  long long slot = -1;
  if (seen % every == 0) {
    if (ctl->rows < capacity) slot = ctl->rows++;
    else ++ctl->dropped;
  }
  ctl->slot = slot;
  if (slot >= 0) {
    head[slot].cycle = cycle;
    head[slot].time = tstate ? tstate[0] : time;
    head[slot].dt = tstate ? tstate[1] : dt;
  }
}

template <bool CURV, class OUT, bool DERIVED>
__global__ __launch_bounds__(STX) void record_samples_kernel(const PackView P, const FieldSelection S, long npoints, const int4 *loc,
                                                            const long *order, const artemis_record_ctl_t *__restrict__ ctl, long capacity,
                                                            long row, OUT *rows) {
  const long long slot = ctl->slot; // wave-uniform
  if (slot < 0 || slot >= capacity) return;
  OUT *out = rows + slot * row;
  const int nx1 = P.ie - P.is + 1, nx2 = P.je - P.js + 1, nx3 = P.ke - P.ks + 1;
  for (long t = static_cast<long>(blockIdx.x) * STX + threadIdx.x; t < npoints; t += static_cast<long>(gridDim.x) * STX) {
    const long p = order ? order[t] : t;
    if (p < 0 || p >= npoints) continue;
    const int4 l = loc[p]; // {block, k, j, i}
    OUT *o = out + p;
    const bool found = l.x >= 0 && l.x < P.nb && l.y >= 0 && l.y < nx3 && l.z >= 0 && l.z < nx2 && l.w >= 0 && l.w < nx1;
    if (!found) put_missing<DERIVED>(P, S, o, npoints);
    else if constexpr (DERIVED) put_point_derived<CURV>(P, S, l.x, P.ks + l.y, P.js + l.z, P.is + l.w, o, npoints);
    else put_point<CURV>(P, S, l.x, P.ks + l.y, P.js + l.z, P.is + l.w, o, npoints);
  }
}

template <class OUT>
void launch_record_passes(const PackView &P, long npoints, const int4 *loc, const long *order, const FieldPasses &X,
                          const artemis_record_ctl_t *ctl, long capacity, long row, OUT *rows, hipStream_t s) {
  const dim3 t(STX), g(sample_grid(npoints));
  const bool curv = P.coords != ARTEMIS_CARTESIAN;
  if (X.has_plain) {
    if (curv) hipLaunchKernelGGL((record_samples_kernel<true, OUT, false>), g, t, 0, s, P, X.plain, npoints, loc, order, ctl, capacity, row, rows);
    else hipLaunchKernelGGL((record_samples_kernel<false, OUT, false>), g, t, 0, s, P, X.plain, npoints, loc, order, ctl, capacity, row, rows);
  }
  if (X.has_derived) {
    if (curv) hipLaunchKernelGGL((record_samples_kernel<true, OUT, true>), g, t, 0, s, P, X.derived, npoints, loc, order, ctl, capacity, row, rows);
    else hipLaunchKernelGGL((record_samples_kernel<false, OUT, true>), g, t, 0, s, P, X.derived, npoints, loc, order, ctl, capacity, row, rows);
  }
}
} // namespace

void launch_record_tick(void *ctl, void *head, const double *tstate, double time, double dt, long every, long capacity, hipStream_t s) {
  hipLaunchKernelGGL(record_tick_kernel, dim3(1), dim3(64), 0, s, static_cast<artemis_record_ctl_t *>(ctl),
                     static_cast<artemis_record_head_t *>(head), tstate, time, dt, every, capacity);
}

void launch_record_samples(const PackView &P, long npoints, const int *loc, const long *order, const FieldSelection &S, bool single,
                           const void *ctl, long capacity, void *rows, hipStream_t s) {
  if (npoints <= 0 || S.ncomp == 0) return;
  const FieldPasses X = field_passes(S);
  const int4 *l = reinterpret_cast<const int4 *>(loc);
  const artemis_record_ctl_t *c = static_cast<const artemis_record_ctl_t *>(ctl);
  const long row = static_cast<long>(S.ncomp) * npoints;
  if (single) launch_record_passes(P, npoints, l, order, X, c, capacity, row, static_cast<float *>(rows), s);
  else launch_record_passes(P, npoints, l, order, X, c, capacity, row, static_cast<double *>(rows), s);
}

} // namespace artemis
