// History integrals (utils/history.hpp:29-100; gas.cpp:648-676, dust.cpp:332-352) straight from the primitives: the
// volume integrals of the conserved variables over the interior zones of a pack, without a conserved array being read or
// written.  Every zone's conserved value is formed in registers with PrimToCons's own expressions and operation order
// (fill_derived.cpp:212-276, prim_to_cons_kernel in kernels_unfused.hip), so each term of a sum is the very double the
// host loop of artemis_sim_history multiplies; only the order of the additions differs.
//
// Two launches, no floating-point atomics and no last-block ticket:
//   1. history_partial_kernel: grid-stride over 64 x 4 tiles (lanes along x1) like estimate_dt_kernel, species outermost
//      (every species has its own arrays: nothing is read twice and 6 / 4 accumulators are live), shuffle reduction over
//      the wave, LDS over the four waves, one row of partial sums per workgroup in scratch[workgroup][quantity];
//   2. history_combine_kernel: one workgroup adds the rows in index order.
// The number of workgroups is a function of the pack's shape alone, so the result is the same bits from run to run and
// from device to device.
//
// The recorded form (artemis_hip_record_integrals, include/artemis_hip_record.h; at the end of this file) is the same
// two launches with the sums of up to seven index windows beside the whole pack's, written into the row a recorder's tick
// opened; artemis_hip_record_nbody adds the n-body accumulators to their host base into such a row.
#include "device_math.hpp"
#include "geometry.hpp"
#include "kernels.hpp"
#include "kernels_record.hpp"
#include "pack_view.hpp"
#include "task_device.hpp"

namespace artemis {

namespace {
constexpr int HTX = 64, HTY = 4;
constexpr long HIST_MAX_WG = 1024;

struct HistTiles {
  int gx, gy, nkr;
  long ntile;
};
inline HistTiles hist_tiles(const PackView &P) {
  HistTiles t;
  t.gx = (P.ie - P.is + HTX) / HTX, t.gy = (P.je - P.js + HTY) / HTY, t.nkr = P.ke - P.ks + 1;
  t.ntile = static_cast<long>(t.gx) * t.gy * t.nkr * P.nb;
  return t;
}

// sum over the workgroup of acc[0..NQ) -> scratch row entries [q0, q0 + NQ)
template <int NQ>
__device__ __forceinline__ void reduce_store(double (&acc)[NQ], double (*wsum)[6], double *row, int q0) {
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_down(acc[q], off, 64);
  const int lane = threadIdx.x, wave = threadIdx.y;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) wsum[wave][q] = acc[q];
  }
  __syncthreads();
  if (wave == 0 && lane < NQ) {
    double s = wsum[0][lane];
    for (int w = 1; w < HTY; ++w) s += wsum[w][lane];
    row[q0 + lane] = s;
  }
  __syncthreads(); // (wsum is reused by the next species)
}

template <bool CURV>
__global__ __launch_bounds__(HTX *HTY) void history_partial_kernel(const PackView P, const HistTiles T, double *scratch) {
  __shared__ double wsum[HTY][6];
  const int nsg = P.gas.ns, nsd = P.dust.ns;
  double *row = scratch + static_cast<long>(blockIdx.x) * (6 * nsg + 4 * nsd);
  for (int n = 0; n < nsg + nsd; ++n) {
    const bool gas = n < nsg;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long tile = blockIdx.x; tile < T.ntile; tile += gridDim.x) {
      const int i = P.is + static_cast<int>(tile % T.gx) * HTX + threadIdx.x;
      const int j = P.js + static_cast<int>((tile / T.gx) % T.gy) * HTY + threadIdx.y;
      const int bz = static_cast<int>(tile / (static_cast<long>(T.gx) * T.gy));
      const int b = bz / T.nkr;
      const int k = P.ks + bz % T.nkr;
      if (i > P.ie || j > P.je) continue;
      const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;
      double vol, hx[3] = {1.0, 1.0, 1.0}; // Coords::Volume (history.hpp:49-50), GetScaleFactors
      if constexpr (CURV) {
        const DCoords co = make_coords(P, b, k, j, i);
        vol = co.volume();
        hx[1] = co.hx2v(), hx[2] = co.hx3v();
      } else {
        const CellGeom g = cell_geom(P.geom + 6 * b, k, j, i);
        vol = g.dx1 * g.dx2 * g.dx3;
      }
      if (gas) {
        const FluidView &f = P.gas;
        const int nv = 6 * nsg;
        double w_d = f.prim[b * nv + n][c];
        w_d = (w_d > f.dfloor) ? w_d : f.dfloor;
        const double vel1 = f.prim[b * nv + nsg + 3 * n + 0][c];
        const double vel2 = f.prim[b * nv + nsg + 3 * n + 1][c];
        const double vel3 = f.prim[b * nv + nsg + 3 * n + 2][c];
        double w_s = f.prim[b * nv + 5 * nsg + n][c];
        w_s = (w_s > f.siefloor) ? w_s : f.siefloor;
        const double u_u = w_s * w_d;
        const double ke = 0.5 * w_d * (sqr(vel1) + sqr(vel2) + sqr(vel3));
        acc[0] += w_d * vol;
        acc[1] += (w_d * vel1 * hx[0]) * vol;
        acc[2] += (w_d * vel2 * hx[1]) * vol;
        acc[3] += (w_d * vel3 * hx[2]) * vol;
        acc[4] += (u_u + ke) * vol;
        acc[5] += u_u * vol;
      } else {
        const FluidView &f = P.dust;
        const int m = n - nsg, nv = 4 * nsd;
        double w_d = f.prim[b * nv + m][c];
        w_d = (w_d > f.dfloor) ? w_d : f.dfloor;
        acc[0] += w_d * vol;
        for (int d = 0; d < 3; ++d) acc[1 + d] += (w_d * f.prim[b * nv + nsd + 3 * m + d][c] * hx[d]) * vol;
      }
    }
    if (gas) {
      reduce_store<6>(acc, wsum, row, 6 * n);
    } else {
      double a4[4] = {acc[0], acc[1], acc[2], acc[3]};
      reduce_store<4>(a4, wsum, row, 6 * nsg + 4 * (n - nsg));
    }
  }
}

// rows [nrow][nq] -> sums[nq], rows added in index order
__global__ __launch_bounds__(64) void history_combine_kernel(const double *scratch, int nrow, int nq, double *sums) {
  for (int q = threadIdx.x; q < nq; q += blockDim.x) {
    double s = 0.0;
#pragma unroll 8
    for (int r = 0; r < nrow; ++r) s += scratch[static_cast<long>(r) * nq + q];
    sums[q] = s;
  }
}

// ---- recorded integrals (artemis_hip_record_integrals) -------------------------------------------------------------------
// history_partial_kernel with 1 + nwin sets of accumulators: set 0 takes every zone exactly as above -- the same tiles, the
// same terms in the same order, the same reduce_store -- so it holds the bits of artemis_hip_history_sums; set 1 + w takes
// the zones inside window w, zones[b][w] = {i0, i1, j0, j1, k0, k1}, half-open and interior-relative, and nothing else, so
// a window that holds every zone has the bits of set 0 and one that holds none stays +0.0.  Only integers are compared.
// What is the same for the whole workgroup is decided once per tile from scalar values: whether the tile meets a window at
// all (`live`; a tile outside every window costs the compares of that test and nothing per lane), and, over the tiles of
// the workgroup, whether any met window w (`hit`): the sums of a window the workgroup never met are stored as +0.0 without
// a reduction.  NW is the compile-time bucket of nwin (0, 1, 2, 4, 7): (1 + NW) * 6 doubles of accumulators in registers.
// The row index comes from the recorder's control block, a uniform load; nothing is launched differently for a cycle that
// is not due, the workgroups return at once.
template <bool CURV, int NW>
__global__ __launch_bounds__(HTX *HTY) void record_integrals_partial_kernel(const PackView P, const HistTiles T, const int *__restrict__ zones,
                                                                          int nwin, const artemis_record_ctl_t *__restrict__ ctl,
                                                                          long capacity, double *scratch) {
  const long long slot = ctl->slot; // workgroup-uniform
  if (slot < 0 || slot >= capacity) return;
  __shared__ double wsum[HTY][6];
  const int nsg = P.gas.ns, nsd = P.dust.ns, nq = 6 * nsg + 4 * nsd;
  double *row = scratch + static_cast<long>(blockIdx.x) * (1 + nwin) * nq;
  for (int n = 0; n < nsg + nsd; ++n) {
    const bool gas = n < nsg;
    double acc[1 + NW][6];
#pragma unroll
    for (int s = 0; s < 1 + NW; ++s)
#pragma unroll
      for (int q = 0; q < 6; ++q) acc[s][q] = 0.0;
    unsigned hit = 0u;
    for (long tile = blockIdx.x; tile < T.ntile; tile += gridDim.x) {
      const int ti = static_cast<int>(tile % T.gx) * HTX, tj = static_cast<int>((tile / T.gx) % T.gy) * HTY;
      const int bz = static_cast<int>(tile / (static_cast<long>(T.gx) * T.gy));
      const int b = bz / T.nkr, kr = bz % T.nkr;
      const int *z = zones + static_cast<long>(b) * nwin * 6;
      unsigned live = 0u; // windows this tile meets
#pragma unroll
      for (int w = 0; w < NW; ++w)
        if (w < nwin && z[6 * w] < ti + HTX && z[6 * w + 1] > ti && z[6 * w + 2] < tj + HTY && z[6 * w + 3] > tj && z[6 * w + 4] <= kr &&
            z[6 * w + 5] > kr)
          live |= 1u << w;
      hit |= live;
      const int ir = ti + static_cast<int>(threadIdx.x), jr = tj + static_cast<int>(threadIdx.y);
      const int i = P.is + ir, j = P.js + jr, k = P.ks + kr;
      if (i > P.ie || j > P.je) continue;
      const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;
      double vol, hx[3] = {1.0, 1.0, 1.0};
      if constexpr (CURV) {
        const DCoords co = make_coords(P, b, k, j, i);
        vol = co.volume();
        hx[1] = co.hx2v(), hx[2] = co.hx3v();
      } else {
        const CellGeom g = cell_geom(P.geom + 6 * b, k, j, i);
        vol = g.dx1 * g.dx2 * g.dx3;
      }
      double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // the zone's terms, the expressions of history_partial_kernel
      if (gas) {
        const FluidView &f = P.gas;
        const int nv = 6 * nsg;
        double w_d = f.prim[b * nv + n][c];
        w_d = (w_d > f.dfloor) ? w_d : f.dfloor;
        const double vel1 = f.prim[b * nv + nsg + 3 * n + 0][c];
        const double vel2 = f.prim[b * nv + nsg + 3 * n + 1][c];
        const double vel3 = f.prim[b * nv + nsg + 3 * n + 2][c];
        double w_s = f.prim[b * nv + 5 * nsg + n][c];
        w_s = (w_s > f.siefloor) ? w_s : f.siefloor;
        const double u_u = w_s * w_d;
        const double ke = 0.5 * w_d * (sqr(vel1) + sqr(vel2) + sqr(vel3));
        t[0] = w_d * vol;
        t[1] = (w_d * vel1 * hx[0]) * vol;
        t[2] = (w_d * vel2 * hx[1]) * vol;
        t[3] = (w_d * vel3 * hx[2]) * vol;
        t[4] = (u_u + ke) * vol;
        t[5] = u_u * vol;
      } else {
        const FluidView &f = P.dust;
        const int m = n - nsg, nv = 4 * nsd;
        double w_d = f.prim[b * nv + m][c];
        w_d = (w_d > f.dfloor) ? w_d : f.dfloor;
        t[0] = w_d * vol;
        for (int d = 0; d < 3; ++d) t[1 + d] = (w_d * f.prim[b * nv + nsd + 3 * m + d][c] * hx[d]) * vol;
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) acc[0][q] += t[q];
      if (live) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const bool in = ((live >> w) & 1u) && ir >= z[6 * w] && ir < z[6 * w + 1] && jr >= z[6 * w + 2] && jr < z[6 * w + 3];
#pragma unroll
          for (int q = 0; q < 6; ++q) acc[1 + w][q] = in ? acc[1 + w][q] + t[q] : acc[1 + w][q];
        }
      }
    }
    const int q0 = gas ? 6 * n : 6 * nsg + 4 * (n - nsg);
#pragma unroll
    for (int s = 0; s < 1 + NW; ++s) {
      if (s > nwin) break;
      double *rs = row + static_cast<long>(s) * nq;
      if (s == 0 || ((hit >> (s - 1)) & 1u)) {
        if (gas) {
          reduce_store<6>(acc[s], wsum, rs, q0);
        } else {
          double a4[4] = {acc[s][0], acc[s][1], acc[s][2], acc[s][3]};
          reduce_store<4>(a4, wsum, rs, q0);
        }
      } else if (threadIdx.y == 0 && static_cast<int>(threadIdx.x) < (gas ? 6 : 4)) {
        rs[q0 + threadIdx.x] = 0.0;
      }
    }
  }
}

// rows [nrow][ncol] of partial sums -> the opened row of the recorder, added in index order like history_combine_kernel
__global__ __launch_bounds__(64) void record_integrals_combine_kernel(const double *scratch, int nrow, int ncol,
                                                                     const artemis_record_ctl_t *__restrict__ ctl, long capacity, double *rows) {
  const long long slot = ctl->slot;
  if (slot < 0 || slot >= capacity) return;
  double *out = rows + slot * ncol;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < ncol; q += gridDim.x * blockDim.x) {
    double s = 0.0;
#pragma unroll 8
    for (int r = 0; r < nrow; ++r) s += scratch[static_cast<long>(r) * ncol + q];
    out[q] = s;
  }
}

// rows[slot][q] = base[q] + acc[q]: the one addition of the driver's flush_nbody_force, into the opened row
__global__ __launch_bounds__(64) void record_nbody_kernel(const double *__restrict__ base, const double *__restrict__ acc, long n,
                                                         const artemis_record_ctl_t *__restrict__ ctl, long capacity, double *rows) {
  const long long slot = ctl->slot;
  if (slot < 0 || slot >= capacity) return;
  double *out = rows + slot * n;
  for (long q = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x; q < n; q += static_cast<long>(gridDim.x) * blockDim.x)
    out[q] = base[q] + acc[q];
}

template <int NW>
void launch_record_partial(const PackView &P, const HistTiles &T, int nwg, const int *zones, int nwin, const artemis_record_ctl_t *ctl,
                           long capacity, double *scratch, hipStream_t s) {
  const dim3 t(HTX, HTY), g(static_cast<unsigned>(nwg));
  if (P.coords != ARTEMIS_CARTESIAN)
    hipLaunchKernelGGL((record_integrals_partial_kernel<true, NW>), g, t, 0, s, P, T, zones, nwin, ctl, capacity, scratch);
  else hipLaunchKernelGGL((record_integrals_partial_kernel<false, NW>), g, t, 0, s, P, T, zones, nwin, ctl, capacity, scratch);
}
} // namespace

long history_workgroups(const PackView &P) {
  const long ntile = hist_tiles(P).ntile;
  return grid_capped(ntile < HIST_MAX_WG ? ntile : HIST_MAX_WG); // (GRID_CAP: fewer rows of partial sums, other bits)
}

void launch_history_sums(const PackView &P, double *sums, double *scratch, hipStream_t s) {
  const HistTiles T = hist_tiles(P);
  const int nwg = static_cast<int>(history_workgroups(P)), nq = 6 * P.gas.ns + 4 * P.dust.ns;
  const dim3 t(HTX, HTY), g(static_cast<unsigned>(nwg));
  if (P.coords != ARTEMIS_CARTESIAN) hipLaunchKernelGGL((history_partial_kernel<true>), g, t, 0, s, P, T, scratch);
  else hipLaunchKernelGGL((history_partial_kernel<false>), g, t, 0, s, P, T, scratch);
  hipLaunchKernelGGL(history_combine_kernel, dim3(1), dim3(64), 0, s, scratch, nwg, nq, sums);
}

void launch_record_integrals(const PackView &P, int nwin, const int *zones, double *scratch, const void *ctl, long capacity, double *rows,
                             hipStream_t s) {
  const HistTiles T = hist_tiles(P);
  const int nwg = static_cast<int>(history_workgroups(P)), ncol = (1 + nwin) * (6 * P.gas.ns + 4 * P.dust.ns);
  const artemis_record_ctl_t *c = static_cast<const artemis_record_ctl_t *>(ctl);
  if (nwin == 0) launch_record_partial<0>(P, T, nwg, zones, nwin, c, capacity, scratch, s);
  else if (nwin == 1) launch_record_partial<1>(P, T, nwg, zones, nwin, c, capacity, scratch, s);
  else if (nwin == 2) launch_record_partial<2>(P, T, nwg, zones, nwin, c, capacity, scratch, s);
  else if (nwin <= 4) launch_record_partial<4>(P, T, nwg, zones, nwin, c, capacity, scratch, s);
  else launch_record_partial<RECORD_MAX_WINDOWS>(P, T, nwg, zones, nwin, c, capacity, scratch, s);
  hipLaunchKernelGGL(record_integrals_combine_kernel, dim3(static_cast<unsigned>((ncol + 63) / 64)), dim3(64), 0, s, scratch, nwg, ncol, c,
                     capacity, rows);
}

void launch_record_nbody(const double *base, const double *acc, long n, const void *ctl, long capacity, double *rows, hipStream_t s) {
  const long blocks = (n + 63) / 64;
  hipLaunchKernelGGL(record_nbody_kernel, dim3(static_cast<unsigned>(blocks < 64 ? blocks : 64)), dim3(64), 0, s, base, acc, n,
                     static_cast<const artemis_record_ctl_t *>(ctl), capacity, rows);
}

} // namespace artemis
