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
#include "device_math.hpp"
#include "geometry.hpp"
#include "kernels.hpp"
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

} // namespace artemis
