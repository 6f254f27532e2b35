// Field output (artemis_hip_pack_fields): the requested variables of every interior zone of a range of blocks, formed from
// the PRIMITIVES and stored ghost-free in one contiguous buffer [block - block0][component][k][j][i], as double or
// narrowed to float.  Every value is the double PrimToCons (fill_derived.cpp:212-276, prim_to_cons_kernel in
// kernels_unfused.hip) would leave in that slot -- floors applied, P = max(0, (gamma-1) rho sie), M_d = rho v_d h_d,
// eint = rho sie, E = eint + rho v^2 / 2, same expressions and operation order -- without a conserved array or the stored
// pressure slot being read and without anything being written to the pack.
//
// A copy kernel: no LDS, no atomics.  Grid-stride over 64 x 4 tiles of (i, j) with lanes along x1, like the history sums:
// a wave reads 512 contiguous bytes of a row of every primitive it needs and stores 512 (double) or 256 (float)
// contiguous bytes per component.  One zone per lane: a row's interior starts nghost zones into the array and an output
// row nx1 * (row index) elements into the buffer, so neither side is 16-byte aligned in general (odd nghost, odd nx1) and a
// two-zone lane would need a scalar path next to the vector one; the reads, always 8 bytes a lane, are two thirds of the
// traffic of a float dump anyway.  A thread loads the primitives of one species once and forms every requested component
// of that species from them; the selection is wave-uniform, so the switch below does not diverge.
#include "device_math.hpp"
#include "geometry.hpp"
#include "kernels.hpp"
#include "pack_view.hpp"
#include "task_device.hpp"

namespace artemis {

namespace {
constexpr int FTX = 64, FTY = 4;
constexpr long FIELDS_MAX_WG = 2048; // 256 CUs x 8 workgroups; the rest of the tiles by grid stride

struct FieldTiles {
  int gx, gy, nkr;
  long ntile;
};

template <class OUT>
__device__ __forceinline__ void put(OUT *out, long at, double v) {
  out[at] = static_cast<OUT>(v); // (double -> float: round to nearest even, the correctly rounded narrowing)
}

template <bool CURV, class OUT>
__global__ __launch_bounds__(FTX *FTY) void pack_fields_kernel(const PackView P, const FieldTiles T, const FieldSelection S,
                                                              int block0, OUT *out) {
  const int nsg = P.gas.ns, nsd = P.dust.ns;
  const int nx1 = P.ie - P.is + 1, nx2 = P.je - P.js + 1;
  const long zones = static_cast<long>(nx1) * nx2 * T.nkr; // interior zones of one block = stride of a component
  for (long tile = blockIdx.x; tile < T.ntile; tile += gridDim.x) {
    const int i = P.is + static_cast<int>(tile % T.gx) * FTX + threadIdx.x;
    const int j = P.js + static_cast<int>((tile / T.gx) % T.gy) * FTY + threadIdx.y;
    const long bz = tile / (static_cast<long>(T.gx) * T.gy);
    const int lb = static_cast<int>(bz / T.nkr); // block of the range, [0, nblocks)
    const int b = block0 + lb;
    const int k = P.ks + static_cast<int>(bz % T.nkr);
    if (i > P.ie || j > P.je) continue;
    const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;
    const long z = (static_cast<long>(k - P.ks) * nx2 + (j - P.js)) * nx1 + (i - P.is);
    OUT *o = out + static_cast<long>(lb) * S.ncomp * zones + z;
    double hx[3];
    scale_factors<CURV>(P, b, k, j, i, hx);
    for (int n = 0; n < (S.want_gas ? nsg : 0); ++n) {
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
      for (int e = 0; e < S.nsel; ++e) {
        const long at = S.comp0[e] * zones;
        switch (S.code[e]) {
        case ARTEMIS_VAR_GAS_PRIM_DENSITY:
        case ARTEMIS_VAR_GAS_CONS_DENSITY: put(o, at + n * zones, w_d); break;
        case ARTEMIS_VAR_GAS_PRIM_VELOCITY:
          put(o, at + (3 * n + 0) * zones, vel1), put(o, at + (3 * n + 1) * zones, vel2), put(o, at + (3 * n + 2) * zones, vel3);
          break;
        case ARTEMIS_VAR_GAS_PRIM_PRESSURE: put(o, at + n * zones, amax(0.0, P.gm1 * w_d * w_s)); break;
        case ARTEMIS_VAR_GAS_PRIM_SIE: put(o, at + n * zones, w_s); break;
        case ARTEMIS_VAR_GAS_CONS_MOMENTUM:
          put(o, at + (3 * n + 0) * zones, w_d * vel1 * hx[0]);
          put(o, at + (3 * n + 1) * zones, w_d * vel2 * hx[1]);
          put(o, at + (3 * n + 2) * zones, w_d * vel3 * hx[2]);
          break;
        case ARTEMIS_VAR_GAS_CONS_TOTAL_ENERGY: put(o, at + n * zones, u_u + ke); break;
        case ARTEMIS_VAR_GAS_CONS_INTERNAL_ENERGY: put(o, at + n * zones, u_u); break;
        default: break;
        }
      }
    }
    for (int m = 0; m < (S.want_dust ? nsd : 0); ++m) {
      const FluidView &f = P.dust;
      const int nv = 4 * nsd;
      double w_d = f.prim[b * nv + m][c];
      w_d = (w_d > f.dfloor) ? w_d : f.dfloor;
      const double vel1 = f.prim[b * nv + nsd + 3 * m + 0][c];
      const double vel2 = f.prim[b * nv + nsd + 3 * m + 1][c];
      const double vel3 = f.prim[b * nv + nsd + 3 * m + 2][c];
      for (int e = 0; e < S.nsel; ++e) {
        const long at = S.comp0[e] * zones;
        switch (S.code[e]) {
        case ARTEMIS_VAR_DUST_PRIM_DENSITY:
        case ARTEMIS_VAR_DUST_CONS_DENSITY: put(o, at + m * zones, w_d); break;
        case ARTEMIS_VAR_DUST_PRIM_VELOCITY:
          put(o, at + (3 * m + 0) * zones, vel1), put(o, at + (3 * m + 1) * zones, vel2), put(o, at + (3 * m + 2) * zones, vel3);
          break;
        case ARTEMIS_VAR_DUST_CONS_MOMENTUM:
          put(o, at + (3 * m + 0) * zones, w_d * vel1 * hx[0]);
          put(o, at + (3 * m + 1) * zones, w_d * vel2 * hx[1]);
          put(o, at + (3 * m + 2) * zones, w_d * vel3 * hx[2]);
          break;
        default: break;
        }
      }
    }
  }
}
// The inverse (artemis_hip_unpack_fields): the same buffer read, the primitives of the interior zones written.  The
// selection names one complete form per fluid (fields_form.hpp); every value stored is the one PrimToCons would leave in
// its slot (rho and sie floored, velocities as given), so a PrimToCons behind it changes nothing in these slots.  The
// pressure slot, the conserved arrays and the ghost zones are not written.
//   primitive form   sie as given, or P / ((gamma-1) rho) with the floored rho: the product first, as the pack kernel
//                    forms (gamma-1) rho sie, then one correctly rounded division
//   conserved form   set_aux_kernel followed by cons_to_prim_kernel (kernels_unfused.hip) on the zone's inputs, same
//                    expressions and operation order, the internal-energy input 0 where the selection has none
// Same tiling as above; a wave reads 512 (double) or 256 (float) contiguous bytes per component and stores 512 per
// primitive.
template <class IN>
__device__ __forceinline__ double get(const IN *in, long at) {
  return static_cast<double>(in[at]); // (float -> double: exact)
}

template <bool CURV, class IN>
__global__ __launch_bounds__(FTX *FTY) void unpack_fields_kernel(const PackView P, const FieldTiles T, const FieldUnpack U,
                                                                int block0, const IN *in) {
  const int nsg = P.gas.ns, nsd = P.dust.ns;
  const int nx1 = P.ie - P.is + 1, nx2 = P.je - P.js + 1;
  const long zones = static_cast<long>(nx1) * nx2 * T.nkr; // interior zones of one block = stride of a component
  for (long tile = blockIdx.x; tile < T.ntile; tile += gridDim.x) {
    const int i = P.is + static_cast<int>(tile % T.gx) * FTX + threadIdx.x;
    const int j = P.js + static_cast<int>((tile / T.gx) % T.gy) * FTY + threadIdx.y;
    const long bz = tile / (static_cast<long>(T.gx) * T.gy);
    const int lb = static_cast<int>(bz / T.nkr); // block of the range, [0, nblocks)
    const int b = block0 + lb;
    const int k = P.ks + static_cast<int>(bz % T.nkr);
    if (i > P.ie || j > P.je) continue;
    const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;
    const long z = (static_cast<long>(k - P.ks) * nx2 + (j - P.js)) * nx1 + (i - P.is);
    const IN *q = in + static_cast<long>(lb) * U.ncomp * zones + z;
    double hx[3];
    scale_factors<CURV>(P, b, k, j, i, hx);
    for (int n = 0; n < (U.gas_form != FORM_NONE ? nsg : 0); ++n) {
      const FluidView &f = P.gas;
      const int nv = 6 * nsg;
      const double D = get(q, (U.g_rho + n) * zones);
      const double w_d = (D > f.dfloor) ? D : f.dfloor;
      const double a1 = get(q, (U.g_vec + 3 * n + 0) * zones);
      const double a2 = get(q, (U.g_vec + 3 * n + 1) * zones);
      const double a3 = get(q, (U.g_vec + 3 * n + 2) * zones);
      const double en = get(q, (U.g_en + n) * zones);
      double vel1 = a1, vel2 = a2, vel3 = a3, w_s = en;
      if (U.gas_form == FORM_PRIM_PRESSURE) {
        w_s = en / (P.gm1 * w_d);
      } else if (U.gas_form == FORM_CONS) {
        // SetAuxillaryFields (set_aux_kernel) ...
        const double u_d2 = amax(D, f.dfloor);
        const double rv1 = a1 / hx[0];
        const double rv2 = a2 / hx[1];
        const double rv3 = a3 / hx[2];
        const double ke = 0.5 * (sqr(rv1) + sqr(rv2) + sqr(rv3)) / u_d2;
        const double ue_cons = en - ke;
        const double eg = (U.g_eint >= 0) ? get(q, (U.g_eint + n) * zones) : 0.0;
        double sie = (ue_cons > f.de_switch * en) ? ue_cons / u_d2 : eg / u_d2;
        sie = amax(sie, f.siefloor);
        double u_u = sie * w_d;
        const double uflr = f.siefloor * w_d;
        u_u = (u_u > uflr) ? u_u : uflr;
        // ... then ConsToPrim (cons_to_prim_kernel)
        vel1 = a1 / (w_d * hx[0]);
        vel2 = a2 / (w_d * hx[1]);
        vel3 = a3 / (w_d * hx[2]);
        w_s = u_u / w_d;
      }
      w_s = (w_s > f.siefloor) ? w_s : f.siefloor;
      f.prim[b * nv + n][c] = w_d;
      f.prim[b * nv + nsg + 3 * n + 0][c] = vel1;
      f.prim[b * nv + nsg + 3 * n + 1][c] = vel2;
      f.prim[b * nv + nsg + 3 * n + 2][c] = vel3;
      f.prim[b * nv + 5 * nsg + n][c] = w_s;
    }
    for (int m = 0; m < (U.dust_form != FORM_NONE ? nsd : 0); ++m) {
      const FluidView &f = P.dust;
      const int nv = 4 * nsd;
      const double D = get(q, (U.d_rho + m) * zones);
      const double w_d = (D > f.dfloor) ? D : f.dfloor;
      f.prim[b * nv + m][c] = w_d;
      for (int d = 0; d < 3; ++d) {
        const double a = get(q, (U.d_vec + 3 * m + d) * zones);
        f.prim[b * nv + nsd + 3 * m + d][c] = (U.dust_form == FORM_CONS) ? a / (w_d * hx[d]) : a;
      }
    }
  }
}
} // namespace

void launch_unpack_fields(const PackView &P, int block0, int nblocks, const FieldUnpack &U, bool single, const void *in, hipStream_t s) {
  FieldTiles T;
  T.gx = (P.ie - P.is + FTX) / FTX, T.gy = (P.je - P.js + FTY) / FTY, T.nkr = P.ke - P.ks + 1;
  T.ntile = static_cast<long>(T.gx) * T.gy * T.nkr * nblocks;
  if (T.ntile == 0 || U.ncomp == 0) return;
  const dim3 t(FTX, FTY), g(static_cast<unsigned>(T.ntile < FIELDS_MAX_WG ? T.ntile : FIELDS_MAX_WG));
  const bool curv = P.coords != ARTEMIS_CARTESIAN;
  if (single) {
    const float *q = static_cast<const float *>(in);
    if (curv) hipLaunchKernelGGL((unpack_fields_kernel<true, float>), g, t, 0, s, P, T, U, block0, q);
    else hipLaunchKernelGGL((unpack_fields_kernel<false, float>), g, t, 0, s, P, T, U, block0, q);
  } else {
    const double *q = static_cast<const double *>(in);
    if (curv) hipLaunchKernelGGL((unpack_fields_kernel<true, double>), g, t, 0, s, P, T, U, block0, q);
    else hipLaunchKernelGGL((unpack_fields_kernel<false, double>), g, t, 0, s, P, T, U, block0, q);
  }
}

void launch_pack_fields(const PackView &P, int block0, int nblocks, const FieldSelection &S, bool single, void *out, hipStream_t s) {
  FieldTiles T;
  T.gx = (P.ie - P.is + FTX) / FTX, T.gy = (P.je - P.js + FTY) / FTY, T.nkr = P.ke - P.ks + 1;
  T.ntile = static_cast<long>(T.gx) * T.gy * T.nkr * nblocks;
  if (T.ntile == 0 || S.ncomp == 0) return;
  const dim3 t(FTX, FTY), g(static_cast<unsigned>(T.ntile < FIELDS_MAX_WG ? T.ntile : FIELDS_MAX_WG));
  const bool curv = P.coords != ARTEMIS_CARTESIAN;
  if (single) {
    float *o = static_cast<float *>(out);
    if (curv) hipLaunchKernelGGL((pack_fields_kernel<true, float>), g, t, 0, s, P, T, S, block0, o);
    else hipLaunchKernelGGL((pack_fields_kernel<false, float>), g, t, 0, s, P, T, S, block0, o);
  } else {
    double *o = static_cast<double *>(out);
    if (curv) hipLaunchKernelGGL((pack_fields_kernel<true, double>), g, t, 0, s, P, T, S, block0, o);
    else hipLaunchKernelGGL((pack_fields_kernel<false, double>), g, t, 0, s, P, T, S, block0, o);
  }
}

} // namespace artemis
