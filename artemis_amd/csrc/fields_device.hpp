// Device code the field-output kernels share (kernels_fields.hip, kernels_reduce.hip): one zone of one species as
// PrimToCons sees it, the components of a variable formed from it, the leaf N = V q of the volume-weighted sums, and the
// exchange between lanes those sums use.  One copy of every expression: what pack_fields stores, what the level kernel
// averages and what the reduce kernel integrates are the same doubles.
#pragma once
#include "device_math.hpp"
#include "fields_derived.hpp"
#include "geometry.hpp"
#include "kernels.hpp"
#include "pack_view.hpp"
#include "task_device.hpp"

namespace artemis {

namespace {
template <class OUT>
__device__ __forceinline__ void put(OUT *out, long at, double v) {
  out[at] = static_cast<OUT>(v); // (double -> float: round to nearest even, the correctly rounded narrowing)
}

// One zone of one species as PrimToCons sees it, and the components of a variable formed from it: the expressions every
// kernel that forms output values shares (f(width, d, v): component d of a variable of `width` components a species).
struct GasZone {
  double w_d, vel1, vel2, vel3, w_s, u_u, ke;
};
struct DustZone {
  double w_d, vel1, vel2, vel3;
};
__device__ __forceinline__ GasZone load_gas(const PackView &P, int b, int n, long c) {
  const FluidView &f = P.gas;
  const int nsg = f.ns, nv = 6 * nsg;
  GasZone z;
  z.w_d = f.prim[b * nv + n][c];
  z.w_d = (z.w_d > f.dfloor) ? z.w_d : f.dfloor;
  z.vel1 = f.prim[b * nv + nsg + 3 * n + 0][c];
  z.vel2 = f.prim[b * nv + nsg + 3 * n + 1][c];
  z.vel3 = f.prim[b * nv + nsg + 3 * n + 2][c];
  z.w_s = f.prim[b * nv + 5 * nsg + n][c];
  z.w_s = (z.w_s > f.siefloor) ? z.w_s : f.siefloor;
  z.u_u = z.w_s * z.w_d;
  z.ke = 0.5 * z.w_d * (sqr(z.vel1) + sqr(z.vel2) + sqr(z.vel3));
  return z;
}
__device__ __forceinline__ DustZone load_dust(const PackView &P, int b, int m, long c) {
  const FluidView &f = P.dust;
  const int nsd = f.ns, nv = 4 * nsd;
  DustZone z;
  z.w_d = f.prim[b * nv + m][c];
  z.w_d = (z.w_d > f.dfloor) ? z.w_d : f.dfloor;
  z.vel1 = f.prim[b * nv + nsd + 3 * m + 0][c];
  z.vel2 = f.prim[b * nv + nsd + 3 * m + 1][c];
  z.vel3 = f.prim[b * nv + nsd + 3 * m + 2][c];
  return z;
}
template <class F>
__device__ __forceinline__ void gas_components(const GasZone &z, double gm1, const double hx[3], int code, F &&f) {
  switch (code) {
  case ARTEMIS_VAR_GAS_PRIM_DENSITY:
  case ARTEMIS_VAR_GAS_CONS_DENSITY: f(1, 0, z.w_d); break;
  case ARTEMIS_VAR_GAS_PRIM_VELOCITY: f(3, 0, z.vel1), f(3, 1, z.vel2), f(3, 2, z.vel3); break;
  case ARTEMIS_VAR_GAS_PRIM_PRESSURE: f(1, 0, amax(0.0, gm1 * z.w_d * z.w_s)); break;
  case ARTEMIS_VAR_GAS_PRIM_SIE: f(1, 0, z.w_s); break;
  case ARTEMIS_VAR_GAS_CONS_MOMENTUM:
    f(3, 0, z.w_d * z.vel1 * hx[0]), f(3, 1, z.w_d * z.vel2 * hx[1]), f(3, 2, z.w_d * z.vel3 * hx[2]);
    break;
  case ARTEMIS_VAR_GAS_CONS_TOTAL_ENERGY: f(1, 0, z.u_u + z.ke); break;
  case ARTEMIS_VAR_GAS_CONS_INTERNAL_ENERGY: f(1, 0, z.u_u); break;
  default: break;
  }
}
template <class F>
__device__ __forceinline__ void dust_components(const DustZone &z, const double hx[3], int code, F &&f) {
  switch (code) {
  case ARTEMIS_VAR_DUST_PRIM_DENSITY:
  case ARTEMIS_VAR_DUST_CONS_DENSITY: f(1, 0, z.w_d); break;
  case ARTEMIS_VAR_DUST_PRIM_VELOCITY: f(3, 0, z.vel1), f(3, 1, z.vel2), f(3, 2, z.vel3); break;
  case ARTEMIS_VAR_DUST_CONS_MOMENTUM:
    f(3, 0, z.w_d * z.vel1 * hx[0]), f(3, 1, z.w_d * z.vel2 * hx[1]), f(3, 2, z.w_d * z.vel3 * hx[2]);
    break;
  default: break;
  }
}

// The derived variables of one species at zone (k, j, i) (fields_derived.hpp: the stencil of the six face neighbours, plain
// 8-byte loads of the stored velocities -- the x1 neighbours in lines the wave or its tile neighbour fetches anyway, the
// x2 / x3 neighbours in rows the tile above or below fetches) and their components, as gas_components hands them out
template <bool CURV, bool GAS>
__device__ __forceinline__ DerivedZone load_derived(const PackView &P, int b, int n, int k, int j, int i) {
  const FluidView &f = GAS ? P.gas : P.dust;
  const int ns = f.ns, v1 = b * (GAS ? 6 : 4) * ns + ns + 3 * n;
  const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;
  const long st[3] = {1, P.ni, static_cast<long>(P.ni) * P.nj};
  const bool act[3] = {P.ie > P.is, P.je > P.js, P.ke > P.ks};
  return derived_zone(
      CURV, act, [&](int d, int a, int s) { return f.prim[v1 + d][c + s * st[a]]; },
      [&](int a, int s) { return make_coords(P, b, k + (a == 2 ? s : 0), j + (a == 1 ? s : 0), i + (a == 0 ? s : 0)); });
}
template <bool GAS, class F>
__device__ __forceinline__ void derived_components(const DerivedZone &z, int code, F &&f) {
  if (code == (GAS ? ARTEMIS_VAR_GAS_DERIVED_DIVERGENCE : ARTEMIS_VAR_DUST_DERIVED_DIVERGENCE)) f(1, 0, z.div);
  else if (code == (GAS ? ARTEMIS_VAR_GAS_DERIVED_VORTICITY : ARTEMIS_VAR_DUST_DERIVED_VORTICITY)) f(3, 0, z.w[0]), f(3, 1, z.w[1]), f(3, 2, z.w[2]);
}
template <int M>
__device__ __forceinline__ double pair_lane(double v) { // v of lane ^ (1 << M), M <= 2
  const int lo = __double2loint(v), hi = __double2hiint(v);
  if constexpr (M == 0) // quad_perm [1, 0, 3, 2]
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xf, 0xf, false));
  else if constexpr (M == 1) // quad_perm [2, 3, 0, 1]
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, 0x4E, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(lo, lo, 0x4E, 0xf, 0xf, false));
  else // ds_swizzle, bit mode: and 0x1f, or 0, xor 4 (the crossbar of the LDS unit; no LDS memory)
    return __hiloint2double(__builtin_amdgcn_ds_swizzle(hi, 0x101F), __builtin_amdgcn_ds_swizzle(lo, 0x101F));
}

// slots of a species: gas  rho | vel 1-3 | P | sie | mom 1-3 | E | eint | V;  dust  rho | vel 1-3 | mom 1-3 | V
template <bool GAS>
struct Slots {
  static constexpr int NV = GAS ? 12 : 8, NCODE = GAS ? 8 : 4, CODE0 = GAS ? 0 : ARTEMIS_VAR_DUST_PRIM_DENSITY;
  static constexpr int slot(int c) { // of variable CODE0 + c
    constexpr int g[8] = {0, 1, 4, 5, 0, 6, 9, 10}, d[4] = {0, 1, 0, 4};
    return GAS ? g[c] : d[c];
  }
  static constexpr int width(int c) { return (c == 1 || (GAS ? c == 5 : c == 3)) ? 3 : 1; }
  double q[NV];
};
// ... and the derived components of a species, a slot set of their own (the level kernel at S = 3 carries seven copies of
// a set: four more slots in Slots<> would cost every existing instantiation about 56 VGPRs):  div | vorticity 1-3 | V
template <bool GAS>
struct DerivedSlots {
  static constexpr int NV = 5, NCODE = 2, CODE0 = GAS ? ARTEMIS_VAR_GAS_DERIVED_DIVERGENCE : ARTEMIS_VAR_DUST_DERIVED_DIVERGENCE;
  static constexpr int slot(int c) { return c == 0 ? 0 : 1; }
  static constexpr int width(int c) { return c == 0 ? 1 : 3; }
  double q[NV];
};
template <int C>
struct IntC {
  static constexpr int value = C;
};
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(IntC<N - 1>{});
  }
}

// N = V q of every slot and V of zone (k, j, i), species n
template <bool CURV, bool GAS>
__device__ __forceinline__ void level_leaf(const PackView &P, int b, int n, int k, int j, int i, Slots<GAS> &s) {
  const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;
  double hx[3];
  scale_factors<CURV>(P, b, k, j, i, hx);
  const double V = make_coords(P, b, k, j, i).volume();
  if constexpr (GAS) {
    const GasZone g = load_gas(P, b, n, c);
    static_for<Slots<GAS>::NCODE>([&](auto cc) {
      constexpr int code = decltype(cc)::value;
      gas_components(g, P.gm1, hx, code, [&](int, int d, double v) { s.q[Slots<GAS>::slot(code) + d] = V * v; });
    });
  } else {
    const DustZone g = load_dust(P, b, n, c);
    static_for<Slots<GAS>::NCODE>([&](auto cc) {
      constexpr int code = decltype(cc)::value;
      dust_components(g, hx, Slots<GAS>::CODE0 + code, [&](int, int d, double v) { s.q[Slots<GAS>::slot(code) + d] = V * v; });
    });
  }
  s.q[Slots<GAS>::NV - 1] = V;
}
template <bool CURV, bool GAS>
__device__ __forceinline__ void level_leaf(const PackView &P, int b, int n, int k, int j, int i, DerivedSlots<GAS> &s) {
  const DerivedZone z = load_derived<CURV, GAS>(P, b, n, k, j, i);
  s.q[0] = z.vol * z.div, s.q[1] = z.vol * z.w[0], s.q[2] = z.vol * z.w[1], s.q[3] = z.vol * z.w[2];
  s.q[4] = z.vol;
}
} // namespace
} // namespace artemis
