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
#include <type_traits>

#include "device_math.hpp"
#include "fields_device.hpp"
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

// every requested component of zone (k, j, i) of block b, component c at o[c * zones]
template <bool CURV, class OUT>
__device__ __forceinline__ void put_zone(const PackView &P, const FieldSelection &S, int b, int k, int j, int i, OUT *o, long zones) {
  const long c = (static_cast<long>(k) * P.nj + j) * P.ni + i;
  double hx[3];
  scale_factors<CURV>(P, b, k, j, i, hx);
  for (int n = 0; n < (S.want_gas ? P.gas.ns : 0); ++n) {
    const GasZone g = load_gas(P, b, n, c);
    for (int e = 0; e < S.nsel; ++e) {
      const long at = S.comp0[e] * zones;
      gas_components(g, P.gm1, hx, S.code[e], [&](int w, int d, double v) { put(o, at + (w * n + d) * zones, v); });
    }
  }
  for (int m = 0; m < (S.want_dust ? P.dust.ns : 0); ++m) {
    const DustZone g = load_dust(P, b, m, c);
    for (int e = 0; e < S.nsel; ++e) {
      const long at = S.comp0[e] * zones;
      dust_components(g, hx, S.code[e], [&](int w, int d, double v) { put(o, at + (w * m + d) * zones, v); });
    }
  }
}

// ... and the derived components of the same selection (codes 16 .. 19: the stencil of fields_derived.hpp).  A pass of its
// own in kernels of its own -- the DERIVED = true instantiations of the kernels below, launched only for a selection that names a
// derived code -- so a request without one runs the kernels it always ran, and the plain kernels skip the derived codes.
template <bool CURV, class OUT>
__device__ __forceinline__ void put_zone_derived(const PackView &P, const FieldSelection &S, int b, int k, int j, int i, OUT *o, long zones) {
  for (int n = 0; n < (S.want_gas ? P.gas.ns : 0); ++n) {
    const DerivedZone z = load_derived<CURV, true>(P, b, n, k, j, i);
    for (int e = 0; e < S.nsel; ++e) {
      const long at = S.comp0[e] * zones;
      derived_components<true>(z, S.code[e], [&](int w, int d, double v) { put(o, at + (w * n + d) * zones, v); });
    }
  }
  for (int m = 0; m < (S.want_dust ? P.dust.ns : 0); ++m) {
    const DerivedZone z = load_derived<CURV, false>(P, b, m, k, j, i);
    for (int e = 0; e < S.nsel; ++e) {
      const long at = S.comp0[e] * zones;
      derived_components<false>(z, S.code[e], [&](int w, int d, double v) { put(o, at + (w * m + d) * zones, v); });
    }
  }
}

// (DERIVED: the derived pass -- S.want_gas / S.want_dust then say which fluids' DERIVED codes the selection names)
template <bool CURV, class OUT, bool DERIVED = false>
__global__ __launch_bounds__(FTX *FTY) void pack_fields_kernel(const PackView P, const FieldTiles T, const FieldSelection S,
                                                              int block0, OUT *out) {
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
    const long z = (static_cast<long>(k - P.ks) * nx2 + (j - P.js)) * nx1 + (i - P.is);
    if constexpr (DERIVED) put_zone_derived<CURV>(P, S, b, k, j, i, out + static_cast<long>(lb) * S.ncomp * zones + z, zones);
    else put_zone<CURV>(P, S, b, k, j, i, out + static_cast<long>(lb) * S.ncomp * zones + z, zones);
  }
}

// ---- field output at a chosen refinement level (artemis_hip_pack_fields_level) ---------------------------------------
// Every block of a launch has one shift s = its level - the level asked for.
//
// s >= 1, pack_fields_level_kernel<CURV, OUT, S>: the volume-weighted mean of RestrictAverage<GEOM> (restriction.hpp:
// 42-114), applied S times with summed volumes.  Per input zone N = V q (q as put_zone forms it, V = Coords::Volume of
// make_coords, Cartesian packs included) and V; both go up the reference's tree
//   X(K,J,I) = ((c000 + c010) + (c001 + c011)) + ((c100 + c110) + (c101 + c111)),   c[ok][oj][oi] = X'(2K+ok, 2J+oj, 2I+oi)
// S times (an inactive direction -- one zone -- is not halved and its offset-1 children are the literal 0.0, added as the
// reference adds them), the output is N / V: one division, then the narrowing.  The read side is pack_fields_kernel's:
// lanes along x1 over the INPUT zones, 64 to a wave, 8-byte loads, the primitives of a species read once per zone.  A
// thread owns one output row and plane: it walks the 2^S rows and 2^S planes under them itself, in the order of the tree
// (t counts the leaves; its bits are j0 k0 j1 k1 ...), and keeps one pending sum per direction and level, so
//   the j pair     is two of its own values,
//   the i pair     one exchange with lane ^ (1 << m) -- a + b and b + a are the same bits, both lanes hold the sum,
//   the k pair     again its own.
// Groups of 2^S lanes start at the interior's first zone (64 is a multiple of 8 and nx1 of 2^S: a tile's ragged tail is
// whole groups); lanes past the row's end load its last zone and store nothing, rows past the block's end are whole waves
// (blockDim.x is the wave).  So every lane of a wave takes every exchange.  No LDS, no atomics, vector stores by the lane
// with (i - is) % 2^S == 0, 64-bit offsets.  All slots of a species are carried (11 + V of a gas species, 7 + V of a
// dust species) and the ones asked for are divided and stored: the slots are registers only while their index is static.
//
// s <= 0, pack_fields_replicate_kernel: out(k, j, i) = q(k >> |s|, j >> |s|, i >> |s|) along the active directions, lanes
// along the OUTPUT x1 -- exact copies, no slopes (a dump invents no gradients, and the ghost zones a prolongation reads
// may be stale).
constexpr int LEVEL_MAX_BLOCKS = 96;
struct LevelBlocks {          // the blocks of one launch, by value: a dump is a handful of launches, no table to upload
  int n, lb[LEVEL_MAX_BLOCKS]; // block of the range
  long off[LEVEL_MAX_BLOCKS];  // element offset of its first value in the output
};
struct LevelTiles {
  int gx, gy, nxo, nyo, nzo; // tiles along x1 (input zones: restrict; output zones: replicate) and along the output rows
  long ntile;
};
static_assert(sizeof(PackView) + sizeof(FieldSelection) + sizeof(LevelBlocks) + sizeof(LevelTiles) + 64 <= 4096, "kernel arguments");

// (SL: the slot set that goes up the tree -- Slots<GAS>, or DerivedSlots<GAS> in the derived pass)
template <bool CURV, bool GAS, int S, class SL, class OUT>
__device__ __forceinline__ void level_species(const PackView &P, const FieldSelection &F, int b, int n, int k0, int j0, int i,
                                              bool store, OUT *o, long ozones) {
  const bool ia = P.ie > P.is, ja = P.je > P.js, ka = P.ke > P.ks;
  const int nbits = (ja ? 1 : 0) + (ka ? 1 : 0), jbit = 0, kbit = ja ? 1 : 0;
  SL v, sj[S], sk[S];
  for (int t = 0; t < (1 << (S * nbits)); ++t) { // (wave-uniform: every branch on t below is)
    int dj = 0, dk = 0;
#pragma unroll
    for (int m = 0; m < S; ++m) {
      if (ja) dj |= ((t >> (m * nbits + jbit)) & 1) << m;
      if (ka) dk |= ((t >> (m * nbits + kbit)) & 1) << m;
    }
    level_leaf<CURV, GAS>(P, b, n, k0 + dk, j0 + dj, i, v);
    bool carry = true; // the sums of level m are complete: they enter level m + 1
    static_for<S>([&](auto mm) {
      constexpr int m = decltype(mm)::value;
      if (carry) { // the j pair
        if (!ja) {
          for (int q = 0; q < SL::NV; ++q) v.q[q] = v.q[q] + 0.0;
        } else if ((t >> (m * nbits + jbit)) & 1) {
          for (int q = 0; q < SL::NV; ++q) v.q[q] = sj[m].q[q] + v.q[q];
        } else {
          sj[m] = v, carry = false;
        }
      }
      if (carry) { // the i pair
        for (int q = 0; q < SL::NV; ++q) v.q[q] = v.q[q] + (ia ? pair_lane<m>(v.q[q]) : 0.0);
      }
      if (carry) { // the k pair
        if (!ka) {
          for (int q = 0; q < SL::NV; ++q) v.q[q] = v.q[q] + 0.0;
        } else if ((t >> (m * nbits + kbit)) & 1) {
          for (int q = 0; q < SL::NV; ++q) v.q[q] = sk[m].q[q] + v.q[q];
        } else {
          sk[m] = v, carry = false;
        }
      }
    });
  }
  if (!store) return;
  const double vol = v.q[SL::NV - 1];
  for (int e = 0; e < F.nsel; ++e) {
    const long at = F.comp0[e] * ozones;
    const int code = F.code[e] - SL::CODE0;
    static_for<SL::NCODE>([&](auto cc) {
      constexpr int c = decltype(cc)::value, w = SL::width(c);
      if (code == c)
        for (int d = 0; d < w; ++d) put(o, at + (w * n + d) * ozones, v.q[SL::slot(c) + d] / vol);
    });
  }
}

template <bool CURV, class OUT, int S, bool DERIVED = false>
__global__ __launch_bounds__(FTX *FTY) void pack_fields_level_kernel(const PackView P, const LevelTiles T, const FieldSelection F,
                                                                    const LevelBlocks B, int block0, OUT *out) {
  const bool ia = P.ie > P.is, ja = P.je > P.js, ka = P.ke > P.ks;
  const long ozones = static_cast<long>(T.nxo) * T.nyo * T.nzo;
  for (long tile = blockIdx.x; tile < T.ntile; tile += gridDim.x) {
    const int i = P.is + static_cast<int>(tile % T.gx) * FTX + threadIdx.x; // input zone
    const int J = static_cast<int>((tile / T.gx) % T.gy) * FTY + threadIdx.y; // output row
    const long bz = tile / (static_cast<long>(T.gx) * T.gy);
    const int q = static_cast<int>(bz / T.nzo), K = static_cast<int>(bz % T.nzo);
    const int b = block0 + B.lb[q];
    if (J >= T.nyo) continue; // (a whole wave)
    const int ic = (i < P.ie) ? i : P.ie;
    const int j0 = P.js + (ja ? J << S : J), k0 = P.ks + (ka ? K << S : K);
    const int io = ia ? (ic - P.is) >> S : ic - P.is;
    const bool store = i <= P.ie && (!ia || ((i - P.is) & ((1 << S) - 1)) == 0);
    OUT *o = out + B.off[q] + (static_cast<long>(K) * T.nyo + J) * T.nxo + io;
    using SG = std::conditional_t<DERIVED, DerivedSlots<true>, Slots<true>>;
    using SD = std::conditional_t<DERIVED, DerivedSlots<false>, Slots<false>>;
    for (int n = 0; n < (F.want_gas ? P.gas.ns : 0); ++n) level_species<CURV, true, S, SG>(P, F, b, n, k0, j0, ic, store, o, ozones);
    for (int m = 0; m < (F.want_dust ? P.dust.ns : 0); ++m) level_species<CURV, false, S, SD>(P, F, b, m, k0, j0, ic, store, o, ozones);
  }
}

template <bool CURV, class OUT, bool DERIVED = false>
__global__ __launch_bounds__(FTX *FTY) void pack_fields_replicate_kernel(const PackView P, const LevelTiles T, const FieldSelection F,
                                                                        const LevelBlocks B, int block0, int r, OUT *out) {
  const int ri = P.ie > P.is ? r : 0, rj = P.je > P.js ? r : 0, rk = P.ke > P.ks ? r : 0;
  const long ozones = static_cast<long>(T.nxo) * T.nyo * T.nzo;
  for (long tile = blockIdx.x; tile < T.ntile; tile += gridDim.x) {
    const int io = static_cast<int>(tile % T.gx) * FTX + threadIdx.x; // output zone
    const int jo = static_cast<int>((tile / T.gx) % T.gy) * FTY + threadIdx.y;
    const long bz = tile / (static_cast<long>(T.gx) * T.gy);
    const int q = static_cast<int>(bz / T.nzo), ko = static_cast<int>(bz % T.nzo);
    if (io >= T.nxo || jo >= T.nyo) continue;
    if constexpr (DERIVED)
      put_zone_derived<CURV>(P, F, block0 + B.lb[q], P.ks + (ko >> rk), P.js + (jo >> rj), P.is + (io >> ri),
                             out + B.off[q] + (static_cast<long>(ko) * T.nyo + jo) * T.nxo + io, ozones);
    else
      put_zone<CURV>(P, F, block0 + B.lb[q], P.ks + (ko >> rk), P.js + (jo >> rj), P.is + (io >> ri),
                     out + B.off[q] + (static_cast<long>(ko) * T.nyo + jo) * T.nxo + io, ozones);
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
  const dim3 t(FTX, FTY), g(static_cast<unsigned>(grid_capped(T.ntile < FIELDS_MAX_WG ? T.ntile : FIELDS_MAX_WG)));
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

namespace {
template <bool CURV, class OUT>
void launch_level_chunk(const PackView &P, int block0, const FieldPasses &X, const LevelBlocks &B, int shift, OUT *o, hipStream_t s) {
  const int nx1 = P.ie - P.is + 1, nx2 = P.je - P.js + 1, nx3 = P.ke - P.ks + 1;
  LevelTiles T;
  T.nxo = level_extent(nx1, shift), T.nyo = level_extent(nx2, shift), T.nzo = level_extent(nx3, shift);
  T.gx = ((shift > 0 ? nx1 : T.nxo) + FTX - 1) / FTX, T.gy = (T.nyo + FTY - 1) / FTY;
  T.ntile = static_cast<long>(T.gx) * T.gy * T.nzo * B.n;
  if (T.ntile == 0) return;
  const dim3 t(FTX, FTY), g(static_cast<unsigned>(grid_capped(T.ntile < FIELDS_MAX_WG ? T.ntile : FIELDS_MAX_WG)));
  if (X.has_plain) {
    const FieldSelection &F = X.plain;
    if (shift == 1) hipLaunchKernelGGL((pack_fields_level_kernel<CURV, OUT, 1>), g, t, 0, s, P, T, F, B, block0, o);
    else if (shift == 2) hipLaunchKernelGGL((pack_fields_level_kernel<CURV, OUT, 2>), g, t, 0, s, P, T, F, B, block0, o);
    else if (shift == 3) hipLaunchKernelGGL((pack_fields_level_kernel<CURV, OUT, 3>), g, t, 0, s, P, T, F, B, block0, o);
    else hipLaunchKernelGGL((pack_fields_replicate_kernel<CURV, OUT>), g, t, 0, s, P, T, F, B, block0, -shift, o);
  }
  if (X.has_derived) {
    const FieldSelection &F = X.derived;
    if (shift == 1) hipLaunchKernelGGL((pack_fields_level_kernel<CURV, OUT, 1, true>), g, t, 0, s, P, T, F, B, block0, o);
    else if (shift == 2) hipLaunchKernelGGL((pack_fields_level_kernel<CURV, OUT, 2, true>), g, t, 0, s, P, T, F, B, block0, o);
    else if (shift == 3) hipLaunchKernelGGL((pack_fields_level_kernel<CURV, OUT, 3, true>), g, t, 0, s, P, T, F, B, block0, o);
    else hipLaunchKernelGGL((pack_fields_replicate_kernel<CURV, OUT, true>), g, t, 0, s, P, T, F, B, block0, -shift, o);
  }
}
} // namespace

// One launch per distinct shift and LEVEL_MAX_BLOCKS blocks of it; off[b]: element offset of block block0 + b in `out`.
// The caller has checked the shifts (|shift| <= 3, extents divisible).
void launch_pack_fields_level(const PackView &P, int block0, int nblocks, const FieldSelection &F, bool single, const int *shift,
                              const long *off, void *out, hipStream_t s) {
  if (F.ncomp == 0) return;
  const bool curv = P.coords != ARTEMIS_CARTESIAN;
  const FieldPasses X = field_passes(F);
  for (int sh = -FIELDS_MAX_SHIFT; sh <= FIELDS_MAX_SHIFT; ++sh) {
    LevelBlocks B;
    B.n = 0;
    for (int b = 0; b <= nblocks; ++b) {
      if (b < nblocks && shift[b] == sh) B.lb[B.n] = b, B.off[B.n] = off[b], B.n++;
      if (B.n == LEVEL_MAX_BLOCKS || (b == nblocks && B.n > 0)) {
        if (single) {
          float *o = static_cast<float *>(out);
          if (curv) launch_level_chunk<true>(P, block0, X, B, sh, o, s);
          else launch_level_chunk<false>(P, block0, X, B, sh, o, s);
        } else {
          double *o = static_cast<double *>(out);
          if (curv) launch_level_chunk<true>(P, block0, X, B, sh, o, s);
          else launch_level_chunk<false>(P, block0, X, B, sh, o, s);
        }
        B.n = 0;
      }
    }
  }
}

void launch_pack_fields(const PackView &P, int block0, int nblocks, const FieldSelection &S, bool single, void *out, hipStream_t s) {
  FieldTiles T;
  T.gx = (P.ie - P.is + FTX) / FTX, T.gy = (P.je - P.js + FTY) / FTY, T.nkr = P.ke - P.ks + 1;
  T.ntile = static_cast<long>(T.gx) * T.gy * T.nkr * nblocks;
  if (T.ntile == 0 || S.ncomp == 0) return;
  const dim3 t(FTX, FTY), g(static_cast<unsigned>(grid_capped(T.ntile < FIELDS_MAX_WG ? T.ntile : FIELDS_MAX_WG)));
  const bool curv = P.coords != ARTEMIS_CARTESIAN;
  const FieldPasses X = field_passes(S);
  if (single) {
    float *o = static_cast<float *>(out);
    if (X.has_plain) {
      if (curv) hipLaunchKernelGGL((pack_fields_kernel<true, float>), g, t, 0, s, P, T, X.plain, block0, o);
      else hipLaunchKernelGGL((pack_fields_kernel<false, float>), g, t, 0, s, P, T, X.plain, block0, o);
    }
    if (X.has_derived) {
      if (curv) hipLaunchKernelGGL((pack_fields_kernel<true, float, true>), g, t, 0, s, P, T, X.derived, block0, o);
      else hipLaunchKernelGGL((pack_fields_kernel<false, float, true>), g, t, 0, s, P, T, X.derived, block0, o);
    }
  } else {
    double *o = static_cast<double *>(out);
    if (X.has_plain) {
      if (curv) hipLaunchKernelGGL((pack_fields_kernel<true, double>), g, t, 0, s, P, T, X.plain, block0, o);
      else hipLaunchKernelGGL((pack_fields_kernel<false, double>), g, t, 0, s, P, T, X.plain, block0, o);
    }
    if (X.has_derived) {
      if (curv) hipLaunchKernelGGL((pack_fields_kernel<true, double, true>), g, t, 0, s, P, T, X.derived, block0, o);
      else hipLaunchKernelGGL((pack_fields_kernel<false, double, true>), g, t, 0, s, P, T, X.derived, block0, o);
    }
  }
}

} // namespace artemis
