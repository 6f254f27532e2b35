// Reduced field output (artemis_hip_reduce_fields): the requested components integrated over chosen directions of every
// block of a range.  include/artemis_hip.h has the definition; it fixes the bits, this file only has to produce them.
//
// Per interior zone and requested component c the leaf is N_c = V q_c, q_c the double pack_fields_kernel stores (the shared
// expressions of fields_device.hpp) and V = Coords::Volume, and W = V.  N_c and W are summed one direction at a time, x1
// first, then x2, then x3, the directions not asked for skipped; a block leaves [ncomp + 1][nz'][ny'][nx'], W last.
//
// The FIRST pass reads the primitives and is the hot one -- every later pass reads arrays smaller by a whole extent.  It
// keeps the read side of pack_fields_kernel: lanes along x1, 64 to a wave, 8-byte loads, the primitives of a species read
// once per zone, all slots of a species in registers with static indices (Slots<GAS>, as the level kernel carries them).
//   x1 reduced (reduce_fields_kernel<.., 0>)   a wave owns one row (k, j).  It walks the row in chunks of 64 zones from the
//       interior's first zone; lanes past the row's end hold the literal 0.0; six exchanges x' = x + x[lane ^ (1 << m)],
//       m = 0..5 (DPP quad_perm, DPP row_ror:8, ds_swizzle, ds_bpermute: register traffic, no LDS memory), leave the
//       chunk's sum in every lane; the chunks are added in increasing order.  Rows past the block's end are whole waves,
//       so every lane takes every exchange.  Lane 0 stores.
//   x1 kept (.., 1: x2 first; .., 2: x3 only)   a thread owns a column (i and the other kept index) and walks the reduced
//       direction itself, acc = x[0]; acc = acc + x[1]; ..., the leaf of the next zone loaded before the current is added.
// The later passes (reduce_axis_kernel) walk x2 or x3 of a double work array the same way, one thread per output element,
// four loads ahead of the additions.  Only the last pass narrows to float.  The sums of one direction are independent for
// every index of the directions still to come: a radial profile of a 256 x 128^2 block is 128 x 128 waves on the rows,
// then 128 chains of 128, then one of 128 -- never one wave walking a block.
// No LDS, no atomics, no tickets: no sum's order depends on the launch.  64-bit offsets.
#include <type_traits>

#include "device_math.hpp"
#include "fields_device.hpp"
#include "geometry.hpp"
#include "kernels.hpp"
#include "pack_view.hpp"
#include "task_device.hpp"

namespace artemis {

namespace {
constexpr int RTX = 64, RTY = 4;
constexpr long REDUCE_MAX_WG = 2048; // 256 CUs x 8 workgroups; the rest of the tiles by grid stride

struct ReduceTiles {
  int gx, gy, nxo, nyo, nzo; // tiles of 64 along x1 (1 where x1 is reduced), of 4 along the other kept index; output extents
  long ntile;
  unsigned gmask, dmask; // the slots of a gas / dust species the selection needs (bit NV - 1: the volume, always)
};

template <int M>
__device__ __forceinline__ double xor_lane(double v) { // v of lane ^ (1 << M) of a 64-lane wave
  if constexpr (M <= 2) {
    return pair_lane<M>(v);
  } else {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    if constexpr (M == 3) // row_ror:8 -- lane (l + 8) % 16 of the row of 16, which is l ^ 8
      return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, 0x128, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(lo, lo, 0x128, 0xf, 0xf, false));
    else if constexpr (M == 4) // ds_swizzle, bit mode: and 0x1f, or 0, xor 16
      return __hiloint2double(__builtin_amdgcn_ds_swizzle(hi, 0x401F), __builtin_amdgcn_ds_swizzle(lo, 0x401F));
    else { // ds_bpermute: the other half of the wave (byte address of the source lane)
      const int from = (static_cast<int>(threadIdx.x) ^ 32) << 2;
      return __hiloint2double(__builtin_amdgcn_ds_bpermute(from, hi), __builtin_amdgcn_ds_bpermute(from, lo));
    }
  }
}
// the sum of a chunk of 64, in every lane: a + b and b + a are the same bits
__device__ __forceinline__ double chunk_sum(double v) {
  static_for<6>([&](auto mm) { v = v + xor_lane<decltype(mm)::value>(v); });
  return v;
}

// The first pass for one species: DIR = 0 the x1 row of (k, j) in chunks, DIR = 1 the x2 column of (k, i), DIR = 2 the x3
// column of (j, i); `a` and `c` are the two fixed indices in (k, j, i) order.
// (SL: Slots<GAS>, or DerivedSlots<GAS> in the derived pass)
template <bool CURV, bool GAS, int DIR, class SL>
__device__ __forceinline__ void first_pass(const PackView &P, int b, int n, int a, int c, unsigned mask, SL &acc) {
  if constexpr (DIR == 0) {
    const int nx1 = P.ie - P.is + 1;
    for (int i0 = 0; i0 < nx1; i0 += RTX) { // (wave-uniform)
      const int i = P.is + i0 + static_cast<int>(threadIdx.x);
      SL v;
      level_leaf<CURV, GAS>(P, b, n, a, c, i <= P.ie ? i : P.ie, v);
      static_for<SL::NV>([&](auto qq) {
        constexpr int q = decltype(qq)::value;
        if ((mask >> q) & 1) {
          const double s = chunk_sum(i <= P.ie ? v.q[q] : 0.0);
          acc.q[q] = (i0 == 0) ? s : acc.q[q] + s;
        }
      });
    }
  } else {
    const int t0 = (DIR == 1) ? P.js : P.ks, t1 = (DIR == 1) ? P.je : P.ke;
    auto leaf = [&](int t, SL &v) {
      if constexpr (DIR == 1) level_leaf<CURV, GAS>(P, b, n, a, t, c, v);
      else level_leaf<CURV, GAS>(P, b, n, t, a, c, v);
    };
    SL cur{}, nxt{}; // (value-initialised: the last iteration copies a `nxt` no leaf has filled)
    leaf(t0, acc);
    if (t0 < t1) leaf(t0 + 1, cur);
    for (int t = t0 + 1; t <= t1; ++t) {
      if (t < t1) leaf(t + 1, nxt); // (issued ahead of the additions below)
      static_for<SL::NV>([&](auto qq) {
        constexpr int q = decltype(qq)::value;
        if ((mask >> q) & 1) acc.q[q] = acc.q[q] + cur.q[q];
      });
      cur = nxt;
    }
  }
}

template <class SL, class OUT>
__device__ __forceinline__ void store_species(const FieldSelection &F, int n, const SL &acc, OUT *o, long ozones) {
  for (int e = 0; e < F.nsel; ++e) {
    const long at = F.comp0[e] * ozones;
    const int code = F.code[e] - SL::CODE0;
    static_for<SL::NCODE>([&](auto cc) {
      constexpr int c = decltype(cc)::value, w = SL::width(c);
      if (code == c)
        for (int d = 0; d < w; ++d) put(o, at + (w * n + d) * ozones, acc.q[SL::slot(c) + d]);
    });
  }
  put(o, F.ncomp * ozones, acc.q[SL::NV - 1]); // W: the same bits from every species
}

// DERIVED: the derived pass, a launch of its own -- F.want_gas / F.want_dust name the fluids whose derived codes are asked
// for, T.gmask / T.dmask are masks of DerivedSlots; W is the same sum from either pass
template <bool CURV, class OUT, int DIR, bool DERIVED = false>
__global__ __launch_bounds__(RTX *RTY) void reduce_fields_kernel(const PackView P, const ReduceTiles T, const FieldSelection F, int block0,
                                                                OUT *out) {
  using SG = std::conditional_t<DERIVED, DerivedSlots<true>, Slots<true>>;
  using SD = std::conditional_t<DERIVED, DerivedSlots<false>, Slots<false>>;
  const long ozones = static_cast<long>(T.nxo) * T.nyo * T.nzo;
  for (long tile = blockIdx.x; tile < T.ntile; tile += gridDim.x) {
    const int tx = static_cast<int>(tile % T.gx), ty = static_cast<int>((tile / T.gx) % T.gy);
    const long rest = tile / (static_cast<long>(T.gx) * T.gy);
    int lb, a, c;     // block of the range and the two fixed indices, (k, j, i) order
    long z;           // output zone
    bool store = true;
    if constexpr (DIR == 0) { // a wave per row: rest = (block, k), ty tiles j
      lb = static_cast<int>(rest / T.nzo);
      const int K = static_cast<int>(rest % T.nzo), J = ty * RTY + static_cast<int>(threadIdx.y);
      if (J >= T.nyo) continue; // (a whole wave)
      a = P.ks + K, c = P.js + J, z = static_cast<long>(K) * T.nyo + J;
      store = threadIdx.x == 0;
    } else if constexpr (DIR == 1) { // thread (k, i): rest = block, ty tiles k
      lb = static_cast<int>(rest);
      const int K = ty * RTY + static_cast<int>(threadIdx.y), I = tx * RTX + static_cast<int>(threadIdx.x);
      if (K >= T.nzo || I >= T.nxo) continue;
      a = P.ks + K, c = P.is + I, z = static_cast<long>(K) * T.nxo + I;
    } else { // thread (j, i): rest = block, ty tiles j
      lb = static_cast<int>(rest);
      const int J = ty * RTY + static_cast<int>(threadIdx.y), I = tx * RTX + static_cast<int>(threadIdx.x);
      if (J >= T.nyo || I >= T.nxo) continue;
      a = P.js + J, c = P.is + I, z = static_cast<long>(J) * T.nxo + I;
    }
    const int b = block0 + lb;
    OUT *o = out + static_cast<long>(lb) * (F.ncomp + 1) * ozones + z;
    for (int n = 0; n < (F.want_gas ? P.gas.ns : 0); ++n) {
      SG acc{}; // (the slots outside the mask stay 0.0 and are never stored)
      first_pass<CURV, true, DIR>(P, b, n, a, c, T.gmask, acc);
      if (store) store_species(F, n, acc, o, ozones);
    }
    for (int m = 0; m < (F.want_dust ? P.dust.ns : 0); ++m) {
      SD acc{};
      first_pass<CURV, false, DIR>(P, b, m, a, c, T.dmask, acc);
      if (store) store_species(F, m, acc, o, ozones);
    }
  }
}

// A later pass: in [rows][len][inner] -> out [rows][inner], out(r, x) = in(r, 0, x) + in(r, 1, x) + ... in increasing order
template <class OUT>
__global__ __launch_bounds__(256) void reduce_axis_kernel(const double *in, long rows, int len, long inner, OUT *out) {
  const long total = rows * inner;
  for (long e = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += static_cast<long>(gridDim.x) * blockDim.x) {
    const double *x = in + (e / inner) * len * inner + e % inner;
    double acc = x[0];
    int t = 1;
    for (; t + 3 < len; t += 4) {
      const double a0 = x[t * inner], a1 = x[(t + 1) * inner], a2 = x[(t + 2) * inner], a3 = x[(t + 3) * inner];
      acc = acc + a0, acc = acc + a1, acc = acc + a2, acc = acc + a3;
    }
    for (; t < len; ++t) acc = acc + x[t * inner];
    put(out, e, acc);
  }
}

// ---- reduced output on a chosen level (artemis_hip_reduce_fields_level) -------------------------------------------------
// The passes above leave every block of the range as doubles [ncomp + 1][n3][n2][n1] in the work buffer, the reduced
// extents 1.  resample_reduced_kernel brings block q to its shift s along the KEPT directions (active and not reduced; at
// most two, A before B in the order x1, x2, x3) and narrows at this one store:
//   s >= 1   out = the pair tree x[0::2] + x[1::2], s times along A, then s times along B: the thread reads its 2^s values
//            along A (all loads of a row issued ahead of its additions), adds them as the tree, and does so for each of
//            its 2^s rows along B, whose results go up the same tree.  Plain additions.
//   s == 0   a copy.
//   s <= -1  out(k, j, i) = x(k >> |s|, j >> |s|, i >> |s|) * 2^(-|s| m) along the kept directions, m their number: one load,
//            one exact multiply (a power of two), one store; m = 0: no multiply at all.
// One thread per OUTPUT element, consecutive lanes on consecutive elements of a block's output -- the first kept direction
// is the fastest one -- 256 to a tile, the tiles of the launch's blocks one after the other (tile0) and taken by grid
// stride; lanes past a block's last element store nothing.  The blocks of a launch are consecutive blocks of the range
// and may differ in shift: shift, output offset and first tile travel by value (no table to upload).  No LDS, no atomics,
// vector stores, 64-bit offsets.
constexpr int RESAMPLE_MAX_BLOCKS = 192;
struct ResampleBlocks {
  int n, q0;                          // blocks of this launch, the first one's place in the range
  int tile0[RESAMPLE_MAX_BLOCKS + 1]; // first tile of every block, and the number of tiles
  long off[RESAMPLE_MAX_BLOCKS];      // element offset of the block's first value in the output
  signed char shift[RESAMPLE_MAX_BLOCKS];
};
struct ResampleShape {
  int n[3], kept[3]; // extents the passes left (1 where reduced); 1 where the direction is kept
  int rows, m;       // ncomp + 1; kept directions
};
static_assert(sizeof(ResampleBlocks) + sizeof(ResampleShape) + 64 <= 4096, "kernel arguments");

template <int S>
__device__ __forceinline__ double pair_tree(double (&v)[1 << S]) {
  static_for<S>([&](auto mm) {
    constexpr int half = 1 << (S - 1 - decltype(mm)::value);
#pragma unroll
    for (int l = 0; l < half; ++l) v[l] = v[2 * l] + v[2 * l + 1];
  });
  return v[0];
}
// x: the first of the 2^S (A) x 2^S (B) inputs of one output element; a direction that is not there has stride 0 and one value
template <int S>
__device__ __forceinline__ double restrict_pairs(const double *x, bool hasA, long sA, bool hasB, long sB) {
  constexpr int R = 1 << S;
  double b[R];
#pragma unroll
  for (int tb = 0; tb < R; ++tb) {
    b[tb] = 0.0;
    if (tb == 0 || hasB) {
      double a[R];
#pragma unroll
      for (int ta = 0; ta < R; ++ta) a[ta] = (ta == 0 || hasA) ? x[tb * sB + ta * sA] : 0.0; // (issued ahead of the additions)
      b[tb] = hasA ? pair_tree<S>(a) : a[0];
    }
  }
  return hasB ? pair_tree<S>(b) : b[0];
}

template <class OUT>
__global__ __launch_bounds__(256) void resample_reduced_kernel(const double *in, const ResampleShape H, const ResampleBlocks B, OUT *out) {
  const long zin = static_cast<long>(H.n[0]) * H.n[1] * H.n[2];
  const long stride[3] = {1, H.n[0], static_cast<long>(H.n[0]) * H.n[1]};
  for (long tile = blockIdx.x; tile < B.tile0[B.n]; tile += gridDim.x) {
    int q = 0, hi = B.n; // the block of this tile: the last one with tile0 <= tile (uniform over the workgroup)
    while (hi - q > 1) {
      const int mid = (q + hi) >> 1;
      if (B.tile0[mid] <= tile) q = mid;
      else hi = mid;
    }
    const int s = B.shift[q], r = s < 0 ? -s : s;
    int o[3];
    for (int d = 0; d < 3; ++d) o[d] = !H.kept[d] ? H.n[d] : (s >= 0 ? H.n[d] >> r : H.n[d] << r);
    const long oz = static_cast<long>(o[0]) * o[1] * o[2];
    const long e = (tile - B.tile0[q]) * 256 + threadIdx.x;
    if (e >= H.rows * oz) continue;
    const long c = e / oz, z = e % oz;
    const int io[3] = {static_cast<int>(z % o[0]), static_cast<int>((z / o[0]) % o[1]), static_cast<int>(z / (static_cast<long>(o[0]) * o[1]))};
    long at = ((static_cast<long>(B.q0) + q) * H.rows + c) * zin; // the input element this one starts from
    bool hasA = false, hasB = false;
    long sA = 0, sB = 0;
    for (int d = 0; d < 3; ++d) {
      at += stride[d] * (!H.kept[d] ? io[d] : (s >= 0 ? static_cast<long>(io[d]) << r : io[d] >> r));
      if (H.kept[d]) {
        if (!hasA) hasA = true, sA = stride[d];
        else hasB = true, sB = stride[d];
      }
    }
    const double *x = in + at;
    double v;
    if (s == 1) v = restrict_pairs<1>(x, hasA, sA, hasB, sB);
    else if (s == 2) v = restrict_pairs<2>(x, hasA, sA, hasB, sB);
    else if (s == 3) v = restrict_pairs<3>(x, hasA, sA, hasB, sB);
    else {
      v = x[0];
      if (s < 0 && H.m > 0) v = v * __hiloint2double((1023 - r * H.m) << 20, 0); // 2^(-|s| m), exact
    }
    put(out, B.off[q] + e, v);
  }
}

template <class SL>
unsigned slot_mask(const FieldSelection &F) {
  unsigned m = 1u << (SL::NV - 1);
  for (int e = 0; e < F.nsel; ++e) {
    const int c = F.code[e] - SL::CODE0;
    if (c < 0 || c >= SL::NCODE) continue;
    for (int d = 0; d < SL::width(c); ++d) m |= 1u << (SL::slot(c) + d);
  }
  return m;
}

template <bool CURV, class OUT>
void launch_first(const PackView &P, int block0, int nblocks, const FieldSelection &F, int dir, OUT *o, hipStream_t s) {
  const int nx1 = P.ie - P.is + 1, nx2 = P.je - P.js + 1, nx3 = P.ke - P.ks + 1;
  ReduceTiles T;
  T.nxo = dir == 0 ? 1 : nx1, T.nyo = dir == 1 ? 1 : nx2, T.nzo = dir == 2 ? 1 : nx3;
  T.gx = dir == 0 ? 1 : (nx1 + RTX - 1) / RTX;
  T.gy = ((dir == 1 ? nx3 : nx2) + RTY - 1) / RTY;
  T.ntile = static_cast<long>(T.gx) * T.gy * (dir == 0 ? nx3 : 1) * nblocks;
  const dim3 t(RTX, RTY), g(static_cast<unsigned>(grid_capped(T.ntile < REDUCE_MAX_WG ? T.ntile : REDUCE_MAX_WG)));
  const FieldPasses X = field_passes(F);
  if (X.has_plain) {
    T.gmask = slot_mask<Slots<true>>(F), T.dmask = slot_mask<Slots<false>>(F);
    if (dir == 0) hipLaunchKernelGGL((reduce_fields_kernel<CURV, OUT, 0>), g, t, 0, s, P, T, F, block0, o);
    else if (dir == 1) hipLaunchKernelGGL((reduce_fields_kernel<CURV, OUT, 1>), g, t, 0, s, P, T, F, block0, o);
    else hipLaunchKernelGGL((reduce_fields_kernel<CURV, OUT, 2>), g, t, 0, s, P, T, F, block0, o);
  }
  if (X.has_derived) { // a launch of its own, for a selection that names a derived code
    const FieldSelection &D = X.derived;
    T.gmask = slot_mask<DerivedSlots<true>>(F), T.dmask = slot_mask<DerivedSlots<false>>(F);
    if (dir == 0) hipLaunchKernelGGL((reduce_fields_kernel<CURV, OUT, 0, true>), g, t, 0, s, P, T, D, block0, o);
    else if (dir == 1) hipLaunchKernelGGL((reduce_fields_kernel<CURV, OUT, 1, true>), g, t, 0, s, P, T, D, block0, o);
    else hipLaunchKernelGGL((reduce_fields_kernel<CURV, OUT, 2, true>), g, t, 0, s, P, T, D, block0, o);
  }
}

template <class OUT>
void launch_axis(const double *in, long rows, int len, long inner, OUT *o, hipStream_t s) {
  const long total = rows * inner, wg = (total + 255) / 256;
  hipLaunchKernelGGL((reduce_axis_kernel<OUT>), dim3(static_cast<unsigned>(grid_capped(wg < REDUCE_MAX_WG ? wg : REDUCE_MAX_WG))), dim3(256), 0, s, in, rows,
                     len, inner, o);
}
} // namespace

// doubles of work the passes before the last leave behind them, for nblocks blocks of nx zones and ncomp components
long reduce_fields_work_elements(const int nx[3], int nblocks, int ncomp, int axes) {
  long n[3] = {nx[0], nx[1], nx[2]}, total = 0;
  int left = ((axes >> 0) & 1) + ((axes >> 1) & 1) + ((axes >> 2) & 1);
  for (int d = 0; d < 3 && left > 1; ++d)
    if ((axes >> d) & 1) n[d] = 1, --left, total += static_cast<long>(nblocks) * (ncomp + 1) * n[0] * n[1] * n[2];
  return total;
}

// The caller has checked `axes` (1..7, active directions only) and the selection (ncomp > 0).
void launch_reduce_fields(const PackView &P, int block0, int nblocks, const FieldSelection &F, bool single, int axes, void *out, double *work,
                          hipStream_t s) {
  if (nblocks == 0 || F.ncomp == 0) return;
  const bool curv = P.coords != ARTEMIS_CARTESIAN;
  long n[3] = {P.ie - P.is + 1, P.je - P.js + 1, P.ke - P.ks + 1};
  int left = ((axes >> 0) & 1) + ((axes >> 1) & 1) + ((axes >> 2) & 1);
  const long rows0 = static_cast<long>(nblocks) * (F.ncomp + 1);
  const double *in = nullptr;
  for (int d = 0; d < 3; ++d) {
    if (!((axes >> d) & 1)) continue;
    const bool last = --left == 0, first = in == nullptr;
    const int len = static_cast<int>(n[d]);
    n[d] = 1;
    double *w = work; // where a pass that is not the last leaves its sums
    if (first) {
      if (last && single) {
        float *o = static_cast<float *>(out);
        if (curv) launch_first<true>(P, block0, nblocks, F, d, o, s);
        else launch_first<false>(P, block0, nblocks, F, d, o, s);
      } else {
        double *o = last ? static_cast<double *>(out) : w;
        if (curv) launch_first<true>(P, block0, nblocks, F, d, o, s);
        else launch_first<false>(P, block0, nblocks, F, d, o, s);
      }
    } else {
      // x2 of [rows0][nz][len][nx]: rows = rows0 nz, inner = nx;  x3 of [rows0][len][ny'][nx]: rows = rows0, inner = ny' nx
      const long rows = d == 1 ? rows0 * n[2] : rows0, inner = d == 1 ? n[0] : n[1] * n[0];
      if (last && single) launch_axis(in, rows, len, inner, static_cast<float *>(out), s);
      else launch_axis(in, rows, len, inner, last ? static_cast<double *>(out) : w, s);
    }
    in = w, work = w + rows0 * n[0] * n[1] * n[2];
  }
}

// doubles of work artemis_hip_reduce_fields_level takes: the blocks reduced at their own resolution, then what those passes need
long reduce_fields_level_work_elements(const int nx[3], int nblocks, int ncomp, int axes) {
  long own = static_cast<long>(nblocks) * (ncomp + 1);
  for (int d = 0; d < 3; ++d)
    if (!((axes >> d) & 1)) own *= nx[d];
  return own + reduce_fields_work_elements(nx, nblocks, ncomp, axes);
}

// The caller has checked axes, selection and shifts (|shift| <= 3, kept extents divisible by 2^shift); off[b]: element offset
// of block block0 + b in `out`.  The existing passes run unchanged with double output into the head of `work`; one resample
// launch per RESAMPLE_MAX_BLOCKS consecutive blocks follows on the same stream.
void launch_reduce_fields_level(const PackView &P, int block0, int nblocks, const FieldSelection &F, bool single, int axes, const int *shift,
                                const long *off, void *out, double *work, hipStream_t s) {
  if (nblocks == 0 || F.ncomp == 0) return;
  ResampleShape H;
  const int nx[3] = {P.ie - P.is + 1, P.je - P.js + 1, P.ke - P.ks + 1};
  H.rows = F.ncomp + 1, H.m = 0;
  long zin = 1;
  for (int d = 0; d < 3; ++d) {
    H.n[d] = ((axes >> d) & 1) ? 1 : nx[d];
    H.kept[d] = (!((axes >> d) & 1) && nx[d] > 1) ? 1 : 0;
    H.m += H.kept[d], zin *= H.n[d];
  }
  const long own = static_cast<long>(nblocks) * H.rows * zin;
  launch_reduce_fields(P, block0, nblocks, F, false, axes, work, work + own, s);
  ResampleBlocks B;
  B.n = 0, B.q0 = 0, B.tile0[0] = 0;
  auto flush = [&]() {
    if (B.n == 0) return;
    const long wg = B.tile0[B.n];
    const dim3 g(static_cast<unsigned>(grid_capped(wg < REDUCE_MAX_WG ? wg : REDUCE_MAX_WG)));
    if (single) hipLaunchKernelGGL((resample_reduced_kernel<float>), g, dim3(256), 0, s, work, H, B, static_cast<float *>(out));
    else hipLaunchKernelGGL((resample_reduced_kernel<double>), g, dim3(256), 0, s, work, H, B, static_cast<double *>(out));
    B.n = 0;
  };
  for (int b = 0; b < nblocks; ++b) {
    long oz = 1;
    for (int d = 0; d < 3; ++d) oz *= H.kept[d] ? (shift[b] >= 0 ? H.n[d] >> shift[b] : H.n[d] << -shift[b]) : H.n[d];
    const long tiles = (H.rows * oz + 255) / 256;
    if (B.n == RESAMPLE_MAX_BLOCKS || (B.n > 0 && B.tile0[B.n] + tiles > (1L << 30))) flush(); // (tile0 is an int)
    if (B.n == 0) B.q0 = b;
    B.shift[B.n] = static_cast<signed char>(shift[b]), B.off[B.n] = off[b];
    B.tile0[B.n + 1] = static_cast<int>(B.tile0[B.n] + tiles), B.n++;
  }
  flush();
}

} // namespace artemis
