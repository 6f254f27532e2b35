// The array stages of the host fallback of a field gather (driver.cpp, artemis_sim_impl::gather_fields): what the kernels
// of kernels_fields.hip and kernels_reduce.hip do to one block, on vectors and extents, with every floating-point addition
// in the kernels' order.  No simulation state: a stand-alone host program can include and exercise this header.
// An array is [rows][n[2]][n[1]][n[0]] doubles; every stage takes it in `cur` and leaves its result there, n updated.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace artemis_fields_host {

typedef double Real;

// rows 0 .. ncomp - 1: N = V q, row ncomp: V -- what the reduction and the restriction tree add up
inline void weigh(const std::vector<Real> &q, const std::vector<Real> &vol, int ncomp, std::vector<Real> &cur) {
  const size_t zin = vol.size();
  cur.assign((static_cast<size_t>(ncomp) + 1) * zin, 0.0);
  for (int c = 0; c < ncomp; ++c)
    for (size_t z = 0; z < zin; ++z) cur[c * zin + z] = vol[z] * q[c * zin + z];
  std::copy(vol.begin(), vol.end(), cur.begin() + static_cast<size_t>(ncomp) * zin);
}

// Means on a coarser level: N and V each go s times up the tree of restriction.hpp:107-112, the pairs of the active
// directions (more than one zone) added x2 first, then x1, then x3; then N / V, which drops the row of V.
inline void restrict_means(std::vector<Real> &cur, int ncomp, int n[3], int s) {
  std::vector<Real> nxt;
  for (int m = 0; m < s; ++m) {
    const bool a[3] = {n[0] > 1, n[1] > 1, n[2] > 1};
    const int o[3] = {a[0] ? n[0] / 2 : 1, a[1] ? n[1] / 2 : 1, a[2] ? n[2] / 2 : 1};
    const size_t zi = static_cast<size_t>(n[0]) * n[1] * n[2], zo = static_cast<size_t>(o[0]) * o[1] * o[2];
    nxt.assign((static_cast<size_t>(ncomp) + 1) * zo, 0.0);
    for (int c = 0; c <= ncomp; ++c) {
      const Real *x = cur.data() + c * zi;
      auto child = [&](int K, int J, int I, int ok, int oj, int oi) -> Real { // 0.0: the offset-1 child of an inactive direction
        if ((ok && !a[2]) || (oj && !a[1]) || (oi && !a[0])) return 0.0;
        const int k = a[2] ? 2 * K + ok : K, j = a[1] ? 2 * J + oj : J, i = a[0] ? 2 * I + oi : I;
        return x[(static_cast<size_t>(k) * n[1] + j) * n[0] + i];
      };
      for (int K = 0; K < o[2]; ++K)
        for (int J = 0; J < o[1]; ++J)
          for (int I = 0; I < o[0]; ++I)
            nxt[c * zo + (static_cast<size_t>(K) * o[1] + J) * o[0] + I] =
                ((child(K, J, I, 0, 0, 0) + child(K, J, I, 0, 1, 0)) + (child(K, J, I, 0, 0, 1) + child(K, J, I, 0, 1, 1))) +
                ((child(K, J, I, 1, 0, 0) + child(K, J, I, 1, 1, 0)) + (child(K, J, I, 1, 0, 1) + child(K, J, I, 1, 1, 1)));
    }
    cur.swap(nxt);
    for (int d = 0; d < 3; ++d) n[d] = o[d];
  }
  const size_t zo = static_cast<size_t>(n[0]) * n[1] * n[2];
  for (int c = 0; c < ncomp; ++c)
    for (size_t z = 0; z < zo; ++z) cur[c * zo + z] = cur[c * zo + z] / cur[static_cast<size_t>(ncomp) * zo + z];
  cur.resize(static_cast<size_t>(ncomp) * zo);
}

// A finer level: every zone of `rows` rows repeated 2^r times along the directions of `along`, each value times `scale`
// (means: along = the active directions, scale = 1, which is exact; integrals: the kept directions and their even share)
inline void replicate(std::vector<Real> &cur, int rows, int n[3], int r, const bool along[3], Real scale, bool scaled) {
  const int rs[3] = {along[0] ? r : 0, along[1] ? r : 0, along[2] ? r : 0};
  const int o[3] = {n[0] << rs[0], n[1] << rs[1], n[2] << rs[2]};
  const size_t zi = static_cast<size_t>(n[0]) * n[1] * n[2], zo = static_cast<size_t>(o[0]) * o[1] * o[2];
  std::vector<Real> nxt(static_cast<size_t>(rows) * zo, 0.0);
  for (int c = 0; c < rows; ++c)
    for (int k = 0; k < o[2]; ++k)
      for (int j = 0; j < o[1]; ++j)
        for (int i = 0; i < o[0]; ++i) {
          const Real x = cur[c * zi + (static_cast<size_t>(k >> rs[2]) * n[1] + (j >> rs[1])) * n[0] + (i >> rs[0])];
          nxt[c * zo + (static_cast<size_t>(k) * o[1] + j) * o[0] + i] = scaled ? x * scale : x;
        }
  cur.swap(nxt);
  for (int d = 0; d < 3; ++d) n[d] = o[d];
}

// The sums over the directions of `axes`, x1 first: along x1 the 64-wide butterfly in chunks, the chunks in increasing
// order; along x2 and x3 sequential from the first element.  A reduced extent becomes 1.
inline void reduce_axes(std::vector<Real> &cur, int n[3], int axes) {
  std::vector<Real> nxt;
  for (int d = 0; d < 3; ++d) {
    if (!((axes >> d) & 1)) continue;
    // cur is [rows][len][inner]: x1 rows = (ncomp + 1) nz ny, inner = 1; x2 inner = nx'; x3 inner = ny' nx'
    const size_t len = static_cast<size_t>(n[d]), inner = d == 0 ? 1 : (d == 1 ? n[0] : static_cast<size_t>(n[0]) * n[1]);
    const size_t rows = cur.size() / (len * inner);
    nxt.assign(rows * inner, 0.0);
    for (size_t r = 0; r < rows; ++r)
      for (size_t x = 0; x < inner; ++x) {
        const Real *in = cur.data() + r * len * inner + x;
        Real acc = 0.0;
        if (d == 0) {
          for (size_t c0 = 0; c0 < len; c0 += 64) {
            Real w[64], y[64];
            for (size_t l = 0; l < 64; ++l) w[l] = (c0 + l < len) ? in[c0 + l] : 0.0;
            for (int m = 0; m < 6; ++m) {
              for (int l = 0; l < 64; ++l) y[l] = w[l] + w[l ^ (1 << m)];
              std::copy(y, y + 64, w);
            }
            acc = (c0 == 0) ? w[0] : acc + w[0];
          }
        } else {
          acc = in[0];
          for (size_t t = 1; t < len; ++t) acc = acc + in[t * inner];
        }
        nxt[r * inner + x] = acc;
      }
    cur.swap(nxt);
    n[d] = 1;
  }
}

// Integrals on a coarser level: x = x[0::2] + x[1::2] along each direction of `kept`, s times
inline void pair_sums(std::vector<Real> &cur, int n[3], int s, const bool kept[3]) {
  std::vector<Real> nxt;
  for (int d = 0; d < 3; ++d) {
    if (!kept[d]) continue;
    for (int t = 0; t < s; ++t) {
      const size_t inner = d == 0 ? 1 : (d == 1 ? n[0] : static_cast<size_t>(n[0]) * n[1]), half = static_cast<size_t>(n[d]) / 2;
      const size_t rows = cur.size() / (static_cast<size_t>(n[d]) * inner);
      nxt.assign(rows * half * inner, 0.0);
      for (size_t row = 0; row < rows; ++row)
        for (size_t h = 0; h < half; ++h)
          for (size_t x = 0; x < inner; ++x)
            nxt[(row * half + h) * inner + x] = cur[(row * 2 * half + 2 * h) * inner + x] + cur[(row * 2 * half + 2 * h + 1) * inner + x];
      cur.swap(nxt);
      n[d] = static_cast<int>(half);
    }
  }
}

// Integrals on a finer level: every output cell under a coarse zone takes the even share 2^(-r m) of it, m the number of
// kept directions -- an exact scaling
inline void share(std::vector<Real> &cur, int rows, int n[3], int r, const bool kept[3]) {
  const int m = (kept[0] ? 1 : 0) + (kept[1] ? 1 : 0) + (kept[2] ? 1 : 0);
  replicate(cur, rows, n, r, kept, std::ldexp(1.0, -r * m), m > 0);
}

// the gathered values as the caller's floats or doubles
inline void store(const std::vector<Real> &vals, bool single, void *out) {
  for (size_t e = 0; e < vals.size(); ++e) {
    if (single) static_cast<float *>(out)[e] = static_cast<float>(vals[e]);
    else static_cast<double *>(out)[e] = vals[e];
  }
}

} // namespace artemis_fields_host
