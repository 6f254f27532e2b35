// Point location in a pack's blocks (include/artemis_hip_sample.h has the definition): the search table the host builds
// and the per-point search, one copy for the device kernel (kernels_sample.hip) and for the host driver's fallback loop
// (driver/sample.cpp).  Plain C++: double compares only, nothing here allocates or touches a device.
//
// The table: a lattice over the bounding box of the blocks, along every active direction cells of the SMALLEST block extent
// (halved no further than LOCATE_MAX_CELLS cells allow), and per cell the blocks that can hold a point of it, lowest index
// first.  On a mesh whose leaves tile the box on a 2:1 tree a cell lies in one block, so a point costs one cell index and
// one containment test; a pack of any other shape (gaps, overlaps) costs as many tests as blocks meet the cell.  Nothing
// depends on the cell index being exact: cell_of is a monotone function of the coordinate (one subtraction, one
// multiplication, one floor, the same IEEE operations on the host and on the device), a block is listed in every cell from
// cell_of(lo) to cell_of(the largest coordinate it can hold), and the containment test on the block's own doubles decides.
//
// Layout (position independent, the caller copies it to the device as it is):
//   Header | bounds [nblocks][6] doubles (lo1 hi1 lo2 hi2 lo3 hi3) | start [ncell + 1] ints | entries [nentries] ints
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>

#if defined(__HIPCC__)
#define ARTEMIS_LOCATE_HD __host__ __device__
#else
#define ARTEMIS_LOCATE_HD
#endif

namespace artemis_locate {

constexpr long LOCATE_MAGIC = 0x61727431'6c6f6331; // "art1loc1"
constexpr long LOCATE_MAX_CELLS = 1L << 22;

struct Header {
  long magic, nblocks, ncell, nentries;
  long n[3];     // cells along each direction (1 along an inactive one)
  long active;   // bit d: blocks have more than one zone along direction d
  double lo[3];  // lower corner of the lattice
  double inv[3]; // cells per unit length
};

ARTEMIS_LOCATE_HD inline bool finite_value(double x) { return (x - x) == 0.0; }

// the cell of coordinate x (finite) along direction d: monotone in x, clipped into the lattice
ARTEMIS_LOCATE_HD inline long cell_of(const Header &H, int d, double x) {
  const double top = static_cast<double>(H.n[d] - 1);
  double c = floor((x - H.lo[d]) * H.inv[d]);
  c = (c > 0.0) ? c : 0.0; // (a NaN product, 0 * inf, lands in cell 0: the containment test decides anyway)
  c = (c < top) ? c : top;
  return static_cast<long>(c);
}

inline size_t align8(size_t n) { return (n + 7) & ~static_cast<size_t>(7); }
inline size_t bounds_offset() { return align8(sizeof(Header)); }
inline size_t start_offset(long nblocks) { return bounds_offset() + static_cast<size_t>(nblocks) * 6 * sizeof(double); }
inline size_t entries_offset(long nblocks, long ncell) { return start_offset(nblocks) + align8(static_cast<size_t>(ncell + 1) * sizeof(int)); }

// The largest coordinate block bounds `bd` can hold along d: hi itself on the closed mesh edge, else the double below it
inline double last_held(const double *bd, const double *closed_hi, int d) {
  const double hi = bd[2 * d + 1];
  return (hi == closed_hi[d]) ? hi : std::nextafter(hi, -HUGE_VAL);
}

// "" and the header (lattice only), or what is wrong with the arguments
inline const char *plan(int nblocks, const double *bounds, const double *closed_hi, int active, Header &H) {
  if (nblocks < 1 || !bounds || !closed_hi) return "locate table: at least one block, its bounds and closed_hi are required";
  if (active < 0 || active > 7) return "locate table: active is a mask of x1 (1), x2 (2), x3 (4)";
  std::memset(&H, 0, sizeof H);
  H.magic = LOCATE_MAGIC, H.nblocks = nblocks, H.active = active;
  double ext[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
  for (int d = 0; d < 3; ++d) {
    H.n[d] = 1, H.lo[d] = 0.0, H.inv[d] = 0.0;
    if (!((active >> d) & 1)) continue;
    for (int b = 0; b < nblocks; ++b) {
      const double l = bounds[6 * b + 2 * d], h = bounds[6 * b + 2 * d + 1];
      if (!finite_value(l) || !finite_value(h) || !(h > l)) return "locate table: a block's bounds are not finite or not ordered";
      if (b == 0 || l < H.lo[d]) H.lo[d] = l;
      if (b == 0 || h > hi[d]) hi[d] = h;
      if (b == 0 || h - l < ext[d]) ext[d] = h - l;
    }
  }
  // cells of the smallest extent, doubled along the longest direction (in cells) until the lattice fits
  double cells[3] = {1.0, 1.0, 1.0};
  for (int d = 0; d < 3; ++d)
    if ((active >> d) & 1) {
      cells[d] = std::floor((hi[d] - H.lo[d]) / ext[d] + 0.5);
      if (!(cells[d] >= 1.0)) cells[d] = 1.0;
    }
  while (cells[0] * cells[1] * cells[2] > static_cast<double>(LOCATE_MAX_CELLS)) {
    int m = 0;
    for (int d = 1; d < 3; ++d)
      if (cells[d] > cells[m]) m = d;
    cells[m] = std::ceil(cells[m] / 2.0);
  }
  H.ncell = 1;
  for (int d = 0; d < 3; ++d) {
    H.n[d] = static_cast<long>(cells[d]);
    if ((active >> d) & 1) H.inv[d] = cells[d] / (hi[d] - H.lo[d]);
    H.ncell *= H.n[d];
  }
  return "";
}

// the cells a block is listed in: [c0[d], c1[d]] along every direction
inline void block_cells(const Header &H, const double *bd, const double *closed_hi, long c0[3], long c1[3]) {
  for (int d = 0; d < 3; ++d) {
    c0[d] = c1[d] = 0;
    if (!((H.active >> d) & 1)) continue;
    c0[d] = cell_of(H, d, bd[2 * d]);
    c1[d] = cell_of(H, d, last_held(bd, closed_hi, d));
    if (c1[d] < c0[d]) c1[d] = c0[d];
  }
}

// bytes of the table, 0 for arguments plan() refuses
inline size_t table_bytes(int nblocks, const double *bounds, const double *closed_hi, int active) {
  Header H;
  if (*plan(nblocks, bounds, closed_hi, active, H)) return 0;
  long entries = 0;
  for (int b = 0; b < nblocks; ++b) {
    long c0[3], c1[3];
    block_cells(H, bounds + 6 * b, closed_hi, c0, c1);
    entries += (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  }
  return entries_offset(nblocks, H.ncell) + align8(static_cast<size_t>(entries) * sizeof(int));
}

// fills `table` (table_bytes() bytes, 8-byte aligned); "" or what is wrong
inline const char *table_build(int nblocks, const double *bounds, const double *closed_hi, int active, void *table, size_t bytes) {
  Header H;
  const char *bad = plan(nblocks, bounds, closed_hi, active, H);
  if (*bad) return bad;
  if (!table || bytes < table_bytes(nblocks, bounds, closed_hi, active)) return "locate table: the buffer is smaller than artemis_hip_locate_table_bytes";
  char *base = static_cast<char *>(table);
  std::memset(base, 0, bytes);
  std::memcpy(base + bounds_offset(), bounds, static_cast<size_t>(nblocks) * 6 * sizeof(double));
  int *start = reinterpret_cast<int *>(base + start_offset(nblocks));
  int *entries = reinterpret_cast<int *>(base + entries_offset(nblocks, H.ncell));
  auto each_cell = [&](int b, auto &&f) {
    long c0[3], c1[3];
    block_cells(H, bounds + 6 * b, closed_hi, c0, c1);
    for (long k = c0[2]; k <= c1[2]; ++k)
      for (long j = c0[1]; j <= c1[1]; ++j)
        for (long i = c0[0]; i <= c1[0]; ++i) f((k * H.n[1] + j) * H.n[0] + i);
  };
  for (int b = 0; b < nblocks; ++b) each_cell(b, [&](long c) { start[c + 1]++; }); // counts, then their running sum
  for (long c = 0; c < H.ncell; ++c) start[c + 1] += start[c];
  H.nentries = start[H.ncell];
  // blocks in increasing order: every cell's list comes out lowest index first (start[c] moves on as the list fills)
  for (int b = 0; b < nblocks; ++b) each_cell(b, [&](long c) { entries[start[c]++] = b; });
  for (long c = H.ncell; c > 0; --c) start[c] = start[c - 1];
  start[0] = 0;
  std::memcpy(base, &H, sizeof H);
  return "";
}

// Block and zone of point x (include/artemis_hip_sample.h, steps 1 and 2).  geom: the pack's [nblocks][6] table of
// {xf0, dx} per direction; nx: interior zones of a block; nghost: the pack's ghost width.  loc = {block, k, j, i},
// all -1 for a point that is not found.  A table whose blocks the pack does not have (b >= nblocks) finds nothing there.
ARTEMIS_LOCATE_HD inline void locate_point(const void *table, const double *geom, int nblocks, const int nx[3], int nghost,
                                           const double closed_hi[3], const double x[3], int loc[4]) {
  const char *base = static_cast<const char *>(table);
  const Header &H = *reinterpret_cast<const Header *>(base);
  loc[0] = loc[1] = loc[2] = loc[3] = -1;
  if (H.magic != LOCATE_MAGIC) return;
  long c[3] = {0, 0, 0};
  for (int d = 0; d < 3; ++d)
    if ((H.active >> d) & 1) {
      if (!finite_value(x[d])) return;
      c[d] = cell_of(H, d, x[d]);
    }
  const size_t boff = (sizeof(Header) + 7) & ~static_cast<size_t>(7);
  const double *bounds = reinterpret_cast<const double *>(base + boff);
  const size_t soff = boff + static_cast<size_t>(H.nblocks) * 6 * sizeof(double);
  const int *start = reinterpret_cast<const int *>(base + soff);
  const int *entries = reinterpret_cast<const int *>(base + soff + ((static_cast<size_t>(H.ncell + 1) * sizeof(int) + 7) & ~static_cast<size_t>(7)));
  const long cell = (c[2] * H.n[1] + c[1]) * H.n[0] + c[0];
  int found = -1;
  for (int e = start[cell]; e < start[cell + 1] && found < 0; ++e) {
    const int b = entries[e];
    if (b < 0 || b >= nblocks) continue;
    const double *bd = bounds + 6 * static_cast<long>(b);
    bool in = true;
    for (int d = 0; d < 3; ++d)
      if ((H.active >> d) & 1) {
        const double lo = bd[2 * d], hi = bd[2 * d + 1];
        in = in && lo <= x[d] && (x[d] < hi || (x[d] == hi && hi == closed_hi[d]));
      }
    if (in) found = b;
  }
  if (found < 0) return;
  loc[0] = found;
  for (int d = 0; d < 3; ++d) {
    int z = 0;
    if ((H.active >> d) & 1) {
      const int n = nx[d], g = nghost;
      const double xf0 = geom[6 * static_cast<long>(found) + 2 * d], dx = geom[6 * static_cast<long>(found) + 2 * d + 1];
      auto Xf = [&](int t) { return xf0 + static_cast<double>(t) * dx; }; // one multiplication, one addition
      double guess = floor((x[d] - Xf(g)) / dx);
      guess = (guess > 0.0) ? guess : 0.0;
      guess = (guess < static_cast<double>(n - 1)) ? guess : static_cast<double>(n - 1);
      z = static_cast<int>(guess);
      while (z < n - 1 && Xf(g + z + 1) <= x[d]) ++z; // the last face at or below x ...
      while (z > 0 && Xf(g + z) > x[d]) --z;          // ... clipped into the interior at both ends
    }
    loc[3 - d] = z;
  }
}

} // namespace artemis_locate
