// The shapes of a field output and the rules a request must keep, for the kernel ABI (abi.hip), the host driver and its
// output scheduler alike.  Plain C++17 on the host: no HIP types.  A request makes two independent choices -- integrate
// every block over the directions of `axes` (a mask, bit 0 x1, bit 1 x2, bit 2 x3; 0: none), and bring every block by a
// `shift` (its level - the level asked for; 0: none) to another zone size along the directions it keeps.
#pragma once
#include <string>
#include <vector>

namespace artemis_fields {

constexpr int kMaxShift = 3;
// (kernels.hpp, which every kernel unit includes and which therefore stays as it is, holds FIELDS_MAX_SHIFT, level_extent
//  and reduce_level_extent once more for the launchers: a known duplicate of the three lines below)
// zones of an extent n at this shift: an inactive direction (one zone) stays, s >= 1 halves s times, s <= -1 doubles
inline int level_extent(int n, int shift) { return n == 1 ? 1 : (shift >= 0 ? n >> shift : n << -shift); }
// ... of direction d after the reduction over axes: a reduced extent is 1 at every shift
inline int reduce_level_extent(int n, int shift, int axes, int d) { return ((axes >> d) & 1) ? 1 : level_extent(n, shift); }

// "" or what is wrong with a non-zero mask on blocks of nx zones; bad_mask: the caller's words for a mask outside 1 .. 7
inline std::string axes_rule(int axes, const int nx[3], const std::string &bad_mask) {
  if (axes < 1 || axes > 7) return bad_mask;
  for (int d = 0; d < 3; ++d)
    if (((axes >> d) & 1) && nx[d] < 2) return "x" + std::to_string(d + 1) + " has one zone and is not a direction to reduce";
  return "";
}
// "" or the rule a block of nx zones breaks at this shift along the directions it keeps ("shift 2, and its nx1 = ...");
// nx_word: how the caller names an extent
inline std::string shift_rule(int shift, int axes, const int nx[3], const char *nx_word = "nx") {
  if (shift > kMaxShift || shift < -kMaxShift) return "shift " + std::to_string(shift) + ", |shift| <= 3 is built";
  for (int d = 0; d < 3; ++d)
    if (shift > 0 && !((axes >> d) & 1) && nx[d] > 1 && nx[d] % (1 << shift) != 0)
      return "shift " + std::to_string(shift) + ", and its " + nx_word + std::to_string(d + 1) + " = " + std::to_string(nx[d]) +
             " is not divisible by " + std::to_string(1 << shift);
  return "";
}
// The layout of nblocks blocks one after the other, each [rows][nk'][nj'][ni']: off[b] the element offset of block b,
// off[nblocks] the total.  shift: one per block, or null for none.  Returns "" or shift_rule's text for the first block that
// breaks it, bad_block set to its index.
inline std::string block_offsets(const int nx[3], int rows, int axes, int nblocks, const int *shift, std::vector<long> &off,
                                 int &bad_block, const char *nx_word = "nx") {
  off.assign(static_cast<size_t>(nblocks) + 1, 0);
  for (int b = 0; b < nblocks; ++b) {
    const int s = shift ? shift[b] : 0;
    const std::string bad = shift_rule(s, axes, nx, nx_word);
    if (!bad.empty()) {
      bad_block = b;
      return bad;
    }
    long zones = 1;
    for (int d = 0; d < 3; ++d) zones *= reduce_level_extent(nx[d], s, axes, d);
    off[static_cast<size_t>(b) + 1] = off[static_cast<size_t>(b)] + zones * rows;
  }
  return "";
}

} // namespace artemis_fields
