// Stand-in for <parthenon/package.hpp>: only the names the reference's leaf headers (artemis.hpp, geometry/,
// utils/fluxes/reconstruction/, utils/fluxes/riemann/) mention, with serial host meanings.  Test infrastructure:
// this is the project's own text; the reference's headers themselves are found through -I $(REFERENCE)/src.
#ifndef ORACLE_REF_STANDIN_PARTHENON_PACKAGE_HPP_
#define ORACLE_REF_STANDIN_PARTHENON_PACKAGE_HPP_

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>

#define KOKKOS_FUNCTION
#define KOKKOS_INLINE_FUNCTION inline
#define KOKKOS_FORCEINLINE_FUNCTION inline
#define KOKKOS_LAMBDA [=]
#define SQR(x) ((x) * (x))
#define PARTHENON_FAIL(msg) (std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, msg), std::abort())
#define PARTHENON_REQUIRE(cond, msg)                                                                                   \
  do {                                                                                                                 \
    if (!(cond)) PARTHENON_FAIL(msg);                                                                                  \
  } while (0)
#define DEFAULT_INNER_LOOP_PATTERN 0

namespace parthenon {

using Real = double;

enum CoordinateDirection { NODIR = -1, X0DIR = 0, X1DIR = 1, X2DIR = 2, X3DIR = 3 };
enum class TopologicalElement { CC = 0, F1 = 3, F2 = 4, F3 = 5 };
enum class AmrTag { derefine = -1, same = 0, refine = 1 };

// uniform Cartesian logical coordinates: face `i` of direction `dir` lies at x0 + i*dx
struct Coordinates_t {
  Real x0[3], dx[3];
  template <int dir>
  Real Xf(const int i) const {
    return x0[dir - 1] + i * dx[dir - 1];
  }
};

// one team of one thread
struct team_mbr_t {
  void team_barrier() const {}
};

// a [n0][n1] view of scratch that the caller owns
template <class T>
struct ScratchPad2D {
  T *data = nullptr;
  int n0 = 0, n1 = 0;
  ScratchPad2D() {}
  ScratchPad2D(T *data_, int n0_, int n1_) : data(data_), n0(n0_), n1(n1_) {}
  T &operator()(const int n, const int i) const { return data[static_cast<std::size_t>(n) * n1 + i]; }
};

template <class F>
inline void par_for_inner(int, const team_mbr_t &, const int il, const int iu, const F &f) {
  for (int i = il; i <= iu; ++i) f(i);
}

namespace variable_names {
template <bool REGEX>
struct base_t {
  template <class... Ts>
  base_t(Ts &&...) {}
};
} // namespace variable_names

// named by artemis.hpp's declarations only
class Mesh;
class TaskCollection;
template <class T>
class MeshBlockData;
template <class T>
class MeshData;
struct ParameterInput {
  int GetInteger(const std::string &, const std::string &) { return 1; }
};

namespace package {
namespace prelude {}
} // namespace package

} // namespace parthenon

#endif // ORACLE_REF_STANDIN_PARTHENON_PACKAGE_HPP_
