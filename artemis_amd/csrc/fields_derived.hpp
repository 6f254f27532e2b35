// The derived field outputs -- velocity divergence and vorticity of one species at one zone (include/artemis_hip.h,
// "derived variables", has the definition) -- as one copy of the two expressions for the device kernels
// (fields_device.hpp) and the host driver's gather (driver.cpp, host_block_components).  Usable from g++ and hipcc alike,
// like geometry_core.hpp.  Only the six face neighbours of the zone are read, and those of an inactive direction not at all.
#pragma once
#include "geometry_core.hpp"

namespace artemis {

struct DerivedZone {
  double div, w[3], vol; // divergence, vorticity 1-3, Coords::Volume of the zone
};

GDEV double face_area(const DCoords &c, int d, int f) { return d == 0 ? c.area1(f) : (d == 1 ? c.area2(f) : c.area3(f)); }

// vel(d, a, s): the stored velocity component d of the species at c + s e_a (s = -1, 0, +1; a does not matter at s = 0);
// coords(a, s): the Coords of that zone.  curv = false: the scale factors are the literal 1.0 (Cartesian packs).
template <class VEL, class COORDS>
GDEV DerivedZone derived_zone(bool curv, const bool act[3], VEL &&vel, COORDS &&coords) {
  const DCoords c0 = coords(0, 0);
  const double v0[3] = {vel(0, 0, 0), vel(1, 0, 0), vel(2, 0, 0)};
  double T[3] = {0.0, 0.0, 0.0};                                       // F_d^+ - F_d^-
  double D[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}; // D[a][d] = D_a[g_d]
  auto direction = [&](const int a) {
    if (!act[a]) return;
    const DCoords cm = coords(a, -1), cp = coords(a, +1);
    const double fp = face_area(c0, a, 1) * (0.5 * (v0[a] + vel(a, a, +1)));
    const double fm = face_area(c0, a, 0) * (0.5 * (vel(a, a, -1) + v0[a]));
    T[a] = fp - fm;
    double xm[3], xp[3];
    cm.centre(xm), cp.centre(xp);
    const double dxi = xp[a] - xm[a];
    const double hm[3] = {1.0, curv ? cm.hx2v() : 1.0, curv ? cm.hx3v() : 1.0};
    const double hp[3] = {1.0, curv ? cp.hx2v() : 1.0, curv ? cp.hx3v() : 1.0};
    for (int d = 0; d < 3; ++d)
      if (d != a) D[a][d] = (hp[d] * vel(d, a, +1) - hm[d] * vel(d, a, -1)) / dxi;
  };
  direction(0), direction(1), direction(2);
  const double h2 = curv ? c0.hx2v() : 1.0, h3 = curv ? c0.hx3v() : 1.0;
  DerivedZone z;
  z.vol = c0.volume();
  z.div = ((T[0] + T[1]) + T[2]) / z.vol;
  z.w[0] = (D[1][2] - D[2][1]) / (h2 * h3);
  z.w[1] = (D[2][0] - D[0][2]) / h3;
  z.w[2] = (D[0][1] - D[1][0]) / h2;
  return z;
}

} // namespace artemis
