// Sample plans of the host driver (include/artemis_driver.h: artemis_sim_sample_plan_*): the value of field variables at
// arbitrary points, located in this rank's blocks and formed from the primitives on the device (include/artemis_hip_sample.h
// has the definition).  Plain C++ like the rest of the driver; the state is reached through sample_hooks.hpp.
//
// A plan lives with the handle.  It keeps the points, their locations {block, k, j, i} and the order of the points sorted by
// location -- on the device, with a host copy of the locations, which is what artemis_sim_sample_plan_locations returns and
// what the order is sorted from, once, when the plan is located -- and the mesh epoch it was located on.  When the block list
// has been rebuilt since (a remesh; a restore makes a new handle), the next call locates again by itself.  Values go
// through the bounded staging buffer of the gathers: one launch where [ncomp][npoints] fits it, else chunks of the sorted
// order whose values are put to the caller's places on the host.  Nothing of the run is written: primitives are read, and a
// derived variable first fills the ghost zones a stage loop left for later, as a gather does.
//
// The kernel entry points are referenced weakly like the other field kernels: a host that exports the driver's C ABI without
// them (the CPU stand-in of the tests) takes the host loops below -- the same search (csrc/locate_table.hpp is one copy for
// both) and the gather's host loop over the downloaded primitives, block by block in the sorted order.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "artemis_driver.h"
#include "artemis_hip.h"
#include "artemis_hip_sample.h"
#include "artemis_rt.h"
#include "../locate_table.hpp"
#include "../options.hpp"
#include "checkpoint_hooks.hpp"
#include "outputs_hooks.hpp"
#include "record_hooks.hpp"
#include "sample_hooks.hpp"

extern "C" int artemis_hip_locate_points(const artemis_pack_t *p, const void *table_dev, const double *closed_hi, long npoints,
                                         const double *points_dev, int *loc_dev, void *stream) __attribute__((weak));
extern "C" int artemis_hip_sample_fields(const artemis_pack_t *p, long npoints, const int *loc_dev, const long *order_dev, int nsel,
                                         const int *sel, int single, void *out_dev, void *stream) __attribute__((weak));

namespace artemis_sample {

namespace {
void CK(int rc, const char *what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + ": " + artemis_hip_last_error());
}
struct DevMem { // a device allocation of the plan
  void *p = nullptr;
  void alloc(size_t bytes) {
    release();
    p = artemis_rt_malloc(std::max<size_t>(bytes, 16));
    if (!p) throw std::runtime_error(std::string("sample plan: device allocation failed: ") + artemis_hip_last_error());
  }
  void release() {
    if (p) artemis_rt_free(p);
    p = nullptr;
  }
  ~DevMem() { release(); }
  DevMem() = default;
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
};
bool on_device() { return artemis_hip_locate_points != nullptr && artemis_hip_sample_fields != nullptr; }
} // namespace

struct Plan {
  long npoints = 0;
  long epoch = -1;            // the mesh epoch the locations belong to; -1: not located yet
  std::vector<double> points; // host copy [npoints][3] (the host loop locates from it; empty on the device path)
  std::vector<int> loc;       // [npoints][4] {block, k, j, i}
  std::vector<long> order;    // the points sorted by (block, k, j, i), points that were not found last
  int nx[3] = {1, 1, 1};      // zones of a block when the plan was located
  DevMem points_dev, loc_dev, order_dev, chunk_dev;
};

struct State {
  long next_id = 0;
  std::map<long, std::unique_ptr<Plan>> plans;
};

void destroy(State *st) { delete st; }

namespace {

Plan &plan_of(artemis_sim_t *sim, long id) {
  State *st = state_of(sim);
  if (!st || !st->plans.count(id)) throw std::runtime_error("sample plan " + std::to_string(id) + " does not exist (closed, or never made)");
  return *st->plans[id];
}

// Locations and order of the plan on the current block list
void locate(artemis_sim_t *sim, Plan &P) {
  const Mesh M = mesh_of(sim);
  const long n = P.npoints;
  P.loc.assign(static_cast<size_t>(4 * n), -1);
  for (int d = 0; d < 3; ++d) P.nx[d] = M.nx[d];
  if (n > 0 && M.nb > 0) {
    const size_t tbytes = artemis_locate::table_bytes(M.nb, M.bounds.data(), M.closed_hi, M.active);
    std::vector<double> table((tbytes + sizeof(double) - 1) / sizeof(double));
    const char *bad = artemis_locate::table_build(M.nb, M.bounds.data(), M.closed_hi, M.active, table.data(), tbytes);
    if (*bad || tbytes == 0) throw std::runtime_error(*bad ? bad : "locate table: no table for these blocks");
    if (on_device()) {
      const artemis_pack_t p = pack_of(sim);
      void *stream = stream_of(sim);
      DevMem table_dev;
      table_dev.alloc(tbytes);
      CK(artemis_rt_memcpy_h2d(table_dev.p, table.data(), tbytes, stream), "h2d");
      CK(artemis_hip_locate_points(&p, table_dev.p, M.closed_hi, n, static_cast<const double *>(P.points_dev.p), static_cast<int *>(P.loc_dev.p), stream),
         "locate points");
      CK(artemis_rt_memcpy_d2h(P.loc.data(), P.loc_dev.p, static_cast<size_t>(n) * 4 * sizeof(int), stream), "d2h");
      CK(artemis_rt_stream_sync(stream), "sync"); // (the table goes out of scope)
    } else {
      for (long q = 0; q < n; ++q)
        artemis_locate::locate_point(table.data(), M.geom.data(), M.nb, M.nx, M.ng, M.closed_hi, P.points.data() + 3 * q, P.loc.data() + 4 * q);
    }
  }
  // the order: by the linear index of the zone in the block list, ties (points of one zone) by the caller's index
  std::vector<std::pair<int64_t, long>> key(static_cast<size_t>(n));
  for (long q = 0; q < n; ++q) {
    const int *l = P.loc.data() + 4 * q;
    key[q].first = l[0] < 0 ? std::numeric_limits<int64_t>::max() : ((static_cast<int64_t>(l[0]) * M.nx[2] + l[1]) * M.nx[1] + l[2]) * M.nx[0] + l[3];
    key[q].second = q;
  }
  std::sort(key.begin(), key.end());
  P.order.resize(static_cast<size_t>(n));
  for (long q = 0; q < n; ++q) P.order[q] = key[q].second;
  if (on_device() && n > 0) {
    void *stream = stream_of(sim);
    CK(artemis_rt_memcpy_h2d(P.order_dev.p, P.order.data(), static_cast<size_t>(n) * sizeof(long), stream), "h2d");
    CK(artemis_rt_stream_sync(stream), "sync");
  }
  P.epoch = M.epoch;
}

void ensure_located(artemis_sim_t *sim, Plan &P) {
  if (P.epoch != epoch_of(sim)) locate(sim, P);
}

void store(double v, bool single, void *out, size_t at) {
  if (single) static_cast<float *>(out)[at] = static_cast<float>(v);
  else static_cast<double *>(out)[at] = v;
}

// [ncomp][npoints] of the variables at the plan's points; returns the bytes
size_t values(artemis_sim_t *sim, Plan &P, const std::vector<int> &codes, bool single, void *host_out) {
  const Mesh head = mesh_of(sim); // (species counts; the blocks are taken again below, after a relocation)
  std::vector<int> comp0;
  int ncomp = 0;
  bool derived = false;
  for (const int code : codes) {
    comp0.push_back(ncomp);
    ncomp += artemis_out::field_var_components(code, head.ns_gas, head.ns_dust);
    derived = derived || artemis_out::field_var_is_derived(code);
  }
  const long n = P.npoints;
  const size_t esz = single ? sizeof(float) : sizeof(double), total = static_cast<size_t>(ncomp) * static_cast<size_t>(n) * esz;
  if (!host_out || total == 0) return total;
  ensure_located(sim, P);
  if (derived) fill_stale_ghosts(sim);
  const int nsel = static_cast<int>(codes.size());
  if (on_device()) {
    const artemis_pack_t p = pack_of(sim);
    void *stream = stream_of(sim);
    const long mb = artemis::opt(artemis::OPT_FIELDS_STAGE_MB);
    const size_t cap = static_cast<size_t>(mb > 0 ? mb : 256) << 20;
    if (total <= cap) {
      void *stage = stage_of(sim, total);
      CK(artemis_hip_sample_fields(&p, n, static_cast<const int *>(P.loc_dev.p), static_cast<const long *>(P.order_dev.p), nsel, codes.data(),
                                   single ? 1 : 0, stage, stream), "sample fields");
      CK(artemis_rt_memcpy_d2h(host_out, stage, total, stream), "d2h");
      CK(artemis_rt_stream_sync(stream), "sync");
      return total;
    }
    // chunks of the sorted order: their locations one after the other, their values put to the caller's places here
    const long per = std::max<long>(1, static_cast<long>(cap / (static_cast<size_t>(ncomp) * esz)));
    std::vector<int> cl(static_cast<size_t>(4 * per));
    std::vector<char> got(static_cast<size_t>(ncomp) * per * esz);
    P.chunk_dev.alloc(static_cast<size_t>(per) * 4 * sizeof(int));
    void *stage = stage_of(sim, got.size());
    for (long t0 = 0; t0 < n; t0 += per) {
      const long m = std::min(per, n - t0);
      for (long t = 0; t < m; ++t) std::memcpy(cl.data() + 4 * t, P.loc.data() + 4 * P.order[t0 + t], 4 * sizeof(int));
      CK(artemis_rt_memcpy_h2d(P.chunk_dev.p, cl.data(), static_cast<size_t>(m) * 4 * sizeof(int), stream), "h2d");
      CK(artemis_hip_sample_fields(&p, m, static_cast<const int *>(P.chunk_dev.p), nullptr, nsel, codes.data(), single ? 1 : 0, stage, stream),
         "sample fields");
      CK(artemis_rt_memcpy_d2h(got.data(), stage, static_cast<size_t>(ncomp) * m * esz, stream), "d2h");
      CK(artemis_rt_stream_sync(stream), "sync"); // (the next chunk reuses the buffers)
      for (int c = 0; c < ncomp; ++c)
        for (long t = 0; t < m; ++t)
          std::memcpy(static_cast<char *>(host_out) + (static_cast<size_t>(c) * n + P.order[t0 + t]) * esz, got.data() + (static_cast<size_t>(c) * m + t) * esz, esz);
    }
    P.chunk_dev.release();
    return total;
  }
  // host loop: the sorted order visits a block's points together, so a block is formed once
  const size_t zones = static_cast<size_t>(P.nx[0]) * P.nx[1] * P.nx[2];
  std::vector<double> vals;
  int have = -1;
  for (long t = 0; t < n; ++t) {
    const long q = P.order[t];
    const int *l = P.loc.data() + 4 * q;
    if (l[0] < 0) {
      for (int c = 0; c < ncomp; ++c) store(std::numeric_limits<double>::quiet_NaN(), single, host_out, static_cast<size_t>(c) * n + q);
      continue;
    }
    if (l[0] != have) host_components(sim, l[0], codes, comp0, ncomp, vals), have = l[0];
    const size_t z = (static_cast<size_t>(l[1]) * P.nx[1] + l[2]) * P.nx[0] + l[3];
    for (int c = 0; c < ncomp; ++c) store(vals[c * zones + z], single, host_out, static_cast<size_t>(c) * n + q);
  }
  return total;
}

} // namespace

bool plan_exists(artemis_sim_t *sim, long id) {
  State *st = state_of(sim);
  return st && st->plans.count(id) != 0;
}
PlanView located_plan(artemis_sim_t *sim, long id) {
  Plan &P = plan_of(sim, id);
  ensure_located(sim, P);
  PlanView v;
  v.npoints = P.npoints;
  v.loc_dev = static_cast<const int *>(P.loc_dev.p), v.order_dev = static_cast<const long *>(P.order_dev.p);
  return v;
}
size_t plan_values(artemis_sim_t *sim, long id, const std::vector<int> &codes, bool single, void *host_out) {
  return values(sim, plan_of(sim, id), codes, single, host_out);
}

} // namespace artemis_sample

extern "C" {

long artemis_sim_sample_plan_create(artemis_sim_t *sim, long npoints, const double *points_host) {
  using namespace artemis_sample;
  try {
    if (!sim) throw std::runtime_error("sample_plan_create: no simulation");
    const std::string dead = artemis_ckpt::dead_reason(sim);
    if (!dead.empty()) throw std::runtime_error(dead);
    if (npoints < 0 || (npoints > 0 && !points_host)) throw std::runtime_error("sample_plan_create: npoints >= 0 points of three doubles are taken");
    std::unique_ptr<Plan> P(new Plan());
    P->npoints = npoints;
    if (on_device() && npoints > 0) {
      void *stream = stream_of(sim);
      P->points_dev.alloc(static_cast<size_t>(npoints) * 3 * sizeof(double));
      P->loc_dev.alloc(static_cast<size_t>(npoints) * 4 * sizeof(int));
      P->order_dev.alloc(static_cast<size_t>(npoints) * sizeof(long));
      CK(artemis_rt_memcpy_h2d(P->points_dev.p, points_host, static_cast<size_t>(npoints) * 3 * sizeof(double), stream), "h2d");
      CK(artemis_rt_stream_sync(stream), "sync"); // (the caller's array is free again)
    } else {
      P->points.assign(points_host, points_host + 3 * npoints);
    }
    locate(sim, *P);
    State *&st = state_of(sim);
    if (!st) st = new State();
    const long id = st->next_id++;
    st->plans[id] = std::move(P);
    return id;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

int artemis_sim_sample_plan_locations(artemis_sim_t *sim, long id, int *loc_host) {
  using namespace artemis_sample;
  try {
    if (!sim) throw std::runtime_error("sample_plan_locations: no simulation");
    const std::string dead = artemis_ckpt::dead_reason(sim);
    if (!dead.empty()) throw std::runtime_error(dead);
    Plan &P = plan_of(sim, id);
    ensure_located(sim, P);
    if (loc_host && P.npoints > 0) std::memcpy(loc_host, P.loc.data(), static_cast<size_t>(P.npoints) * 4 * sizeof(int));
    return 0;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

long artemis_sim_sample_plan_values(artemis_sim_t *sim, long id, int nvar, const char *const *names, int single, void *host_out) {
  using namespace artemis_sample;
  try {
    if (!sim) throw std::runtime_error("sample_plan_values: no simulation");
    const std::string dead = artemis_ckpt::dead_reason(sim);
    if (!dead.empty()) throw std::runtime_error(dead);
    Plan &P = plan_of(sim, id);
    const artemis_out::Clock c = artemis_out::clock_of(sim);
    std::vector<int> codes;
    long ncomp = 0;
    for (int v = 0; v < nvar; ++v) {
      const std::string name = (names && names[v]) ? names[v] : "";
      const int code = artemis_out::field_var_code(name);
      const int nc = code < 0 ? 0 : artemis_out::field_var_components(code, c.ns_gas, c.ns_dust);
      if (nc == 0) throw std::runtime_error("sample: unknown variable " + name);
      codes.push_back(code);
      ncomp += nc;
    }
    if (static_cast<int>(codes.size()) > 32) throw std::runtime_error("sample: at most 32 variables are taken");
    const size_t bytes = values(sim, P, codes, single != 0, host_out);
    return host_out ? ncomp : static_cast<long>(bytes);
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

int artemis_sim_sample_plan_destroy(artemis_sim_t *sim, long id) {
  using namespace artemis_sample;
  try {
    if (!sim) throw std::runtime_error("sample_plan_destroy: no simulation");
    plan_of(sim, id);
    if (artemis_record::plan_in_use(sim, id)) throw std::runtime_error("sample plan " + std::to_string(id) + " is in use by a recorder: close the recorder first");
    state_of(sim)->plans.erase(id);
    return 0;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

} // extern "C"
