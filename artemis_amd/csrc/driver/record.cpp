// Recorders of the host driver (include/artemis_driver.h: artemis_sim_record_*): a time series of the sample of a plan, one
// row {cycle, time, dt, values[ncomp][npoints]} after every cycle that is due, taken on the device inside the time loop
// (include/artemis_hip_sample.h has the two kernels' definition).  Plain C++ like the rest of the driver; the state is reached
// through sample_hooks.hpp and record_hooks.hpp.
//
// A recorder lives with the handle and refers to one of its plans.  It owns a control block, `capacity` heads and `capacity`
// rows on the device, and host storage that grows.  The time loop (artemis_sim_impl::evolve) calls record_cycle after every
// cycle -- inside the capture when one is open: the tick takes the row index, the cycle number and, in the unsynchronised
// loop, the clock from device memory, so a replayed graph records the right row -- and count_cycle for a replayed graph.
// The host counts along (`seen`, the rows on the device), which is all it needs to know how many cycles it may queue before a
// buffer is full: it asks room() and calls drain() at a batch boundary, the only synchronisation a recorder adds.  What the
// device counted is compared with the host's count at every drain; a dropped row is an error, not a gap.
//
// The kernel entry points are referenced weakly like the sample kernels: a host without them (the CPU stand-in of the tests)
// keeps seen, cycle and the rows itself and forms a row with the host loop of artemis_sim_sample_plan_values.
//
// A recorder of the second kind (artemis_sim_record_integrals_*) has no plan: its row is the history integrals of this rank's
// blocks, over the whole mesh and over up to seven windows, and optionally the n-body force sums
// (include/artemis_hip_record.h).  It is the same mechanism -- the same control block, tick, counting, room and drain -- with
// another payload: it owns the per-block index ranges of its windows, rebuilt when the mesh epoch moved as a plan locates
// again, the scratch of the partial sums, and the base array of the n-body rows.
#include <algorithm>
#include <cstddef>
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
#include "artemis_hip_record.h"
#include "artemis_hip_sample.h"
#include "artemis_rt.h"
#include "checkpoint_hooks.hpp"
#include "outputs_hooks.hpp"
#include "record_hooks.hpp"
#include "sample_hooks.hpp"

extern "C" int artemis_hip_record_tick(void *ctl_dev, void *head_dev, const double *tstate_dev, double time, double dt, long every, long capacity,
                                       void *stream) __attribute__((weak));
extern "C" int artemis_hip_record_samples(const artemis_pack_t *p, long npoints, const int *loc_dev, const long *order_dev, int nsel,
                                          const int *sel, int single, const void *ctl_dev, long capacity, void *rows_dev, void *stream)
    __attribute__((weak));
extern "C" size_t artemis_hip_record_integrals_scratch_bytes(const artemis_pack_t *p, int nwin) __attribute__((weak));
extern "C" int artemis_hip_record_integrals(const artemis_pack_t *p, int nwin, const int *window_zones_dev, double *scratch_dev,
                                            const void *ctl_dev, long capacity, double *rows_dev, void *stream) __attribute__((weak));
extern "C" int artemis_hip_record_nbody(const double *base_dev, const double *acc_dev, long n, const void *ctl_dev, long capacity,
                                        double *rows_dev, void *stream) __attribute__((weak));

namespace artemis_record {

namespace {
void CK(int rc, const char *what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + ": " + artemis_hip_last_error());
}
struct DevMem { // a device allocation of the recorder
  void *p = nullptr;
  void alloc(size_t bytes) {
    release();
    p = artemis_rt_malloc(std::max<size_t>(bytes, 16));
    if (!p) throw std::runtime_error(std::string("recorder: device allocation failed: ") + artemis_hip_last_error());
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
bool on_device() {
  return artemis_hip_record_tick != nullptr && artemis_hip_record_samples != nullptr && artemis_hip_record_integrals_scratch_bytes != nullptr &&
         artemis_hip_record_integrals != nullptr && artemis_hip_record_nbody != nullptr;
}
} // namespace

enum Kind { SAMPLES = 0, INTEGRALS = 1 };

struct Recorder {
  Kind kind = SAMPLES;
  long plan = -1;
  std::vector<int> codes;
  bool derived = false, single = false;
  long every = 1, capacity = 1, npoints = 0;
  int ncomp = 0;
  size_t row_bytes = 0; // ncomp * npoints * (4 or 8); integrals: (1 + nwin) * nq * 8
  // integrals: the windows [nwin][3][2] as given, their index ranges [nb][nwin][6] on the blocks of `epoch`, the n-body rows
  int nwin = 0, nq = 0;
  bool nbody = false;
  long epoch = -1;
  size_t nbody_bytes = 0; // 7 * npart * 8, 0 without n-body rows
  std::vector<double> windows, base_host;
  std::vector<int> zones;
  DevMem zones_dev, scratch, base, zero, rows2; // (zero: the accumulators of a run that has none on the device; rows2: the n-body rows)
  std::vector<char> h_nbody;
  // the host's count of what the device does
  long seen = 0, on_dev = 0; // cycles ticked; rows in the device buffers (on a host without the kernels: always 0)
  long cycle = 0;            // the run's cycle count (host path only; the device keeps its own)
  DevMem ctl, head, rows;
  // the rows drained so far, oldest first
  std::vector<long> h_cycle;
  std::vector<double> h_time, h_dt;
  std::vector<char> h_values;
};

struct State {
  long next_id = 0;
  std::map<long, std::unique_ptr<Recorder>> recs;
};

void destroy(State *st) { delete st; }
bool attached(const State *st) { return st && !st->recs.empty(); }

bool plan_in_use(artemis_sim_t *sim, long plan_id) {
  const State *st = state_of(sim);
  if (!st) return false;
  for (const auto &kv : st->recs)
    if (kv.second->plan == plan_id) return true;
  return false;
}

namespace {

Recorder &recorder_of(artemis_sim_t *sim, long id) {
  State *st = state_of(sim);
  if (!st || !st->recs.count(id)) throw std::runtime_error("recorder " + std::to_string(id) + " does not exist (closed, or never made)");
  return *st->recs[id];
}

void upload_ctl(artemis_sim_t *sim, Recorder &R, const artemis_record_ctl_t &c) {
  void *stream = artemis_sample::stream_of(sim);
  CK(artemis_rt_memcpy_h2d(R.ctl.p, &c, sizeof c, stream), "h2d");
  CK(artemis_rt_stream_sync(stream), "sync"); // (c is the caller's local)
}

// the device rows of one recorder to its host storage; the stream has been waited for
void drain_one(artemis_sim_t *sim, Recorder &R) {
  if (!on_device()) return;
  void *stream = artemis_sample::stream_of(sim);
  artemis_record_ctl_t c;
  CK(artemis_rt_memcpy_d2h(&c, R.ctl.p, sizeof c, stream), "d2h");
  CK(artemis_rt_stream_sync(stream), "sync");
  if (c.dropped != 0)
    throw std::runtime_error("recorder: " + std::to_string(c.dropped) + " rows found the device buffer full (the batches were sized wrongly)");
  if (c.rows != R.on_dev || c.seen != R.seen)
    throw std::runtime_error("recorder: the device counted " + std::to_string(c.seen) + " cycles and " + std::to_string(c.rows) +
                             " rows, the host " + std::to_string(R.seen) + " and " + std::to_string(R.on_dev));
  const size_t n = static_cast<size_t>(c.rows);
  if (n == 0) return;
  std::vector<artemis_record_head_t> heads(n);
  CK(artemis_rt_memcpy_d2h(heads.data(), R.head.p, n * sizeof(artemis_record_head_t), stream), "d2h");
  const size_t at = R.h_values.size();
  R.h_values.resize(at + n * R.row_bytes);
  if (R.row_bytes) CK(artemis_rt_memcpy_d2h(R.h_values.data() + at, R.rows.p, n * R.row_bytes, stream), "d2h");
  if (R.nbody_bytes) {
    const size_t at2 = R.h_nbody.size();
    R.h_nbody.resize(at2 + n * R.nbody_bytes);
    CK(artemis_rt_memcpy_d2h(R.h_nbody.data() + at2, R.rows2.p, n * R.nbody_bytes, stream), "d2h");
  }
  CK(artemis_rt_stream_sync(stream), "sync");
  for (const artemis_record_head_t &h : heads) R.h_cycle.push_back(static_cast<long>(h.cycle)), R.h_time.push_back(h.time), R.h_dt.push_back(h.dt);
  c.rows = 0, c.slot = -1;
  upload_ctl(sim, R, c);
  R.on_dev = 0;
}

// The zones of window w on block b: along every active direction the zones whose centre -- the midpoint of the two face
// positions Xf(t) = xf0 + t dx of the block's geom entries -- lies in [lo, hi); inactive directions take their one zone.
// The centres grow with t, so the zones form a range; a window that misses the block along any direction is {0, ...}.
void window_ranges(const artemis_sample::Mesh &m, int b, const double *win, int *z) {
  bool empty = false;
  for (int d = 0; d < 3; ++d) {
    int t0 = 0, t1 = m.nx[d];
    if (m.active & (1 << d)) {
      const double xf0 = m.geom[6 * b + 2 * d], dx = m.geom[6 * b + 2 * d + 1];
      auto centre = [&](int t) {
        const double a = xf0 + (m.ng + t) * dx, c = xf0 + (m.ng + t + 1) * dx;
        return 0.5 * (a + c);
      };
      t0 = 0;
      while (t0 < m.nx[d] && !(centre(t0) >= win[2 * d])) ++t0;
      t1 = t0;
      while (t1 < m.nx[d] && centre(t1) < win[2 * d + 1]) ++t1;
    }
    z[2 * d] = t0, z[2 * d + 1] = t1;
    empty = empty || t0 >= t1;
  }
  if (empty)
    for (int q = 0; q < 6; ++q) z[q] = 0;
}

// an integral recorder on the current blocks: the index ranges and the scratch, rebuilt when the mesh epoch moved (never
// inside a capture: a uniform run keeps its epoch through an evolve call, an adaptive one records between two calls)
void prepare_integrals(artemis_sim_t *sim, Recorder &R) {
  if (R.epoch == artemis_sample::epoch_of(sim)) return;
  const artemis_sample::Mesh m = artemis_sample::mesh_of(sim);
  R.zones.assign(static_cast<size_t>(m.nb) * R.nwin * 6, 0);
  for (int b = 0; b < m.nb; ++b)
    for (int w = 0; w < R.nwin; ++w) window_ranges(m, b, R.windows.data() + 6 * w, R.zones.data() + (static_cast<size_t>(b) * R.nwin + w) * 6);
  if (on_device()) {
    void *stream = artemis_sample::stream_of(sim);
    CK(artemis_rt_stream_sync(stream), "sync"); // (nothing queued still reads the old table or scratch)
    const artemis_pack_t p = artemis_sample::pack_of(sim);
    R.scratch.alloc(artemis_hip_record_integrals_scratch_bytes(&p, R.nwin));
    if (!R.zones.empty()) {
      R.zones_dev.alloc(R.zones.size() * sizeof(int));
      CK(artemis_rt_memcpy_h2d(R.zones_dev.p, R.zones.data(), R.zones.size() * sizeof(int), stream), "h2d");
      CK(artemis_rt_stream_sync(stream), "sync");
    }
  }
  R.epoch = m.epoch;
}

// the host's n-body rows to the recorder's base array on the device, when they differ from what it holds
void upload_base(artemis_sim_t *sim, Recorder &R) {
  if (!R.nbody_bytes || !on_device()) return;
  void *stream = artemis_sample::stream_of(sim);
  const NBodyRows nb = nbody_of(sim);
  const size_t n = 7 * static_cast<size_t>(nb.npart);
  // (the device copy is the last upload: rows that have not changed since -- every cycle of a loop whose accumulators live on
  //  the device -- cost a compare of 7 doubles per particle and no copy)
  if (R.base_host.size() == n && std::memcmp(R.base_host.data(), nb.host_rows, n * sizeof(double)) == 0) return;
  R.base_host.assign(nb.host_rows, nb.host_rows + n);
  CK(artemis_rt_memcpy_h2d(R.base.p, R.base_host.data(), R.nbody_bytes, stream), "h2d");
  CK(artemis_rt_stream_sync(stream), "sync");
}

} // namespace

void begin_evolve(artemis_sim_t *sim, long ncycle) {
  State *st = state_of(sim);
  if (!attached(st)) return;
  void *stream = artemis_sample::stream_of(sim);
  for (auto &kv : st->recs) {
    Recorder &R = *kv.second;
    if (R.kind == SAMPLES) artemis_sample::located_plan(sim, R.plan);
    else prepare_integrals(sim, R), upload_base(sim, R); // (the base again: a flush or a restore since the last call changed the rows)
    R.cycle = ncycle;
    if (on_device()) {
      const long long c = ncycle;
      CK(artemis_rt_memcpy_h2d(static_cast<char *>(R.ctl.p) + offsetof(artemis_record_ctl_t, cycle), &c, sizeof c, stream), "h2d");
      CK(artemis_rt_stream_sync(stream), "sync");
    }
  }
}

long room(const artemis_sim_t *sim) {
  const State *st = state_of(const_cast<artemis_sim_t *>(sim));
  long least = std::numeric_limits<long>::max();
  if (!st) return least;
  for (const auto &kv : st->recs) {
    const Recorder &R = *kv.second;
    const long rows_left = R.capacity - R.on_dev; // (a huge `every`, a user's "never", must not overflow the product)
    const long cycles = (rows_left > 0 && R.every > std::numeric_limits<long>::max() / rows_left) ? std::numeric_limits<long>::max()
                                                                                                 : rows_left * R.every;
    least = std::min(least, cycles - R.seen % R.every);
  }
  return least;
}

void drain(artemis_sim_t *sim) {
  State *st = state_of(sim);
  if (!attached(st) || !on_device()) return;
  CK(artemis_rt_stream_sync(artemis_sample::stream_of(sim)), "sync");
  for (auto &kv : st->recs) drain_one(sim, *kv.second);
}

void count_cycle(artemis_sim_t *sim) {
  State *st = state_of(sim);
  if (!st) return;
  for (auto &kv : st->recs) {
    Recorder &R = *kv.second;
    if (++R.seen % R.every == 0) ++R.on_dev;
  }
}

void record_cycle(artemis_sim_t *sim, const double *tstate_dev, double time, double dt) {
  State *st = state_of(sim);
  if (!attached(st)) return;
  void *stream = artemis_sample::stream_of(sim);
  if (on_device()) {
    for (auto &kv : st->recs) {
      Recorder &R = *kv.second;
      if (R.kind == INTEGRALS) {
        prepare_integrals(sim, R);
        // the loops that keep the clock on the host are the ones whose n-body task may add to the host rows directly,
        // and the adaptive loop's remesh hands flushed rows on: there the base is sent every cycle (nothing is captured)
        if (!tstate_dev) upload_base(sim, R);
        const artemis_pack_t p = artemis_sample::pack_of(sim);
        CK(artemis_hip_record_tick(R.ctl.p, R.head.p, tstate_dev, time, dt, R.every, R.capacity, stream), "record tick");
        CK(artemis_hip_record_integrals(&p, R.nwin, static_cast<const int *>(R.zones_dev.p), static_cast<double *>(R.scratch.p), R.ctl.p,
                                        R.capacity, static_cast<double *>(R.rows.p), stream),
           "record integrals");
        if (R.nbody_bytes) {
          const NBodyRows nb = nbody_of(sim);
          CK(artemis_hip_record_nbody(static_cast<const double *>(R.base.p), nb.acc_dev ? nb.acc_dev : static_cast<const double *>(R.zero.p),
                                      7L * nb.npart, R.ctl.p, R.capacity, static_cast<double *>(R.rows2.p), stream),
             "record nbody");
        }
        continue;
      }
      const artemis_sample::PlanView V = artemis_sample::located_plan(sim, R.plan);
      if (R.derived) artemis_sample::fill_stale_ghosts(sim);
      const artemis_pack_t p = artemis_sample::pack_of(sim);
      CK(artemis_hip_record_tick(R.ctl.p, R.head.p, tstate_dev, time, dt, R.every, R.capacity, stream), "record tick");
      CK(artemis_hip_record_samples(&p, V.npoints, V.loc_dev, V.order_dev, static_cast<int>(R.codes.size()), R.codes.data(), R.single ? 1 : 0, R.ctl.p,
                                    R.capacity, R.rows.p, stream),
         "record samples");
    }
    count_cycle(sim);
    return;
  }
  // a host without the kernels: the clock of the unsynchronised loop is read back, the row is formed by the host loop
  if (tstate_dev) {
    double h[2];
    CK(artemis_rt_memcpy_d2h(h, tstate_dev, sizeof h, stream), "d2h");
    CK(artemis_rt_stream_sync(stream), "sync");
    time = h[0], dt = h[1];
  }
  for (auto &kv : st->recs) {
    Recorder &R = *kv.second;
    ++R.cycle;
    if (++R.seen % R.every != 0) continue;
    R.h_cycle.push_back(R.cycle), R.h_time.push_back(time), R.h_dt.push_back(dt);
    const size_t at = R.h_values.size();
    R.h_values.resize(at + R.row_bytes);
    if (R.kind == INTEGRALS) {
      prepare_integrals(sim, R);
      if (R.row_bytes) host_integrals(sim, R.nwin, R.zones.data(), reinterpret_cast<double *>(R.h_values.data() + at));
      if (R.nbody_bytes) { // the host rows plus a download of the accumulators: the addition of a flush, nothing flushed
        const NBodyRows nb = nbody_of(sim);
        std::vector<double> row(nb.host_rows, nb.host_rows + 7 * static_cast<size_t>(nb.npart)), acc(row.size(), 0.0);
        if (nb.acc_dev) {
          CK(artemis_rt_stream_sync(stream), "sync");
          CK(artemis_rt_memcpy_d2h(acc.data(), nb.acc_dev, R.nbody_bytes, stream), "d2h");
          CK(artemis_rt_stream_sync(stream), "sync");
        }
        for (size_t q = 0; q < row.size(); ++q) row[q] += acc[q];
        const char *bytes = reinterpret_cast<const char *>(row.data());
        R.h_nbody.insert(R.h_nbody.end(), bytes, bytes + R.nbody_bytes);
      }
      continue;
    }
    if (R.row_bytes) artemis_sample::plan_values(sim, R.plan, R.codes, R.single, R.h_values.data() + at);
  }
}

} // namespace artemis_record

extern "C" {

long artemis_sim_record_create(artemis_sim_t *sim, long plan_id, int nvar, const char *const *names, long every, long capacity, int single) {
  using namespace artemis_record;
  try {
    if (!sim) throw std::runtime_error("record_create: no simulation");
    const std::string dead = artemis_ckpt::dead_reason(sim);
    if (!dead.empty()) throw std::runtime_error(dead);
    if (every < 1 || capacity < 1)
      throw std::runtime_error("record_create: every = " + std::to_string(every) + ", capacity = " + std::to_string(capacity) + " (both are at least 1)");
    if (!artemis_sample::plan_exists(sim, plan_id)) throw std::runtime_error("record_create: sample plan " + std::to_string(plan_id) + " does not exist");
    std::unique_ptr<Recorder> R(new Recorder());
    const artemis_out::Clock c = artemis_out::clock_of(sim);
    for (int v = 0; v < nvar; ++v) {
      const std::string name = (names && names[v]) ? names[v] : "";
      const int code = artemis_out::field_var_code(name);
      const int nc = code < 0 ? 0 : artemis_out::field_var_components(code, c.ns_gas, c.ns_dust);
      if (nc == 0) throw std::runtime_error("record: unknown variable " + name);
      R->codes.push_back(code);
      R->ncomp += nc;
      R->derived = R->derived || artemis_out::field_var_is_derived(code);
    }
    if (R->codes.size() > 32) throw std::runtime_error("record: at most 32 variables are taken");
    R->plan = plan_id, R->every = every, R->capacity = capacity, R->single = single != 0;
    R->npoints = artemis_sample::located_plan(sim, plan_id).npoints;
    R->row_bytes = static_cast<size_t>(R->ncomp) * static_cast<size_t>(R->npoints) * (R->single ? sizeof(float) : sizeof(double));
    R->cycle = c.ncycle;
    if (on_device()) {
      if (R->row_bytes && static_cast<size_t>(capacity) > std::numeric_limits<size_t>::max() / 2 / R->row_bytes)
        throw std::runtime_error("record_create: capacity times the bytes of a row overflows");
      R->ctl.alloc(sizeof(artemis_record_ctl_t));
      R->head.alloc(static_cast<size_t>(capacity) * sizeof(artemis_record_head_t));
      R->rows.alloc(static_cast<size_t>(capacity) * R->row_bytes);
      artemis_record_ctl_t z = {0, c.ncycle, 0, -1, 0};
      upload_ctl(sim, *R, z);
    }
    State *&st = state_of(sim);
    if (!st) st = new State();
    const long id = st->next_id++;
    st->recs[id] = std::move(R);
    return id;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

long artemis_sim_record_integrals_create(artemis_sim_t *sim, long every, long capacity, int nwin, const double *windows, int nbody) {
  using namespace artemis_record;
  try {
    if (!sim) throw std::runtime_error("record_integrals_create: no simulation");
    const std::string dead = artemis_ckpt::dead_reason(sim);
    if (!dead.empty()) throw std::runtime_error(dead);
    if (every < 1 || capacity < 1)
      throw std::runtime_error("record_integrals_create: every = " + std::to_string(every) + ", capacity = " + std::to_string(capacity) +
                               " (both are at least 1)");
    if (nwin < 0 || nwin > ARTEMIS_RECORD_MAX_WINDOWS || (nwin > 0 && !windows))
      throw std::runtime_error("record_integrals_create: nwin = " + std::to_string(nwin) + " (0 to 7 windows [nwin][3][2] are taken)");
    const artemis_sample::Mesh m = artemis_sample::mesh_of(sim);
    for (int w = 0; w < nwin; ++w)
      for (int d = 0; d < 3; ++d)
        if ((m.active & (1 << d)) && !(windows[6 * w + 2 * d] < windows[6 * w + 2 * d + 1]))
          throw std::runtime_error("record_integrals_create: window " + std::to_string(w) + " is empty along x" + std::to_string(d + 1) +
                                   " (lo < hi along every direction with more than one zone)");
    const NBodyRows nb = nbody_of(sim);
    if (nbody && nb.npart == 0) throw std::runtime_error("record_integrals_create: nbody rows on a deck without particles");
    std::unique_ptr<Recorder> R(new Recorder());
    const artemis_out::Clock c = artemis_out::clock_of(sim);
    R->kind = INTEGRALS, R->every = every, R->capacity = capacity, R->nwin = nwin, R->nbody = nbody != 0;
    R->nq = 6 * c.ns_gas + 4 * c.ns_dust;
    if (nwin) R->windows.assign(windows, windows + 6 * static_cast<size_t>(nwin));
    R->row_bytes = static_cast<size_t>(1 + nwin) * static_cast<size_t>(R->nq) * sizeof(double);
    R->nbody_bytes = R->nbody ? 7 * static_cast<size_t>(nb.npart) * sizeof(double) : 0;
    R->cycle = c.ncycle;
    if (static_cast<size_t>(capacity) > std::numeric_limits<size_t>::max() / 2 / (R->row_bytes + R->nbody_bytes + 1))
      throw std::runtime_error("record_integrals_create: capacity times the bytes of a row overflows");
    if (on_device()) {
      R->ctl.alloc(sizeof(artemis_record_ctl_t));
      R->head.alloc(static_cast<size_t>(capacity) * sizeof(artemis_record_head_t));
      R->rows.alloc(static_cast<size_t>(capacity) * R->row_bytes);
      if (R->nbody_bytes) {
        R->rows2.alloc(static_cast<size_t>(capacity) * R->nbody_bytes);
        R->base.alloc(R->nbody_bytes), R->zero.alloc(R->nbody_bytes);
        CK(artemis_rt_memset(R->zero.p, 0, R->nbody_bytes, artemis_sample::stream_of(sim)), "memset");
      }
      artemis_record_ctl_t z = {0, c.ncycle, 0, -1, 0};
      upload_ctl(sim, *R, z);
    }
    prepare_integrals(sim, *R);
    State *&st = state_of(sim);
    if (!st) st = new State();
    const long id = st->next_id++;
    st->recs[id] = std::move(R);
    return id;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

long artemis_sim_record_integrals_read(artemis_sim_t *sim, long id, long *cycle_out, double *time_out, double *dt_out, double *integrals_out,
                                       double *nbody_out, int clear) {
  using namespace artemis_record;
  try {
    if (!sim) throw std::runtime_error("record_integrals_read: no simulation");
    Recorder &R = recorder_of(sim, id);
    if (R.kind != INTEGRALS) throw std::runtime_error("record_integrals_read: recorder " + std::to_string(id) + " records samples");
    if (!cycle_out && !time_out && !dt_out && !integrals_out && !nbody_out) return R.nq;
    if (on_device()) {
      CK(artemis_rt_stream_sync(artemis_sample::stream_of(sim)), "sync");
      drain_one(sim, R);
    }
    const size_t n = R.h_cycle.size();
    if (cycle_out && n) std::memcpy(cycle_out, R.h_cycle.data(), n * sizeof(long));
    if (time_out && n) std::memcpy(time_out, R.h_time.data(), n * sizeof(double));
    if (dt_out && n) std::memcpy(dt_out, R.h_dt.data(), n * sizeof(double));
    if (integrals_out && !R.h_values.empty()) std::memcpy(integrals_out, R.h_values.data(), R.h_values.size());
    if (nbody_out && !R.h_nbody.empty()) std::memcpy(nbody_out, R.h_nbody.data(), R.h_nbody.size());
    if (clear) R.h_cycle.clear(), R.h_time.clear(), R.h_dt.clear(), R.h_values.clear(), R.h_nbody.clear();
    return R.nq;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

long artemis_sim_record_integrals_window_zones(artemis_sim_t *sim, long id, int *zones_out) {
  using namespace artemis_record;
  try {
    if (!sim) throw std::runtime_error("record_integrals_window_zones: no simulation");
    Recorder &R = recorder_of(sim, id);
    if (R.kind != INTEGRALS) throw std::runtime_error("record_integrals_window_zones: recorder " + std::to_string(id) + " records samples");
    prepare_integrals(sim, R);
    if (zones_out && !R.zones.empty()) std::memcpy(zones_out, R.zones.data(), R.zones.size() * sizeof(int));
    return R.nwin ? static_cast<long>(R.zones.size() / (6 * static_cast<size_t>(R.nwin))) : artemis_sample::mesh_of(sim).nb;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

long artemis_sim_record_rows(artemis_sim_t *sim, long id) {
  using namespace artemis_record;
  try {
    if (!sim) throw std::runtime_error("record_rows: no simulation");
    Recorder &R = recorder_of(sim, id);
    if (on_device()) {
      CK(artemis_rt_stream_sync(artemis_sample::stream_of(sim)), "sync");
      drain_one(sim, R);
    }
    return static_cast<long>(R.h_cycle.size());
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

long artemis_sim_record_read(artemis_sim_t *sim, long id, long *cycle_out, double *time_out, double *dt_out, void *values_out, int clear) {
  using namespace artemis_record;
  try {
    if (!sim) throw std::runtime_error("record_read: no simulation");
    Recorder &R = recorder_of(sim, id);
    if (R.kind != SAMPLES) throw std::runtime_error("record_read: recorder " + std::to_string(id) + " records integrals (artemis_sim_record_integrals_read)");
    if (!cycle_out && !time_out && !dt_out && !values_out) return R.ncomp;
    if (on_device()) {
      CK(artemis_rt_stream_sync(artemis_sample::stream_of(sim)), "sync");
      drain_one(sim, R);
    }
    const size_t n = R.h_cycle.size();
    if (cycle_out && n) std::memcpy(cycle_out, R.h_cycle.data(), n * sizeof(long));
    if (time_out && n) std::memcpy(time_out, R.h_time.data(), n * sizeof(double));
    if (dt_out && n) std::memcpy(dt_out, R.h_dt.data(), n * sizeof(double));
    if (values_out && !R.h_values.empty()) std::memcpy(values_out, R.h_values.data(), R.h_values.size());
    if (clear) R.h_cycle.clear(), R.h_time.clear(), R.h_dt.clear(), R.h_values.clear();
    return R.ncomp;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

int artemis_sim_record_destroy(artemis_sim_t *sim, long id) {
  using namespace artemis_record;
  try {
    if (!sim) throw std::runtime_error("record_destroy: no simulation");
    recorder_of(sim, id);
    CK(artemis_rt_stream_sync(artemis_sample::stream_of(sim)), "sync"); // (nothing queued still writes the buffers)
    state_of(sim)->recs.erase(id);
    return 0;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

} // extern "C"
