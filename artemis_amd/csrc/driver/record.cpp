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
bool on_device() { return artemis_hip_record_tick != nullptr && artemis_hip_record_samples != nullptr; }
} // namespace

struct Recorder {
  long plan = -1;
  std::vector<int> codes;
  bool derived = false, single = false;
  long every = 1, capacity = 1, npoints = 0;
  int ncomp = 0;
  size_t row_bytes = 0; // ncomp * npoints * (4 or 8)
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
  CK(artemis_rt_stream_sync(stream), "sync");
  for (const artemis_record_head_t &h : heads) R.h_cycle.push_back(static_cast<long>(h.cycle)), R.h_time.push_back(h.time), R.h_dt.push_back(h.dt);
  c.rows = 0, c.slot = -1;
  upload_ctl(sim, R, c);
  R.on_dev = 0;
}

} // namespace

void begin_evolve(artemis_sim_t *sim, long ncycle) {
  State *st = state_of(sim);
  if (!attached(st)) return;
  void *stream = artemis_sample::stream_of(sim);
  for (auto &kv : st->recs) {
    Recorder &R = *kv.second;
    artemis_sample::located_plan(sim, R.plan);
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
