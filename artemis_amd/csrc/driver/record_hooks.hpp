// What csrc/driver/record.cpp (the recorders of a handle: artemis_sim_record_*, include/artemis_driver.h) and driver.cpp need
// from each other.  A recorder appends, after every cycle that is due, a row {cycle, time, dt, the sample of a plan} to buffers
// on the device, from inside the time loop and its captured graphs.  The recorders live with the C handle next to the plans
// they refer to; what they reach of the state goes through sample_hooks.hpp.  Everything here throws std::exception on
// failure; none of it is part of the C ABI.
#pragma once
#include "artemis_driver.h"

namespace artemis_record {

struct State; // the recorders of a handle (record.cpp)

// ---- driver.cpp ------------------------------------------------------------------------------------------------------
State *&state_of(artemis_sim_t *sim);
// The n-body force rows of this rank: the host rows [npart][7] (what a flush adds the device accumulators to) and the
// accumulators on the device, NULL while the run keeps none there.  npart == 0: a deck without particles.
struct NBodyRows {
  int npart = 0;
  const double *host_rows = nullptr;
  const double *acc_dev = nullptr;
};
NBodyRows nbody_of(artemis_sim_t *sim);
// Host fallback of an integral recorder: out[1 + nwin][nq], the rank-local host sum behind artemis_sim_history_device (the
// same loop, the same order of additions, no reduction over the ranks) over every interior zone (set 0) and over the zones
// of zones[b][w] = {i0, i1, j0, j1, k0, k1} (set 1 + w; half-open, interior-relative).
void host_integrals(artemis_sim_t *sim, int nwin, const int *zones, double *out);

// ---- record.cpp: the time loop's side ----------------------------------------------------------------------------------
void destroy(State *st);
bool attached(const State *st); // a live recorder exists
bool plan_in_use(artemis_sim_t *sim, long plan_id);
// Before the first cycle of an artemis_sim_evolve call: the plans located, the device's cycle count set to the run's.
void begin_evolve(artemis_sim_t *sim, long ncycle);
// The cycles that can be queued before a due row would find some recorder's device buffer full, (capacity - rows on the
// device) * every minus the phase of `seen`, the smallest over the recorders: < 1 means drain first.
long room(const artemis_sim_t *sim);
// Wait for the stream, move every recorder's device rows to its host storage and empty the device buffers.
void drain(artemis_sim_t *sim);
// One completed cycle, for every recorder: the ghost fill a derived variable needs, the tick and the sample, queued on the
// run's stream -- capturable, nothing is read back.  tstate_dev: the device clock {time, dt, ...} of the unsynchronised
// loop (after artemis_hip_advance_dt), or NULL: the host's time and dt, by value.  The caller has made room.
void record_cycle(artemis_sim_t *sim, const double *tstate_dev, double time, double dt);
// The same cycle's bookkeeping alone: a replayed graph has launched what record_cycle queued when it was captured.
void count_cycle(artemis_sim_t *sim);

} // namespace artemis_record
