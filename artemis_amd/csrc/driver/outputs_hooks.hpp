// What csrc/driver/outputs.cpp (the scheduler of the deck's <parthenon/output*> blocks) and driver.cpp need from each
// other.  The schedule lives with the C handle, not with the simulation state an adaptive mesh rebuilds.  Everything
// here throws std::exception on failure; none of it is part of the C ABI.
#pragma once
#include <string>
#include <vector>

#include "artemis_driver.h"

namespace artemis_out {

struct State; // parsed blocks, their next_time and counters (outputs.cpp)

struct Clock { // the driver's clock after a cycle and what a history row records next to it
  double time = 0.0, dt = 0.0, tlim = -1.0;
  long ncycle = 0, nlim = -1, nblocks_global = 0;
  int ns_gas = 0, ns_dust = 0, rank = 0;
};

// ---- driver.cpp ------------------------------------------------------------------------------------------------------
Clock clock_of(const artemis_sim_t *sim);
const std::string &deck_of(const artemis_sim_t *sim);
const std::vector<std::string> &overrides_of(const artemis_sim_t *sim);
State *&state_of(artemis_sim_t *sim);
const State *state_of(const artemis_sim_t *sim);
// 6 ns_gas + 4 ns_dust volume integrals of the current state, reduced over the ranks (collective): the device kernel
// (artemis_hip_history_sums) where the library has it, the host sum otherwise
int history_sums(artemis_sim_t *sim, double *out);

// ---- outputs.cpp -----------------------------------------------------------------------------------------------------
void destroy(State *st);
bool enabled(const State *st);
// earliest next_time of a block that is acted on; +infinity without one
double deadline(const State *st);
// Write every block that is due at the simulation's clock (time >= next_time) and move its next_time on.  history_only:
// called from inside the batched time loop, where a dump is not taken -- returns true if an `rst` block is still due, and
// the loop then hands control back to the handle, which calls again with history_only = false.  Collective.
bool write_due(artemis_sim_t *sim, bool history_only);
// The run has ended at tlim or nlim: every block once more, unless this cycle has written it already.  Collective.
void write_final(artemis_sim_t *sim);

} // namespace artemis_out
