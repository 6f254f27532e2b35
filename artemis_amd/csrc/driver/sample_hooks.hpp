// What csrc/driver/sample.cpp (the sample plans of a handle: artemis_sim_sample_plan_*, include/artemis_driver.h) and
// driver.cpp need from each other.  The plans live with the C handle, not with the simulation state an adaptive mesh
// rebuilds.  Everything here throws std::exception on failure; none of it is part of the C ABI.
#pragma once
#include <vector>

#include "artemis_driver.h"
#include "artemis_hip.h"

namespace artemis_sample {

struct State; // the plans of a handle (sample.cpp)

// This rank's blocks as a point search sees them
struct Mesh {
  long epoch = 0; // moves whenever the block list is rebuilt (a remesh, a restore): a plan located on another one locates again
  int nb = 0, nx[3] = {1, 1, 1}, ng = 0;
  int active = 0; // bit d: blocks have more than one zone along direction d
  int ns_gas = 0, ns_dust = 0;
  double closed_hi[3] = {0.0, 0.0, 0.0}; // the mesh's xmax
  std::vector<double> bounds;            // [nb][6]: lo1 hi1 lo2 hi2 lo3 hi3, what artemis_sim_block_bounds returns
  std::vector<double> geom;              // [nb][6]: {xf0, dx} per direction, the host copy of the pack's table
};

// ---- driver.cpp ------------------------------------------------------------------------------------------------------
State *&state_of(artemis_sim_t *sim);
long epoch_of(const artemis_sim_t *sim);
Mesh mesh_of(const artemis_sim_t *sim);
artemis_pack_t pack_of(const artemis_sim_t *sim); // of the current buffer
void *stream_of(const artemis_sim_t *sim);
// the staging buffer of the field gathers, grown to at least `bytes`
void *stage_of(artemis_sim_t *sim, size_t bytes);
// a derived variable reads ghost zones: fill the ones a stage loop left for later (ghost zones only, the run's bits stay)
void fill_stale_ghosts(artemis_sim_t *sim);
// host fallback: the components of `codes` (component comp0[e] first) of every interior zone of local block b,
// [ncomp][nk][nj][ni], by the host loop of the gather
void host_components(artemis_sim_t *sim, int b, const std::vector<int> &codes, const std::vector<int> &comp0, int ncomp, std::vector<double> &vals);

// ---- sample.cpp ------------------------------------------------------------------------------------------------------
void destroy(State *st);
// what a recorder (record.cpp) uses of a plan: located on the current blocks first, if they changed.  The pointers stay
// valid until the plan locates again or is destroyed; the device ones are NULL on a host without the kernels.
struct PlanView {
  long npoints = 0;
  const int *loc_dev = nullptr;
  const long *order_dev = nullptr;
};
bool plan_exists(artemis_sim_t *sim, long id);
PlanView located_plan(artemis_sim_t *sim, long id);
// [ncomp][npoints] of `codes` at the plan's points into host_out: artemis_sim_sample_plan_values without the names
size_t plan_values(artemis_sim_t *sim, long id, const std::vector<int> &codes, bool single, void *host_out);

} // namespace artemis_sample
