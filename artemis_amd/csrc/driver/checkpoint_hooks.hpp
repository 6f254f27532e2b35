// What csrc/driver/checkpoint.cpp needs from the simulation state of driver.cpp: the state's structs live in that
// translation unit, so the checkpoint code reaches them through these few calls.  All of them throw std::exception
// on failure; none is part of the C ABI.
#pragma once
#include <array>
#include <string>
#include <vector>

#include "artemis_driver.h"

namespace artemis_ckpt {

typedef std::array<int, 4> BlockKey; // level, lx1, lx2, lx3

// What a checkpoint's global header records about a run, and what a restored state is checked against
struct Meta {
  std::string deck, integrator;
  std::vector<std::string> overrides;
  double time = 0.0, dt = 0.0;
  long ncycle = 0, remeshes = 0, nblocks_global = 0;
  int rank = 0, nranks = 1;
  int mbnx[3] = {0, 0, 0}, ni = 0, nj = 0, nk = 0, nghost = 0, ndim = 0, ns_gas = 0, ns_dust = 0, coords = 0;
  int multilevel = 0, adaptive = 0, npart = 0;
  // Blocks narrower than the ghost width (a 2-zone block with nghost = 4): the slab a block sends its neighbour then
  // reaches into the block's own ghost zones of the buffer a stage writes to, which still hold what that ping-pong buffer
  // held stages ago.  The state of such a run is all three buffers and the index of the current one, so they are all
  // stored (nbuf = 3, buffer `base` first) and the restored run starts on the stored index; otherwise nbuf = 1, base = 0.
  int nbuf = 1, base = 0;
  std::vector<std::array<int, 5>> deref_count; // level, lx1, lx2, lx3, count
  std::vector<BlockKey> blocks;                // this rank's blocks in local order
};

void set_error(const std::string &msg);
// "" while the handle can be used (a failed lean remesh leaves it dead)
std::string dead_reason(const artemis_sim_t *sim);
const artemis_comm_t *comm_of(const artemis_sim_t *sim); // NULL for a single process
void describe(const artemis_sim_t *sim, Meta &m);

// Save side: complete the ghost zones the stage loop left alone and wait for the device; the n-body rows as they are
// (host rows [npart][7], then the device accumulators [npart][7] that have not been added to them yet -- kept apart so
// that a restored run adds them in the same order as an unbroken one)
void prepare_save(artemis_sim_t *sim, std::vector<double> &nbody_rows);
// whole primitive arrays of local block b: gas [6 ns][nk][nj][ni], dust [4 ns][nk][nj][ni]; which = 0: the current
// buffer, 1 and 2: the other two ping-pong buffers in cyclic order (zeros where a buffer has not been allocated yet)
void download_block(artemis_sim_t *sim, int b, int which, double *gas, double *dust);

// Restore side: a handle for deck + overrides on the given leaves (NULL: the mesh of the deck), problem generator run,
// no initial refinement passes
artemis_sim_t *create_on_leaves(const std::string &deck, const std::vector<std::string> &overrides,
                                const artemis_comm_t *comm, const std::vector<BlockKey> *leaves);
// into ping-pong buffer (base + which) % 3 of the restored state (base = 0 unless Meta::nbuf = 3)
void upload_block(artemis_sim_t *sim, int b, int base, int which, const double *gas, const double *dust);
void finish_restore(artemis_sim_t *sim, const Meta &m, const std::vector<double> &nbody_rows);

} // namespace artemis_ckpt
