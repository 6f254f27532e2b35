// Who runs a call of artemis_hip_stage_general: decided once, in stage_plan.hip, and executed by launch_stage_cell
// (kernels_stage_cell.hip).  The public queries (include/artemis_hip.h) report the same plan.
#pragma once
#include "pack_view.hpp"

namespace artemis {

// (the enumerator values are the codes of artemis_hip_stage_general_variant / _dust_variant)
enum class GasKernel : int { Cell = 0, RowMarch = 1, FusedCurv = 2, TileMarch = 3, PpmMarch = 4 };
enum class DustKernel : int { None = -1, Cell = 0, RowMarch = 1, TileMarch = 3 };

struct StagePlan {
  GasKernel gas;
  DustKernel dust;
  bool finish_in_march;       // the dust march couples the fluids by drag and writes both fluids' primitives itself
  bool to_cons;               // the stage kernels stop at the conserved state (cons0): drag or the caller finishes it
  int recon_gas, recon_dust;  // effective reconstruction (pcm folded in)
  bool grav_on;               // external gravity acts at g.time
  // what the caller still owes once the stage kernels are enqueued
  bool drag_finish;           // launch_drag_finish, or DragSource + SetAuxillaryFields + ConsToPrim where it declines
  bool dt_gas, dt_dust;       // launch_estimate_dt of the new state (no march has folded that fluid's limit in)
  int dust_code() const { return (dust == DustKernel::TileMarch && finish_in_march) ? 5 : static_cast<int>(dust); }
};

StagePlan plan_stage_general(const PackView &P, const artemis_stage_general_args_t &g, int recon_gas, int riemann_gas,
                             int recon_dust, int riemann_dust);

// The small facts every stage launcher and guard shares
bool offsets_fit(const PackView &P);                  // element offsets of a block in 32 bits: fewer than 2^29 zones
bool gravity_type_carried(const artemis_gravity_t *G); // none, or uniform / point / binary: what the kernels carry
bool gravity_active(const artemis_stage_general_args_t &g); // g.gravity inside its [tstart, tstop) window at g.time
inline int effective_recon(const artemis_stage_general_args_t &g, int recon) { return g.pcm ? ARTEMIS_PCM : recon; }

} // namespace artemis
