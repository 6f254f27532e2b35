// Host-side launchers of the HIP kernels (internal; the public surface is include/artemis_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include "fields_form.hpp"
#include "options.hpp"
#include "pack_view.hpp"
#include "stage_plan.hpp"

namespace artemis {
// How the calling thread's most recent march launch cut its work (artemis_hip_last_launch_cut): host-side values each
// march launcher notes as it launches -- nothing of it reaches a kernel.
struct LaunchCut {
  int launcher = 0;                                    // enum artemis_cut_launcher (0: no march launched yet)
  int chunk = 0, nchunk = 0;                           // planes (rows) per chunk and chunks of the main box
  int workgroups = 0, shell_workgroups = 0, redo_workgroups = 0;
};
extern thread_local LaunchCut g_last_cut; // (abi.hip)
inline void note_cut(int launcher, int chunk, int nchunk, long workgroups, long shell_workgroups = 0, long redo_workgroups = 0) {
  g_last_cut.launcher = launcher, g_last_cut.chunk = chunk, g_last_cut.nchunk = nchunk;
  g_last_cut.workgroups = static_cast<int>(workgroups), g_last_cut.shell_workgroups = static_cast<int>(shell_workgroups);
  g_last_cut.redo_workgroups = static_cast<int>(redo_workgroups);
}
// A tuning knob's value as a chunk length: at least one plane, at most `most` (a knob is a long; a value beyond the int
// range must not wrap into the chunk arithmetic)
inline int knob_chunk(long value, int most) { return static_cast<int>(value < 1 ? 1 : (value > most ? most : value)); }
// Workgroups of a grid-stride launch whose own choice is `own`: GRID_CAP, when set, lowers it (never below one), so that
// a small pack makes every workgroup take several trips of its stride loop -- same bits (the history sums, whose bits
// follow the number of partial rows by design, excepted)
inline long grid_capped(long own) {
  const long cap = opt(OPT_GRID_CAP);
  return (cap > 0 && cap < own) ? cap : own;
}
void launch_calculate_fluxes(const PackView &P, int fluid, int riemann, int recon, hipStream_t s);
void launch_apply_update(const PackView &P, double gam0, double gam1, double beta_dt, hipStream_t s);
void launch_flux_source(const PackView &P, int fluid, double dt, hipStream_t s);
void launch_set_aux(const PackView &P, hipStream_t s);
void launch_cons_to_prim(const PackView &P, hipStream_t s);
void launch_prim_to_cons(const PackView &P, hipStream_t s, bool ghosts_only = false);
void launch_deep_copy(const PackView &P, hipStream_t s);
void launch_estimate_dt(const PackView &P, int fluid, double cfl, double *dt_dev, hipStream_t s);
int launch_apply_bc(const PackView &P, const int *bc, const artemis_bc_params_t *par, hipStream_t s);
// kernels_sources.hip
void launch_external_gravity(const PackView &P, const artemis_gravity_t &G, double dt, hipStream_t s);
int nbody_grid(const PackView &P);
void launch_nbody_gravity(const PackView &P, const artemis_nbody_particle_t *pl_dev, int npart, double omf, double dt,
                          double *partial_dev, hipStream_t s);
bool nbody_force_sums_covers(const PackView &P);
void launch_nbody_force_sums(const PackView &P, const artemis_nbody_particle_t *pl_dev, int npart, double omf, double dt,
                             const double *dt_dev, double *partial_dev, double *force_dev, hipStream_t s);
void launch_shearing_box(const PackView &P, double omega, double qshear, double dt, hipStream_t s);
void launch_rotating_frame(const PackView &P, double omega, double dt, hipStream_t s);
void launch_cooling(const PackView &P, const artemis_cooling_t &C, double dt, hipStream_t s);
// dt_dev (optional DEVICE scalar) replaces dt
void launch_drag_source(const PackView &P, const artemis_drag_t &D, double dt, const double *dt_dev,
                        hipStream_t s);
bool launch_drag_finish(const PackView &P, const artemis_drag_t &D, double dt, const double *dt_dev,
                        hipStream_t s);
bool launch_drag_finish_cells(const PackView &P, const artemis_drag_t &D, double dt, const artemis_ml_fix_cell_t *cells,
                              int ncells, hipStream_t s);
bool drag_finish_in_march(const PackView &P, const artemis_drag_t &D);
long halo_count(const PackView &P, int face, int extended = 0);
int launch_halo(const PackView &P, int block, int face, double *buf, int unpack, int extended,
                hipStream_t s);
void invalidate_table_cache();
long plm_table_count(const PackView &P);
void launch_plm_table_fill(const PackView &P, double *tab, hipStream_t s);
// kernels_fused.hip
void launch_advance_dt(double *state, double tlim, int nstages, const double *beta, hipStream_t s);
void launch_wait_counter(unsigned *counter, unsigned target, unsigned *timeout_flag, hipStream_t s);
int launch_stage_fused(const PackView &P, const artemis_stage_args_t &a, int riemann, int recon,
                       hipStream_t s);
int launch_stage_fused_redo_shell(const PackView &P, const artemis_stage_args_t &a, int riemann, int recon, hipStream_t s);
int redo_totals(unsigned long long *out, int reset);
bool fused_flux_covers(const PackView &P, int recon);
int launch_flux_fused(const PackView &P, int riemann, int recon, hipStream_t s);
void launch_stage_fused_curv(const PackView &P, const artemis_stage_general_args_t &g, const StagePlan &pl, int riemann_gas,
                             hipStream_t s);
// kernels_curv.hip
// Chunks of an x3 march (kernels_curv.hip, the viscous source): a launch proceeds in rounds of `slots` resident
// workgroups and a half-empty last round costs a full one; every chunk pays `prime` priming trips (in units of a full
// trip: measured, a priming trip of the stage march costs about half a trip).  The number of chunks
// (each of at most cmax planes) with the best product of round fill and march efficiency; ties go to fewer chunks.
inline int pick_march_chunks(int planes, long tiles, long slots, int cmax, double prime) {
  int best = (planes + cmax - 1) / cmax;
  double score = -1.0;
  for (int n = (planes + cmax - 1) / cmax; n <= planes && n <= 64; ++n) {
    const int kc = (planes + n - 1) / n;
    if (kc < 4 && n > (planes + cmax - 1) / cmax) break;
    const int nchunk = (planes + kc - 1) / kc;
    const long wgs = tiles * nchunk;
    const double fill = static_cast<double>(wgs) / static_cast<double>(((wgs + slots - 1) / slots) * slots);
    const double sc = fill * kc / static_cast<double>(kc + prime);
    if (sc > score + 1e-9) score = sc, best = nchunk;
  }
  return best;
}
// fluid 1 with pl.finish_in_march: the dust march also runs DragSource + SetAuxillaryFields + ConsToPrim of both fluids (the
// gas march has left its conserved state in P.gas.cons0) and, with g.dt_dev, both fluids' timestep limits
void launch_stage_curv(const PackView &P, const artemis_stage_general_args_t &g, const StagePlan &pl, int fluid, int riemann,
                       hipStream_t s);
// kernels_ppm.hip: the PPM tile march (Cartesian 3-D, one gas species)
void launch_stage_ppm(const PackView &P, const artemis_stage_general_args_t &g, int riemann, hipStream_t s);
// kernels_diffusion.hip
void launch_zero_diffusion_flux(const PackView &P, hipStream_t s);
// overwrite: ZeroDiffusionFlux folded in (the flux arrays are overwritten on the face ranges)
size_t viscous_distance_count(const PackView &P);
void launch_viscous_distance_fill(const PackView &P, double *tab, hipStream_t s);
int launch_viscous_flux(const PackView &P, const artemis_diffusion_t &D, hipStream_t s, bool overwrite = false);
void launch_viscous_listed_faces(const PackView &P, const artemis_diffusion_t &D, const artemis_ml_face_box_t *boxes, int nboxes,
                                 const artemis_ml_fix_cell_t *cells, int ncells, hipStream_t s);
bool viscous_source_covers(const PackView &P);
void launch_viscous_source(const PackView &P, const artemis_diffusion_t &D, double dt, const double *dt_dev, double *const *out,
                           hipStream_t s);
void launch_thermal_flux(const PackView &P, const artemis_diffusion_t &D, hipStream_t s);
void launch_diffusion_update(const PackView &P, const artemis_diffusion_t &D, double dt, hipStream_t s);
void launch_timestep_all(const PackView &P, const artemis_diffusion_t *D, double cfl_gas, double cfl_dust, double *dt_dev,
                         hipStream_t s);
void launch_diffusion_dt(const PackView &P, const artemis_diffusion_t &D, double cfl, double *dt_dev,
                         hipStream_t s);
// kernels_stage_cell.hip
void launch_refine(const artemis_refine_t &r, int prolongate, hipStream_t s);
void launch_amr_criterion(const artemis_amr_criterion_t &a, int magnitude, hipStream_t s);
void launch_pack_criterion(const PackView &P, int var, int var_sie, int magnitude, double *maxima, hipStream_t s);
void launch_stage_epilogue(const PackView &P, const artemis_stage_general_args_t &g, hipStream_t s, bool to_cons = false);
void launch_stage_cell(const PackView &P, const artemis_stage_general_args_t &g, int recon_gas,
                       int riemann_gas, int recon_dust, int riemann_dust, hipStream_t s);
// kernels_stage2d.hip
void launch_ml_face_fluxes(const PackView &P, const artemis_stage_general_args_t &g, int recon_gas, int riemann_gas,
                           int recon_dust, int riemann_dust, const artemis_ml_face_box_t *boxes, int nboxes, hipStream_t s);
void launch_ml_stage_fixup(const PackView &P, const artemis_stage_general_args_t &g, int recon_gas, int riemann_gas,
                           int recon_dust, int riemann_dust, const artemis_ml_fix_cell_t *cells, int ncells, hipStream_t s);
void launch_stage2d(const PackView &P, const artemis_stage_general_args_t &g, const StagePlan &pl, int riemann_gas,
                    int riemann_dust, hipStream_t s);
// kernels_amr.hip
void launch_ml_exchange(const PackView &P, const artemis_ml_pack_t &ml, const artemis_ml_op_t *ops, int nops, double *sbuf,
                        const double *rbuf, hipStream_t s);
void launch_ml_flux_correction(const PackView &P, const artemis_ml_op_t *ops, int nops, double *sbuf, const double *rbuf,
                               hipStream_t s);
void launch_ml_restrict_halos(const PackView &P, const artemis_ml_pack_t &ml, const int *blocks, int nblocks, hipStream_t s);
void launch_ml_prolongate(const PackView &P, const artemis_ml_pack_t &ml, const artemis_ml_box_t *boxes, int nboxes,
                          hipStream_t s);
void launch_ml_floor_ghosts(const PackView &P, const int *blocks, int nblocks, hipStream_t s);
// kernels_history.hip: rows of partial sums the first launch writes (a function of the pack's shape alone)
long history_workgroups(const PackView &P);
void launch_history_sums(const PackView &P, double *sums, double *scratch, hipStream_t s);
// kernels_fields.hip: the variables of artemis_hip_pack_fields as a kernel argument -- entry e holds variable code[e] and
// its components start at component comp0[e] of a block's ncomp.  want_gas / want_dust: the fluids whose PLAIN codes
// (0 .. 11) are named; the derived codes (16 .. 19) have a pass and launches of their own (field_passes below)
constexpr int FIELDS_MAX_SEL = 32; // (two entries for each of the 16 variables; its size is part of every kernel's arguments)
struct FieldSelection {
  int nsel, ncomp, want_gas, want_dust;
  int code[FIELDS_MAX_SEL], comp0[FIELDS_MAX_SEL];
};
// The two passes of a selection, for every launcher and for the ABI's checks: `plain` as the plain kernels take it, `derived`
// the same entries with want_gas / want_dust naming the fluids whose DERIVED codes it holds; has_*: the pass has work
struct FieldPasses {
  FieldSelection plain, derived;
  bool has_plain, has_derived;
};
inline FieldPasses field_passes(const FieldSelection &F) {
  FieldPasses X;
  X.plain = X.derived = F;
  X.derived.want_gas = X.derived.want_dust = 0;
  for (int e = 0; e < F.nsel; ++e) {
    if (F.code[e] == ARTEMIS_VAR_GAS_DERIVED_DIVERGENCE || F.code[e] == ARTEMIS_VAR_GAS_DERIVED_VORTICITY) X.derived.want_gas = 1;
    if (F.code[e] == ARTEMIS_VAR_DUST_DERIVED_DIVERGENCE || F.code[e] == ARTEMIS_VAR_DUST_DERIVED_VORTICITY) X.derived.want_dust = 1;
  }
  X.has_plain = F.want_gas || F.want_dust, X.has_derived = X.derived.want_gas || X.derived.want_dust;
  return X;
}
void launch_pack_fields(const PackView &P, int block0, int nblocks, const FieldSelection &S, bool single, void *out, hipStream_t s);
// ... at a chosen refinement level: block block0 + b is restricted shift[b] times (volume-weighted, shift > 0) or replicated
// (shift < 0) and starts off[b] elements into `out`.  An extent of one zone is inactive: never halved or doubled.
constexpr int FIELDS_MAX_SHIFT = 3;
inline int level_extent(int n, int shift) { return n == 1 ? 1 : (shift >= 0 ? n >> shift : n << -shift); }
void launch_pack_fields_level(const PackView &P, int block0, int nblocks, const FieldSelection &S, bool single, const int *shift,
                              const long *off, void *out, hipStream_t s);
// kernels_reduce.hip: the same components integrated over the directions of `axes` (bit 0 x1, bit 1 x2, bit 2 x3; active
// directions only), a block leaving [ncomp + 1][nz'][ny'][nx'] with the volume last (artemis_hip.h has the definition).
// `work`: reduce_fields_work_elements doubles, what the passes before the last leave behind them.
long reduce_fields_work_elements(const int nx[3], int nblocks, int ncomp, int axes);
void launch_reduce_fields(const PackView &P, int block0, int nblocks, const FieldSelection &S, bool single, int axes, void *out, double *work,
                          hipStream_t s);
// ... brought to a chosen refinement level along the KEPT directions (active and not in `axes`): block b has shift[b] = its
// level - the level asked for, |shift| <= FIELDS_MAX_SHIFT; off[b]: element offset of block block0 + b in `out`
// (artemis_hip.h, artemis_hip_reduce_fields_level, has the definition).  `work`: reduce_fields_level_work_elements doubles.
inline int reduce_level_extent(int n, int shift, int axes, int d) {
  return ((axes >> d) & 1) ? 1 : level_extent(n, shift);
}
long reduce_fields_level_work_elements(const int nx[3], int nblocks, int ncomp, int axes);
void launch_reduce_fields_level(const PackView &P, int block0, int nblocks, const FieldSelection &S, bool single, int axes, const int *shift,
                                const long *off, void *out, double *work, hipStream_t s);
// ... and its inverse: the form of each fluid that the buffer holds (fields_form.hpp) written to the interior primitives
void launch_unpack_fields(const PackView &P, int block0, int nblocks, const FieldUnpack &U, bool single, const void *in, hipStream_t s);
} // namespace artemis
