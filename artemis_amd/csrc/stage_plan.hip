// Who runs a general stage (host code only; DESIGN.md "Who runs a general stage").  Top to bottom: the facts every launcher
// shares; what each kernel CAN take, one predicate per kernel, none of which reads a switch or knows of another kernel;
// and plan_stage_general, which alone reads the path-selection switches of this entry point and holds the precedence.
#include "stage_plan.hpp"

#include "kernels.hpp"
#include "options.hpp"

namespace artemis {

// ---- shared facts -----------------------------------------------------------------------------------------------
// the marches address cells with 32-bit byte offsets (fused_device.hpp gld / gst: SGPR base + one VGPR offset per cell)
bool offsets_fit(const PackView &P) { return static_cast<long>(P.nk) * P.nj * P.ni < (1L << 29); }
bool gravity_type_carried(const artemis_gravity_t *G) {
  return !G || G->type == ARTEMIS_GRAVITY_UNIFORM || G->type == ARTEMIS_GRAVITY_POINT || G->type == ARTEMIS_GRAVITY_BINARY;
}
bool gravity_active(const artemis_stage_general_args_t &g) {
  return g.gravity && (g.time >= g.gravity->tstart) && (g.time < g.gravity->tstop);
}

// ---- what each kernel can take ------------------------------------------------------------------------------------
// The PPM tile march (kernels_ppm.hip): one gas species alone on Cartesian 3-D blocks, PPM4 with its three ghost
// zones, every ghost zone filled by the caller, none of the optional tasks, no fix-up to follow.
static bool ppm_march_takes(const PackView &P, const artemis_stage_general_args_t &g, int recon_gas) {
  if (P.coords != ARTEMIS_CARTESIAN || P.ndim != 3 || P.gas.ns != 1 || P.dust.ns != 0) return false;
  if (effective_recon(g, recon_gas) != ARTEMIS_PPM || P.ng < 3 || !offsets_fit(P)) return false;
  if (g.gravity || g.rf_omega != 0.0 || g.drag || g.diffusion || g.cooling || g.nbody_n) return false;
  return g.defer_finish == 0 && g.strat_faces == 0;
}

// The 2-D row march (kernels_stage2d.hip): Cartesian gas with up to two dust species that share its reconstruction,
// the pointwise sources, simple_dust drag without damp_to_visc, the stratified conditions on all four faces of ONE
// block.  (The recon codes are the pack's own: a PPM pack stays off it on its PCM predictor stage too.)
static bool row_march_takes(const PackView &P, const artemis_stage_general_args_t &g, int recon_gas, int recon_dust, int riemann_dust) {
  if (P.coords != ARTEMIS_CARTESIAN || P.ndim != 2 || P.ng < 2 || !offsets_fit(P) || P.gas.ns != 1 || P.dust.ns > 2) return false;
  if (recon_gas == ARTEMIS_PPM || (P.dust.ns && (recon_dust != recon_gas || riemann_dust == ARTEMIS_HLLC))) return false;
  if (g.diffusion || g.cooling || g.nbody_n || g.defer_finish) return false;
  if (g.strat_faces && (g.strat_faces != 15 || P.nb != 1 || P.ie - P.is < 1)) return false;
  if (g.drag && (g.drag->type != ARTEMIS_DRAG_SIMPLE_DUST || g.drag->damp_visc || P.dust.ns == 0)) return false;
  return gravity_type_carried(g.gravity);
}

// The tile march (kernels_curv.hip), gas: one species, PCM / PLM, the pointwise tasks the kernel folds in; diffusion
// only as artemis_hip_viscous_source's sums.  Dust species beside it, drag and N-body gravity are fine: the dust runs on
// its own march or on its cell-centred kernel and the drag finish couples the fluids.  Cartesian packs (every metric
// factor 1) from 2-D up and without N-body gravity; the curvilinear systems by dimensionality (geometry.hpp CoordSelect).
static bool tile_march_takes(const PackView &P, const artemis_stage_general_args_t &g, int recon_gas) {
  if (!offsets_fit(P) || P.gas.ns != 1 || P.dust.ns > ARTEMIS_MAX_DUST_SPECIES || P.ng < 2) return false;
  if (g.strat_faces || g.cooling || (g.diffusion && !g.diffusion_sums)) return false;
  if (g.nbody_n && P.coords != ARTEMIS_CYLINDRICAL && P.coords != ARTEMIS_SPHERICAL3D) return false;
  if (effective_recon(g, recon_gas) == ARTEMIS_PPM || !gravity_type_carried(g.gravity)) return false;
  switch (P.coords) {
  case ARTEMIS_CARTESIAN:
  case ARTEMIS_CYLINDRICAL: return P.ndim >= 2;
  case ARTEMIS_SPHERICAL1D:
  case ARTEMIS_SPHERICAL2D:
  case ARTEMIS_SPHERICAL3D: return P.ndim == P.coords - ARTEMIS_SPHERICAL1D + 1;
  default: return P.coords == ARTEMIS_AXISYMMETRIC;
  }
}
// ... and the dust species beside such gas (DUST instantiations, one launch for all species): PCM / PLM, HLLE / LLF
static bool tile_march_takes_dust(const PackView &P, const artemis_stage_general_args_t &g, int recon_dust, int riemann_dust) {
  if (P.dust.ns < 1 || effective_recon(g, recon_dust) == ARTEMIS_PPM) return false;
  return riemann_dust == ARTEMIS_HLLE || riemann_dust == ARTEMIS_LLF;
}

// The older march (kernels_fused.hip, geometry in registers): one gas species alone on any non-Cartesian system,
// PCM / PLM, the pointwise tasks plane_update_curv folds in, diffusion from stored flux arrays included.
static bool fused_curv_takes(const PackView &P, const artemis_stage_general_args_t &g, int recon_gas) {
  if (P.coords == ARTEMIS_CARTESIAN || P.gas.ns != 1 || P.dust.ns != 0 || P.ng < 2 || !offsets_fit(P)) return false;
  if (effective_recon(g, recon_gas) == ARTEMIS_PPM || g.drag || g.cooling || g.nbody_n || g.defer_finish) return false;
  return gravity_type_carried(g.gravity);
}

// ---- the plan -----------------------------------------------------------------------------------------------------
StagePlan plan_stage_general(const PackView &P, const artemis_stage_general_args_t &g, int recon_gas, int /*riemann_gas*/,
                             int recon_dust, int riemann_dust) { // (every gas kernel has the three gas solvers)
  StagePlan pl;
  pl.recon_gas = effective_recon(g, recon_gas), pl.recon_dust = effective_recon(g, recon_dust);
  pl.grav_on = gravity_active(g);
  const bool cart = P.coords == ARTEMIS_CARTESIAN;
  // Off the tile march: NO_FUSED_CURV takes both curvilinear-era marches, NO_CART_MARCH every Cartesian pack, NO_CART_DUST_MARCH
  // what the march took last (Cartesian packs with dust or the shearing box, several dust species on any system)
  const bool tile_off = opt(OPT_NO_FUSED_CURV) || opt(OPT_NO_CURV_MARCH) || (cart && opt(OPT_NO_CART_MARCH)) ||
                        (opt(OPT_NO_CART_DUST_MARCH) && (P.dust.ns > 1 || (cart && (P.dust.ns != 0 || g.rf_omega != 0.0))));
  if (!opt(OPT_NO_PPM_MARCH) && ppm_march_takes(P, g, recon_gas)) pl.gas = GasKernel::PpmMarch;
  else if (!opt(OPT_NO_STAGE2D) && row_march_takes(P, g, recon_gas, recon_dust, riemann_dust)) pl.gas = GasKernel::RowMarch;
  else if (!tile_off && tile_march_takes(P, g, recon_gas)) pl.gas = GasKernel::TileMarch;
  else if (!opt(OPT_NO_FUSED_CURV) && fused_curv_takes(P, g, recon_gas)) pl.gas = GasKernel::FusedCurv;
  else pl.gas = GasKernel::Cell;

  // the dust follows the gas: inside the row march, on the tile march beside it, else on its cell-centred kernel
  if (P.dust.ns == 0) pl.dust = DustKernel::None;
  else if (pl.gas == GasKernel::RowMarch) pl.dust = DustKernel::RowMarch;
  else if (pl.gas == GasKernel::TileMarch && !opt(OPT_NO_CURV_DUST_MARCH) && tile_march_takes_dust(P, g, recon_dust, riemann_dust))
    pl.dust = DustKernel::TileMarch;
  else pl.dust = DustKernel::Cell;
  // (the dust march does the coupled update, SetAuxillaryFields and ConsToPrim of both fluids on its registers)
  pl.finish_in_march = pl.dust == DustKernel::TileMarch && g.drag && g.defer_finish != 1 && !opt(OPT_NO_DRAG_IN_MARCH) &&
                       drag_finish_in_march(P, *g.drag);
  // The row, PPM and older marches do the whole stage.  The tile march and the cell-centred kernels stop at the
  // conserved state for drag, or for a caller that finishes every zone after its fix-up (defer_finish = 1; 2 = finish
  // here, the caller re-finishes its listed zones; 0 = no fix-up follows); else a march folds its fluid's timestep in.
  const bool whole = pl.gas == GasKernel::RowMarch || pl.gas == GasKernel::PpmMarch || pl.gas == GasKernel::FusedCurv;
  pl.to_cons = !whole && (g.drag || g.defer_finish == 1);
  const bool owed = !whole && g.defer_finish != 1 && !pl.finish_in_march;
  pl.drag_finish = owed && g.drag;
  pl.dt_gas = owed && g.dt_dev && P.gas.ns && (pl.gas != GasKernel::TileMarch || pl.to_cons);
  pl.dt_dust = owed && g.dt_dev && P.dust.ns && (pl.dust != DustKernel::TileMarch || pl.to_cons);
  return pl;
}

} // namespace artemis
