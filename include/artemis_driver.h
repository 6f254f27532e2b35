/* =======================================================================================
 * artemis_driver.h -- C ABI of the host driver that stands in for Parthenon + ArtemisDriver
 * when the path runs outside Artemis (bench, tests, the `artemis` command-line tool).
 *
 * It consumes the reference's own input decks (inputs/<problem>/<name>.in, Parthenon
 * `<block>` / `key = value # comment` syntax with `&` continuation) and `block/key=value`
 * overrides exactly like `artemis -i deck block/key=value ...` (tst/scripts/utils/
 * artemis.py:122-156), builds a uniform Cartesian mesh of equal mesh blocks, runs the problem
 * generator, and advances with the stage order of ArtemisDriver<GEOM>::StepTasks
 * (artemis_driver.cpp:145-273).  All device work goes through artemis_hip.h / artemis_rt.h;
 * this layer contains no HIP code.
 *
 * Decomposition: `nranks` processes, one GPU each; the mesh-block grid is split into a
 * Cartesian grid of rank bricks.  Ghost slabs between blocks of one rank are copied on the
 * device; slabs between ranks go through an `artemis_comm_t`: the native RCCL transport below
 * (artemis_comm_rccl_create; what bench.py and a C++ host use), or callbacks supplied by the launcher
 * (the CPU tests of the host logic bind them to torch.distributed / gloo).
 * ===================================================================================== */
#ifndef ARTEMIS_DRIVER_H_
#define ARTEMIS_DRIVER_H_
#ifdef __cplusplus
extern "C" {
#endif

typedef struct artemis_sim artemis_sim_t;

typedef struct artemis_msg {
  int peer;          /* rank on the other side */
  int tag;           /* unique per (destination block, destination face) */
  double *send;      /* DEVICE buffer to send (NULL if none) */
  double *recv;      /* DEVICE buffer to receive into (NULL if none) */
  long count;        /* doubles in each direction */
} artemis_msg_t;

typedef struct artemis_comm {
  void *ctx;
  int rank, nranks;
  /* Post every send/recv of one halo exchange.  Ordered after work already enqueued on
   * `stream`; returns without waiting. */
  int (*exchange_start)(void *ctx, int nmsg, const artemis_msg_t *msgs, void *stream);
  /* Make work enqueued on `stream` after this call wait for the exchange posted last. */
  int (*exchange_finish)(void *ctx, void *stream);
  int (*allreduce_min)(void *ctx, double *value);        /* host scalar, in place */
  /* optional (may be NULL): min-all-reduce one DEVICE double in place, ordered on `stream`;
   * lets the per-cycle dt reduction ride the stream instead of costing a host round trip */
  int (*allreduce_min_dev)(void *ctx, double *dev_value, void *stream);
  int (*allreduce_sum)(void *ctx, double *values, int n); /* host array, in place */
} artemis_comm_t;

/* ---- native transport: RCCL (xGMI inside a node), artemis_amd/csrc/driver/comm_rccl.cpp -------------
 * The C++ implementation of artemis_comm_t a C++ host links directly -- no Python, no GIL: one
 * ncclGroupStart/End of ncclSend / ncclRecv per ghost exchange on the driver's comm stream (posted in
 * tag order on both sides), ncclAllReduce(min) in place on the device dt scalar, ncclAllReduce(sum) for
 * history / error norms.  Stands where Parthenon's MPI boundary communication and reductions stand
 * (artemis_driver.cpp:258, :279-297; utils/history.hpp:29-100).
 *   rank 0:      artemis_comm_rccl_unique_id(buf, sizeof buf)   -> ship the bytes to every rank (any
 *                out-of-band channel: the launcher's store, MPI_Bcast, a file)
 *   every rank:  artemis_rt_set_device(local_rank); comm = artemis_comm_rccl_create(id, rank, nranks);
 *                sim = artemis_sim_create(deck, n, overrides, comm); ...; artemis_comm_rccl_destroy(comm)
 * create() is collective (ncclCommInitRank).  Returns NULL / non-zero on error
 * (artemis_comm_rccl_last_error()). */
int artemis_comm_rccl_unique_id_bytes(void);
int artemis_comm_rccl_unique_id(char *out, int capacity);
artemis_comm_t *artemis_comm_rccl_create(const char *unique_id, int rank, int nranks);
void artemis_comm_rccl_destroy(artemis_comm_t *comm);
int artemis_comm_rccl_count(const artemis_comm_t *comm);  /* ncclCommCount: ranks RCCL itself reports */
int artemis_comm_rccl_barrier(artemis_comm_t *comm);      /* all-reduce + stream sync */
const char *artemis_comm_rccl_last_error(void);

/* deck_text: contents of an input deck; overrides: `block/key=value` strings (may be NULL).
 * comm: NULL for a single process.  Returns NULL on error (artemis_sim_last_error()). */
artemis_sim_t *artemis_sim_create(const char *deck_text, int noverrides, const char *const *overrides,
                                  const artemis_comm_t *comm);
void artemis_sim_destroy(artemis_sim_t *sim);
const char *artemis_sim_last_error(void);

/* EvolutionDriver::Execute (parthenon, upstream): advance until tlim / nlim of the deck, or by
 * at most `max_cycles` further cycles if max_cycles >= 0.  Returns cycles taken, < 0 on error. */
long artemis_sim_evolve(artemis_sim_t *sim, long max_cycles);

double artemis_sim_time(const artemis_sim_t *sim);
double artemis_sim_dt(const artemis_sim_t *sim);
double artemis_sim_tlim(const artemis_sim_t *sim);
long artemis_sim_ncycle(const artemis_sim_t *sim);
/* interior cells owned by this rank / by all ranks */
long artemis_sim_local_zones(const artemis_sim_t *sim);
long artemis_sim_total_zones(const artemis_sim_t *sim);
/* Statically refined meshes (<parthenon/mesh> refinement = static + <parthenon/static_refinementN>): mesh blocks
 * of this rank carry their level; every block has the same number of zones.  The refined mesh runs the
 * per-task chain (flux correction needs the stage's face fluxes). */
int artemis_sim_block_level(const artemis_sim_t *sim, int block);
long artemis_sim_nblocks_global(const artemis_sim_t *sim);
int artemis_sim_uses_fused_path(const artemis_sim_t *sim);
/* 1 when the fused path runs the hand-tuned gas kernel (artemis_hip_stage_fused), 0 when it runs
 * the general cell-centred stage (artemis_hip_stage_general) or the per-task chain */
int artemis_sim_uses_tuned_kernel(const artemis_sim_t *sim);
/* name of the kernel family the stages run on: "stage_fused_kernel" (tuned 2.5-D), "stage2d_kernel" (2-D row march),
 * "stage_cell_kernel" (cell-centred general stage) or "per-task chain"; static storage */
const char *artemis_sim_stage_kernel(const artemis_sim_t *sim);
/* <parthenon/mesh> refinement = adaptive: how many times the block tree has changed so far (the initial
 * refinement passes included).  The block layout (artemis_sim_dims, block bounds / levels) changes with it. */
long artemis_sim_remeshes(const artemis_sim_t *sim);
/* Wall-clock cost of the remeshes DURING the run (the initial refinement passes are set-up): returns their number and
 * fills out[4] = {total seconds, of which building the new mesh's state, handing the data over, and -- over all
 * cycles, remeshed or not -- evaluating the refinement criterion and the tree}. */
long artemis_sim_remesh_seconds(const artemis_sim_t *sim, double *out);
/* The most recent remesh: leaves4 = {leaves before, leaves after, leaves created (not in the old mesh), leaves destroyed
 * (not in the new one)}, seconds3 = {total, building the new state, handing the data over} (zeros before the first
 * remesh of the run; either pointer may be NULL). */
void artemis_sim_last_remesh(const artemis_sim_t *sim, long *leaves4, double *seconds3);
/* Measurement hook (bench.py's remesh leg): split the leaf with global (Z-order) index gid as if the refinement
 * criterion had tagged it -- the ordinary remesh machinery runs (2:1 balance, new state, hand-over of the data, block
 * migration between ranks) and is timed like any other remesh.  Collective over the ranks (same gid everywhere).
 * Returns 1 if the mesh changed, 0 if not (the leaf is at the finest level), < 0 on error. */
int artemis_sim_force_refine(artemis_sim_t *sim, long gid);
/* ... many leaves at once, the way a criterion tags them: the listed leaves (global Z-order indices) get the tag +1
 * NEXT TO the tags the deck's own criterion gives every other leaf, derefinement counters included -- so leaves the
 * criterion does not want refined merge again `derefine_count` cycles later, by the ordinary path.  One remesh check is
 * run at once (collective; the same list on every rank).  Returns 1 if the mesh changed, 0 if not, < 0 on error. */
int artemis_sim_inject_refine_tags(artemis_sim_t *sim, const long *gids, int n);
/* Refined meshes: the largest rank's cost over the mean cost of the Z-order rank split (1 = perfectly even).  The cost
 * of a block is 1 by default (Parthenon's unit cost per block); the driver's own deck block
 *   <artemis_amd/loadbalance>  level_cost = c0, c1, ...   flux_face_cost = c
 * weighs blocks by refinement level and by the coarse-fine face operations they take part in; the split then evens
 * the cumulative cost of contiguous Z-order runs instead of their lengths.  Results do not depend on the split. */
double artemis_sim_load_balance(const artemis_sim_t *sim);
/* which: "fused" | "unfused"; selects the kernel path (fused only where supported). */
int artemis_sim_set_path(artemis_sim_t *sim, const char *which);
/* Halo exchange on a second stream concurrently with interior compute (fused path, remote
 * neighbours only).  0 = off; 1 = boundary-shell launch, then bulk launch; 2 = one launch whose
 * shell workgroups run first and signal a device counter the comm stream waits on. */
int artemis_sim_set_overlap(artemis_sim_t *sim, int overlap);
/* current mode (a timed-out mode-2 wait resets it to 0 and makes artemis_sim_evolve fail) */
int artemis_sim_overlap(const artemis_sim_t *sim);
/* Drop-in accounting for the tuned fused kernel (bench.py's `dropin` object): the last stage also writes
 * the conserved state (cons_out) and every stage ends with the whole-block PrimToCons a Parthenon host
 * runs as FillDerived (artemis.cpp:123, artemis_driver.cpp:261) -- what the fused path costs when the host
 * keeps `cons` as its Independent / Restart state.  on = 2: every stage stores cons of the zones it updates and only
 * the ghost zones go through PrimToCons after the exchange (artemis_hip_prim_to_cons_ghosts): `cons` is just as
 * current after every stage, at 5 % of the conversion work.  Same results; returns non-zero off the tuned path. */
int artemis_sim_set_dropin(artemis_sim_t *sim, int on);
/* <gravity/nbody> with <nbody> integrator = none: the accumulated particle_force rows [npart][7] = {mass accreted,
 * gravity force x3, accretion force x3} (nbody_gravity.hpp:129-136), summed over ranks like NBody::Advance does
 * (nbody_advance.cpp:123-131); reset != 0 zeroes them afterwards.  Returns the number of particles. */
int artemis_sim_nbody_force(artemis_sim_t *sim, double *out, int reset);
/* number of gas / dust species (sizes the buffers of artemis_sim_get_field and artemis_sim_history) */
void artemis_sim_species(const artemis_sim_t *sim, int *ns_gas, int *ns_dust);

/* Block layout of this rank. dims = {nblocks_local, ni, nj, nk, is, ie, js, je, ks, ke, ng}. */
void artemis_sim_dims(const artemis_sim_t *sim, int *dims);
/* Copy one field of one local block to the host, [nvar][nk][nj][ni] doubles (ghosts included).
 * field: "gas.prim" (6*ns), "gas.cons" (6*ns), "dust.prim" (4*ns), "dust.cons" (4*ns).
 * Conserved fields and pressure are materialised (PrimToCons) first.  Returns nvar or < 0. */
int artemis_sim_get_field(artemis_sim_t *sim, const char *field, int block, double *host_out);
/* interior bounds of a local block: out = {x1min,x1max,x2min,x2max,x3min,x3max} */
void artemis_sim_block_bounds(const artemis_sim_t *sim, int block, double *out);

/* History integrals (utils/history.hpp:29-100, gas.cpp:648-676, dust.cpp:332-352), reduced
 * over ranks: out = [gas mass, mom1..3, energy, internal energy] (species 0) then
 * [mass, mom1..3] per dust species.  Returns the number of values. */
int artemis_sim_history(artemis_sim_t *sim, double *out);
/* Post-loop error norms of the problem generator (linear_wave.hpp:267-377: out[0] rms,
 * out[1..5]; advection.hpp:224-405: out[0..2] rms gas/dust1/dust2, out[3..15]).  Returns the
 * number of values, 0 if the pgen defines none. */
int artemis_sim_errors(artemis_sim_t *sim, double *out);

/* ---- checkpoint and restart ----------------------------------------------------------------------------------------
 * A checkpoint is a directory with one plain binary part file per writing rank (part-00000.bin, ...; layout in
 * artemis_amd/csrc/driver/checkpoint.cpp): the deck and overrides of the run, its clock (time, dt, ncycle), the block tree
 * and the remesh history of an adaptive mesh, the n-body force sums, and per block the whole primitive arrays, ghost zones
 * included, bytes as they are.  Everything else is rebuilt from the deck.  A restored run continues bit for bit like the
 * run that was saved, on any number of ranks (n-body sums regroup across rank counts: equal to round-off there).
 * Callers checkpoint between artemis_sim_evolve calls, or let the deck's `rst` output blocks do it ("deck-driven
 * outputs" below).
 *
 * save: collective over the ranks of the simulation, which must see one file system.  Writes <path>.tmp and renames it
 * once every rank has succeeded (an existing checkpoint at <path> is replaced).  Returns 0, non-zero on error. */
int artemis_sim_save(artemis_sim_t *sim, const char *path);
/* restore: collective over `comm` (NULL: one process); any rank count may read any checkpoint.  `overrides` are applied
 * after the stored ones (nlim, tlim, cfl, solver, ...); one that changes block shape, nghost, species counts, coordinates
 * or dimensionality is refused by name.  Runtime settings (artemis_sim_set_path / _set_overlap / _set_dropin) are not
 * state: re-apply them.  A wrong magic or version, a truncated or missing part, a checksum mismatch or a directory entry
 * that points outside its file return NULL (artemis_sim_last_error()). */
artemis_sim_t *artemis_sim_restore(const char *path, int noverrides, const char *const *overrides,
                                   const artemis_comm_t *comm);
/* The header fields of a checkpoint as one JSON object; touches no device and needs no communicator.  Returns the length
 * of the text (written with its NUL only if capacity exceeds it: call with NULL / 0 for the size), < 0 on error. */
int artemis_sim_checkpoint_describe(const char *path, char *json_out, long capacity);
/* Wall-clock seconds of the calling thread's last save or restore: out4 = {total (a restore: building the state from the
 * deck included), device copies, checksums, file writes or reads}. */
void artemis_sim_checkpoint_seconds(double *out4);

/* ---- deck-driven outputs ---------------------------------------------------------------------------------------------
 * The <parthenon/outputN> blocks of the deck (file_type, dt) are acted on only after artemis_sim_enable_outputs; without
 * it artemis_sim_evolve writes nothing.  Files go to `dir` (created if missing; the ranks must see one file system):
 *   file_type = hst   <dir>/<problem_id>.outN.hst: "#  History data", a label line "# [1]=time [2]=dt [3]=cycle
 *                     [4]=nbtotal [5]=gas_mass_0 ..." (gas_mass_n, gas_momentum_x{1,2,3}_n, gas_energy_n,
 *                     gas_internal_energy_n, dust_mass_n, dust_momentum_x{1,2,3}_n; the species is the inner index), then
 *                     one row per output, floats as %.16e.  time, dt, cycle are the clock after the cycle (dt: the next
 *                     step's).  An existing file is appended to behind a fresh header section.  Rank 0 writes.
 *   file_type = rst   artemis_sim_save into <dir>/<problem_id>.outN.<5-digit counter>.rst, and into ...outN.final.rst
 *                     when the run ends.
 *   file_type = fld   artemis_sim_write_fields ("field output" below) of the block's `variables` (comma list) into
 *                     <dir>/<problem_id>.outN.<5-digit counter>.fld, and into ...outN.final.fld when the run ends; scheduled
 *                     and numbered like `rst`.  single_precision_output = true (parthenon's key) stores float.  A block
 *                     without `variables`, with a name outside the list or of a fluid the run lacks, or with ghost_zones
 *                     = true is listed as skipped ("no variables", "unknown variable NAME", "ghost_zones is not built") and
 *                     writes nothing.  A shipped `hdf5` block becomes one with the override
 *                     parthenon/outputN/file_type=fld.  level = L (negative allowed): artemis_sim_write_fields_level, every
 *                     block on the zone size of refinement level L.  The worst shifts the deck can ever produce -- its
 *                     finest possible level (numlevel - 1, the deepest static region) and the root grid -- are checked
 *                     here against the block extents: a block that could need an impossible one is listed as skipped
 *                     ("level L: a block on level X would need shift s, ...") and never fails in the middle of a run.
 *   anything else     not acted on (never an error); artemis_sim_outputs_describe lists it as skipped.
 * Schedule (parthenon's Outputs, upstream): a block is due after the first cycle that ends with time >= next_time, and
 * next_time then becomes the smallest integer multiple of the block's dt above time; a fresh run writes every block at
 * cycle 0 (once the first dt exists); every block is written once more when the run ends at tlim or nlim -- not when a
 * max_cycles budget runs out, and not twice for one cycle.  A restored run derives next_time from its clock.  Output times
 * never clip dt: the run takes the same steps with and without outputs.  Returns 0, non-zero on error. */
int artemis_sim_enable_outputs(artemis_sim_t *sim, const char *dir);
/* The history integrals of every species, summed on the device from the primitives (artemis_hip_history_sums) and reduced
 * over the ranks: out = [mass, mom1..3, energy, internal energy] per gas species, then [mass, mom1..3] per dust species
 * (the layout of artemis_sim_history for one gas species).  Returns the number of values, < 0 on error. */
int artemis_sim_history_device(artemis_sim_t *sim, double *out);
/* The output blocks of the deck and their state as one JSON object {"enabled", "dir", "problem_id", "blocks": [{"block",
 * "index", "file_type", "dt", "status", "next_time", "written", "last_cycle", "path"}]}; a `fld` block also has
 * "variables" (the names of its list), "single_precision" and, if the block has one, "level".  Returns the length of the text
 * (written with its NUL only if capacity exceeds it: call with NULL / 0 for the size), < 0 on error. */
int artemis_sim_outputs_describe(const artemis_sim_t *sim, char *json_out, long capacity);

/* ---- field output --------------------------------------------------------------------------------------------------
 * Variables are named as in a deck's `variables` line: gas.prim.density | .velocity | .pressure | .sie, gas.cons.density |
 * .momentum | .total_energy | .internal_energy, dust.prim.density | .velocity, dust.cons.density | .momentum.  A scalar has
 * one component per species, a vector three (index 3 n + d).  Every value is what PrimToCons would store for the zone
 * (floors applied; the pressure is (gamma-1) rho sie, not the stored slot, which the one-kernel stages never write), formed
 * from the primitives on the device (artemis_hip_pack_fields): no conserved array is materialised and the run's bits do
 * not change.
 * Derived variables, outputs only: gas.derived.divergence (one component per species), gas.derived.vorticity (three), and
 * dust.derived.divergence | .vorticity -- the velocity divergence and the curl in the mesh's orthogonal coordinates, formed
 * on the device from the stored velocities of a zone and its six face neighbours, ghost zones included (artemis_hip.h,
 * "derived variables", has the definition; in a rotating frame it is the frame's vorticity).  A request that names one
 * first fills the ghost zones a stage loop may have left for later; that writes ghost zones only and the run's bits do not
 * change.  They pass through gather, write, `fld` blocks and the level / reduced forms below like any other component;
 * artemis_sim_scatter_fields refuses them (".. is an output, not part of a state").
 *
 * gather: host_out receives [local block][component][nk][nj][ni] over the INTERIOR zones of this rank's blocks, the
 * components in the order of `names`, as double or (single != 0) float; returns the number of components.  host_out =
 * NULL: returns the size of that buffer in bytes and gathers nothing.  The device side is a staging buffer of a whole
 * number of blocks and at most 256 MiB (switch FIELDS_STAGE_MB, artemis_hip.h), allocated by the first call.  A name
 * outside the list, or of a fluid the run does not have, is an error: < 0 (artemis_sim_last_error()). */
long artemis_sim_gather_fields(artemis_sim_t *sim, int nvar, const char *const *names, int single, void *host_out);
/* write: one dump of those variables as a directory `path` (collective; the ranks must see one file system):
 *   meta.json     {"format": "artemis_fld", "version": 1, "time", "dt", "cycle", "coordinates", "ndim", "nghost": 0,
 *                 "dtype": "<f8" | "<f4", "gamma", "ns_gas", "ns_dust", "nranks", "nx": [nx1, nx2, nx3] of a block,
 *                 "variables": [{"name", "ncomp", "components": [names]}], "blocks": [{"gid", "level", "bounds": [x1min,
 *                 x1max, x2min, x2max, x3min, x3max], "nx", "rank", "index"}] in gid order}; rank 0 writes it, last
 *   rank<r>.bin   the raw little-endian gather of rank r: block `index` of rank `rank` starts at index * ncomp * nx1 *
 *                 nx2 * nx3 elements
 * Everything is written into <path>.tmp, which is renamed once every rank has succeeded (an existing dump at `path` is
 * replaced): a directory that is there is complete.  artemis_amd/fields.py reads it.  Returns 0, non-zero on error. */
int artemis_sim_write_fields(artemis_sim_t *sim, const char *path, int nvar, const char *const *names, int single);
/* ---- field output at a level: the same variables with every block resampled, on the device, to the zone size of
 * refinement level `level` (0 = the root grid; negative = coarser than it) before it leaves the device.  A block on level l
 * has shift s = l - level: s >= 1 restricts it s times with the volume-weighted mean of the reference's RestrictAverage<GEOM>
 * (summed volumes: exactly conservative), s <= -1 replicates its zones 2^|s| times (exact copies, no slopes: a dump invents
 * no gradients), s = 0 leaves it; only directions with more than one zone are halved or doubled (artemis_hip.h,
 * artemis_hip_pack_fields_level, has the definition).  Each REQUESTED COMPONENT is averaged as formed -- gas.prim.velocity
 * as a velocity, as the reference's restriction treats primitives in its ghost exchange; gas.cons.* gives the conservative
 * answer.  So a refined mesh reads as one array, and level = -1 on a one-level mesh is a dump an eighth the size (3-D).
 * |s| <= 3, and s >= 1 needs every active extent of the block divisible by 2^s: a request that breaks either is an error that
 * names the block, its level and the rule, before anything is written.  Primitives are read, nothing in the run moves.
 *
 * gather_level: the blocks follow each other in host_out in local block order, each as [component][nk'][nj'][ni'];
 * block_offsets (nblocks_local + 1 longs, or NULL) receives the element offset of every block and the total.  Returns the
 * number of components; with host_out = NULL only the offsets are filled and the bytes needed are returned.  The staging
 * buffer (FIELDS_STAGE_MB) takes block ranges by bytes.  < 0 on error.
 * write_level: artemis_sim_write_fields with "version": 2 in meta.json, which adds "level": L, and whose block entries carry
 * the "nx" each block was written with and "offset", the element offset of its first value in its rank's part. */
long artemis_sim_gather_fields_level(artemis_sim_t *sim, int nvar, const char *const *names, int single, int level, void *host_out,
                                     long *block_offsets);
int artemis_sim_write_fields_level(artemis_sim_t *sim, const char *path, int nvar, const char *const *names, int single, int level);
/* ---- reduced field output: the same variables INTEGRATED over chosen directions, on the device, before they leave it.
 * `axes` is a non-empty mask of ACTIVE directions (more than one zone): 1 = x1, 2 = x2, 4 = x3.  Per zone and component the
 * leaf is N = V q (q as gather forms it, V = Coords::Volume) and W = V; both are summed one direction at a time -- x1 as a
 * butterfly in chunks of 64 zones whose sums are added in increasing order, then x2, then x3 sequentially in increasing
 * index -- an order that depends on nothing but the block (artemis_hip.h, artemis_hip_reduce_fields, has the definition).
 * Blocks are not combined and nothing is divided: a mean is N / W after the blocks that meet an output cell have been added
 * (artemis_amd/fields.py, FieldDump.reduced).  Primitives are read; cons_valid, the clock, the mesh and the run's bits stay.
 *
 * gather_reduced: host_out is [local block][ncomp + 1][nk'][nj'][ni'] with the reduced extents 1 and the volume W as the
 * last component.  Returns the number of components WITHOUT the volume; with host_out = NULL the bytes needed.  The
 * staging and work buffers (FIELDS_STAGE_MB) take block ranges by bytes.  < 0 on error (axes = 0, an inactive direction).
 * write_reduced: artemis_sim_write_fields with "version": 3 in meta.json, which adds "reduce": ["x2", "x3"], lists the
 * variable "volume" last, and whose block entries carry their reduced "nx" and "offset".  A deck's `reduce = x2,x3` in a
 * `fld` block writes these; a block whose list names an inactive or unknown direction, or that also sets `level`, is listed
 * as skipped with the reason ("reduce: ...") by artemis_sim_outputs_describe and writes nothing. */
long artemis_sim_gather_fields_reduced(artemis_sim_t *sim, int nvar, const char *const *names, int single, int axes, void *host_out);
int artemis_sim_write_fields_reduced(artemis_sim_t *sim, const char *path, int nvar, const char *const *names, int single, int axes);
/* ---- reduced field output on a chosen level: the same integrals with every block brought to the zone size of refinement
 * level `level` (0 the root grid, negative coarser) along the directions it KEEPS (active and outside `axes`), so the blocks
 * of a refined mesh add cell by cell.  A block on level l has shift s = l - level, |s| <= 3.  It is reduced at its own
 * resolution exactly as above; s >= 1 then adds pairs, x = x[0::2] + x[1::2], s times along each kept direction (the kept
 * extents must be divisible by 2^s); s <= -1 gives each of the 2^(|s| m) output cells under a coarse zone (m kept
 * directions) an EQUAL share, N and W times 2^(-|s| m), so every covered cell has the coarse zone's own mean N / W bit for
 * bit and the parts add back to the whole.  Nothing is split along a reduced direction.  The share is even in index space:
 * on a curvilinear mesh the integral of a single output cell under a coarser block is its even share, not its geometric
 * one; means, and sums over whole coarse zones, are exact (artemis_hip.h, artemis_hip_reduce_fields_level, has the
 * definition).  Every shift is checked before anything is written.
 *
 * gather_reduced_level: host_out holds the local blocks one after the other, each [ncomp + 1][nk'][nj'][ni'], the volume
 * last; block_offsets (nblocks_local + 1 longs, or NULL) receives the element offset of every block and the total.
 * Returns the number of components WITHOUT the volume; with host_out = NULL the bytes needed.  < 0 on error.
 * write_reduced_level: "version": 4 in meta.json -- version 3 plus "reduce_level", the block entries carrying the "nx"
 * they were brought to and their "offset".  A deck's `reduce_level = L` beside `reduce` in a `fld` block writes these; it is
 * checked at parse time against the worst shifts the deck can produce, and a block it cannot serve -- or one that sets
 * reduce_level without reduce, or with `level` -- is listed as skipped with the reason ("reduce_level ..."). */
long artemis_sim_gather_fields_reduced_level(artemis_sim_t *sim, int nvar, const char *const *names, int single, int axes, int level,
                                             void *host_out, long *block_offsets);
int artemis_sim_write_fields_reduced_level(artemis_sim_t *sim, const char *path, int nvar, const char *const *names, int single, int axes,
                                           int level);
/* scatter: the inverse of gather -- the run takes its state from the caller's arrays, which is this driver's form of
 * "write your own problem generator".  host_in is this rank's blocks in local order, laid out as gather returns them for
 * the same names ([local block][component][nk][nj][ni] over the INTERIOR zones, double or float).  For each fluid the names
 * give exactly one complete form, or nothing (that fluid keeps its state); each name once:
 *   gas    gas.prim.density + .velocity + one of .sie / .pressure, or gas.cons.density + .momentum + .total_energy
 *          (+ .internal_energy; without it that input is 0 and gas/de_switch decides as in SetAuxillaryFields)
 *   dust   dust.prim.density + .velocity, or dust.cons.density + .momentum
 * (artemis_hip_unpack_fields, artemis_hip.h, has the expressions).  The arrays go through the staging buffer of gather, a
 * whole number of blocks per copy, into the interior primitives of the current buffer; then the state is completed the
 * way a problem generator's is: PrimToCons, ConsToPrim, the ghost fill (neighbours, coarse-fine boundaries, physical
 * conditions), PrimToCons.  `time` becomes the clock (NaN keeps it) and dt a fresh estimate as at the start of a run: the
 * minimum over the ranks, clipped to tlim, without the "at most doubles" rule of a running clock.  ncycle, the mesh (no
 * remesh happens here: the next cycle's tagging adapts it), the n-body rows, the output schedule and the initial-condition
 * states of `ic` boundaries stay as they are; ghost zones no condition or neighbour writes (corners, on runs without
 * viscosity) keep their old values, which nothing reads.
 * host_in = NULL: validates the arguments and returns the size of that buffer in bytes, the number gather returns for them.
 * Collective.  Returns that size, or < 0 (artemis_sim_last_error()): a dead handle, an unknown name or one of a fluid the
 * run lacks, a mixed, incomplete or repeated form, or blocks narrower than nghost -- the state of such a run is all three
 * primitive buffers (checkpoints store them), which one set of arrays does not give. */
long artemis_sim_scatter_fields(artemis_sim_t *sim, int nvar, const char *const *names, int single, const void *host_in,
                                double time);

/* ---- sampling at points: the same variables AT ARBITRARY POINTS of the mesh's own coordinates (x1, x2, x3) -- a slice, a zoom
 * at the finest level, a ray, a pixel grid -- the one field output whose cost follows the number of points and not the mesh.
 * A point is found in this rank's blocks (half-open leaves, the mesh's xmax closed; coordinates along directions with one
 * zone are ignored; no periodic wrapping) and takes the value gather returns for the zone that holds it, bit for bit:
 * nothing is interpolated.  artemis_hip_sample.h has the definition; the search and the values run on the device.
 *
 * plan_create: points_host is [npoints][3] doubles; the plan keeps the points, their locations and the points' order sorted
 * by location on the device, and belongs to the handle.  Returns its id (>= 0), < 0 on error.  npoints = 0 is a plan.
 * plan_locations: loc_host receives [npoints][4] ints {local block, k, j, i} (interior-relative zone indices), all -1 for a
 * point that is not found -- outside the mesh, not finite, or in a block of another rank.
 * plan_values: host_out receives [component][npoints] in the caller's point order, the components in the order of `names`
 * as gather orders them, double or (single != 0) float, NaN for a point that is not found; returns the number of components.
 * host_out = NULL: returns the bytes of that buffer.  The values go through the staging buffer of gather (FIELDS_STAGE_MB).
 * A plan survives a remesh: it records the block list it was located on, and the next plan_locations or plan_values after
 * the blocks have been rebuilt locates again by itself.  scatter leaves plans alone (the mesh stays).  Plans are not part
 * of a checkpoint.  The calls are not collective: every rank answers for its own blocks, and since the leaves tile the mesh
 * an in-domain point is found on exactly one rank.  Primitives are read; the run's bits do not change.
 * plan_destroy frees the plan; every call on an id that does not exist is an error (artemis_sim_last_error()). */
long artemis_sim_sample_plan_create(artemis_sim_t *sim, long npoints, const double *points_host);
int artemis_sim_sample_plan_locations(artemis_sim_t *sim, long id, int *loc_host);
long artemis_sim_sample_plan_values(artemis_sim_t *sim, long id, int nvar, const char *const *names, int single, void *host_out);
int artemis_sim_sample_plan_destroy(artemis_sim_t *sim, long id);

/* ---- a time series of samples, recorded on the device inside the time loop.  A recorder has a plan of this handle, a
 * selection of variables, `every` >= 1, a row `capacity` >= 1 and a precision.  `seen` counts the cycles artemis_sim_evolve
 * has completed since the recorder was made; after a completed cycle with seen % every == 0 one row is appended:
 *   cycle, time, dt   what artemis_sim_ncycle / _time / _dt would return had evolve returned after exactly that cycle
 *   values            [ncomp][npoints]: what artemis_sim_sample_plan_values would return at that moment, bit for bit
 * (on an adaptive mesh: after that cycle's remesh check, the plan located again when the blocks changed).  Only
 * artemis_sim_evolve advances `seen`.  The record steps run inside the time loop and inside its captured graphs; rows
 * collect on the device in buffers of `capacity` rows, which the loop empties into host storage at a batch boundary when they
 * are full -- the only synchronisation a recorder adds -- so no row is lost.  The run is not disturbed: state, time, dt
 * and cycle count are the same bits with and without recorders (a derived variable fills ghost zones first, as a gather does).
 * A recorder is rank-local like its plan, is not part of a checkpoint, and lives until _destroy or the end of the handle.
 *   _create   an id >= 0; -1: no such plan, an unknown variable, every < 1, capacity < 1, an allocation that failed
 *   _rows     the rows recorded and not yet cleared (it drains the device buffers first); -1 on failure
 *   _read     copies them, oldest first, into the buffers that are not NULL -- cycle_out [rows] (long), time_out and dt_out
 *             [rows], values_out [rows][ncomp][npoints] (double, or float for a single recorder) -- and, with clear != 0,
 *             forgets them; returns ncomp.  With every buffer NULL nothing is copied or cleared: ask _rows for the sizes.
 * artemis_sim_sample_plan_destroy refuses a plan that a live recorder uses. */
long artemis_sim_record_create(artemis_sim_t *sim, long plan_id, int nvar, const char *const *names, long every, long capacity, int single);
long artemis_sim_record_rows(artemis_sim_t *sim, long id);
long artemis_sim_record_read(artemis_sim_t *sim, long id, long *cycle_out, double *time_out, double *dt_out, void *values_out, int clear);
int artemis_sim_record_destroy(artemis_sim_t *sim, long id);

/* ---- a time series of the history integrals and of the n-body force sums, through the same tick.  An integral recorder is a
 * recorder of a second kind: no plan, but nwin windows (0 .. 7) and a flag nbody; every, capacity, seen, due rows, drains and
 * the undisturbed run are those of a sample recorder, and _rows and _destroy above serve both kinds (one id space).  A row:
 *   cycle, time, dt            as above;
 *   integrals[1 + nwin][nq]    nq = 6 ns_gas + 4 ns_dust in the layout of artemis_sim_history_device.  Set 0 is this rank's
 *                              mesh: on one rank the bits artemis_sim_history_device would return had evolve returned after
 *                              exactly that cycle (artemis_hip_history_sums on this rank's pack).  Set 1 + w is window w by
 *                              the same pass and the same reduction tree (include/artemis_hip_record.h): a window that holds
 *                              every zone has the bits of set 0, one that holds none is +0.0;
 *   nbody[npart][7]            with nbody != 0: the host's force rows plus this rank's device accumulators -- on one rank the
 *                              bits artemis_sim_nbody_force would return if called for the first time after exactly that
 *                              cycle.  Recording flushes nothing, so later artemis_sim_nbody_force results keep their bits.
 * windows: [nwin][3][2] doubles, the box [lo_d, hi_d) of each window in the mesh's own coordinates (an annular sector on a
 * cylindrical mesh).  A zone belongs to a window when along every direction with more than one zone the midpoint of its two
 * face positions, as the block's geometry holds them, satisfies lo_d <= c_d < hi_d; other directions are ignored, nothing
 * wraps.  The host turns the windows into index ranges per block once per mesh epoch (after a remesh they are rebuilt, as a
 * plan locates again); the device compares indices only.  Rows are rank-local; not part of a checkpoint; only evolve records.
 *   _create        the recorder's id (>= 0), or -1: every < 1, capacity < 1, nwin outside 0 .. 7, a window with lo >= hi along
 *                  a direction with more than one zone, nbody != 0 on a deck without particles
 *   _read          all pointers NULL: nq.  Else the rows so far, oldest first -- integrals_out [rows][1 + nwin][nq], nbody_out
 *                  [rows][npart][7] (ignored without n-body rows) -- and, with clear != 0, forgets them.  Returns nq, -1 on failure
 *   _window_zones  zones_out [nblocks][nwin][6] ints {i0, i1, j0, j1, k0, k1}: the zones of every window on every local block,
 *                  half-open and relative to the block's first interior zone, empty as i0 == i1 (NULL: nothing is copied).
 *                  Returns the number of local blocks, -1 on failure */
long artemis_sim_record_integrals_create(artemis_sim_t *sim, long every, long capacity, int nwin, const double *windows, int nbody);
long artemis_sim_record_integrals_read(artemis_sim_t *sim, long id, long *cycle_out, double *time_out, double *dt_out, double *integrals_out,
                                       double *nbody_out, int clear);
long artemis_sim_record_integrals_window_zones(artemis_sim_t *sim, long id, int *zones_out);

/* Seconds spent inside the timed region of the last artemis_sim_evolve (device-synchronised
 * at both ends), and the average duration in ms of the dominant kernel's launches measured
 * with HIP events on the compute stream. */
void artemis_sim_set_kernel_timing(artemis_sim_t *sim, int on);
double artemis_sim_last_wall_seconds(const artemis_sim_t *sim);
double artemis_sim_kernel_ms(const artemis_sim_t *sim, long *nlaunch);

#ifdef __cplusplus
}
#endif
#endif /* ARTEMIS_DRIVER_H_ */
