/* Point sampling of a pack's fields: part of the C ABI of libartemis_hip.so, in a header of its own beside artemis_hip.h
 * (which it includes).  The value of the requested variables AT A POINT: the point is found in the pack's blocks and the
 * components are formed from the primitives of the zone that holds it, on the device.  It is the one field output whose cost
 * follows the number of points and not the size of the mesh: a slice, a zoom at the finest level, a ray, a pixel grid.
 *
 * ---- definition (fixed in bits; tests/fields_sample_ref.py is its numpy form) -------------------------------------------
 * Inputs: npoints points x[p][0..2], double, in the mesh's own coordinates (x1, x2, x3); the table bounds[b] = {lo_1, hi_1,
 * lo_2, hi_2, lo_3, hi_3} of the pack's blocks; closed_hi[d], the upper edge of the mesh.  A direction is ACTIVE if blocks
 * have more than one zone along it; coordinates along inactive directions are ignored (garbage, NaN: anything).
 *
 * 1. Block.  Block b contains the point if for every active d   lo_d <= x_d   and   x_d < hi_d, or x_d == hi_d where hi_d ==
 *    closed_hi[d].  The lowest such b is the point's block.  Leaves of a block tree carry the same double on a shared face, so
 *    they tile the mesh half-open and every in-domain point has exactly one block.  A coordinate that is not finite along an
 *    active direction is not found; a point no block contains is not found.  No periodic wrapping: the caller wraps.
 * 2. Zone, per active direction.  n: zones of a block along it, g: the pack's nghost, {xf0, dx}: the block's geom entries
 *    (dx = (hi - lo) / n, xf0 = lo - g dx as the driver and MeshBlockPack form them), Xf(t) = xf0 + t * dx for t = g .. g + n
 *    (one multiplication, one addition, not contracted).  The zone is
 *        clip(#{t : Xf(t) <= x} - 1, 0, n - 1)          numpy: clip(searchsorted(Xf, x, side="right") - 1, 0, n - 1)
 *    -- the clip covers Xf(g) differing from lo in its last bit, and the closed mesh edge.  An inactive direction has zone 0.
 * 3. Value.  For every requested component the double artemis_hip_pack_fields stores for that zone of that block, formed by
 *    the same functions (csrc/fields_device.hpp): the same bits as a gather; floats by the same narrowing.  Every code of enum
 *    artemis_field_var is taken, the derived ones (from the zone and its six face neighbours, ghost zones included) too.
 *    Nothing is interpolated: a sample invents no gradients, as a dump invents none.
 * Output: out[c * npoints + p], component c of point p in the caller's order, the components in the order of `sel` exactly
 * as artemis_hip_pack_fields orders them; loc[p] = {block, k, j, i}, interior-relative zone indices.  A point that is not
 * found has loc = {-1, -1, -1, -1} and NaN in every component. */
#ifndef ARTEMIS_HIP_SAMPLE_H_
#define ARTEMIS_HIP_SAMPLE_H_

#include "artemis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The search table of a set of blocks (host side, no device needed): a lattice of cells of the smallest block extent, each
 * listing the blocks that can hold one of its points, lowest index first -- on a tiling block tree one block per cell, so a
 * point costs one cell index and one containment test however many blocks there are.  active: bit d set if blocks have more
 * than one zone along direction d.  _bytes: the size of the table, 0 for arguments _build refuses.  _build fills table_host
 * (8-byte aligned, `bytes` of it); the table holds offsets, not pointers: copy it to the device as it is.
 * ARTEMIS_HIP_EINVAL: no blocks, a mask outside 0 .. 7, bounds that are not finite or not ordered, a buffer too small. */
size_t artemis_hip_locate_table_bytes(int nblocks, const double *bounds, const double *closed_hi, int active);
int artemis_hip_locate_table_build(int nblocks, const double *bounds, const double *closed_hi, int active, void *table_host,
                                   size_t bytes);

/* Steps 1 and 2 for npoints points: points_dev [npoints][3] doubles, loc_dev [npoints][4] ints, table_dev the device copy of
 * a table built for this pack's blocks (its block count must be the pack's), closed_hi: 3 doubles on the host.  One point
 * per lane, grid-stride; double compares only, no LDS, no atomics.  The pack's geom table is read, no primitive.
 * npoints == 0 succeeds and touches nothing; npoints < 0 and null pointers are ARTEMIS_HIP_EINVAL. */
int artemis_hip_locate_points(const artemis_pack_t *p, const void *table_dev, const double *closed_hi, long npoints,
                              const double *points_dev, int *loc_dev, void *stream);

/* Step 3: the components of sel[0 .. nsel) at the located zones into out_dev ([ncomp][npoints], double or -- single != 0 --
 * float).  order_dev: NULL, or a permutation of 0 .. npoints - 1 (longs): lane t serves point order[t] and stores to that
 * point's place, so a caller that sorts the points by (block, k, j, i) makes neighbouring lanes read neighbouring zones -- an
 * element-granular gather is bound by latency, and the sort leaves the rest to the L2.  A thread loads the primitives of one
 * species once and forms every requested component of it; the derived codes run in a pass of their own, so a request without
 * one never pays for the stencil.  A loc entry outside the pack (block >= nblocks, a zone outside the interior) and an order
 * entry outside [0, npoints) are treated as not found / skipped: nothing outside the pack or the buffer is touched.
 * The refusals of artemis_hip_pack_fields (ARTEMIS_HIP_EINVAL: an unknown code, a dust code on a pack without dust, nsel
 * outside 0 .. 32, missing primitive tables) and npoints < 0; npoints == 0 or no components: succeeds, touches nothing. */
int artemis_hip_sample_fields(const artemis_pack_t *p, long npoints, const int *loc_dev, const long *order_dev, int nsel,
                              const int *sel, int single, void *out_dev, void *stream);

/* ---- a time series of samples, recorded inside the time loop ---------------------------------------------------------------
 * A recorder appends, after a completed cycle that is due, one row {cycle, time, dt} and the [ncomp][npoints] sample of that
 * moment to buffers on the device.  Both calls below can be captured into a graph: neither reads anything on the host, and
 * what changes from cycle to cycle -- the row index, the cycle number, and the clock of the unsynchronised loop -- is read
 * from device memory when the kernel runs, because a replayed graph has its arguments baked in.
 *
 * ctl_dev: one artemis_record_ctl_t; the caller zeroes it and sets `cycle` to the run's cycle count.  head_dev: `capacity`
 * artemis_record_head_t.  rows_dev: [capacity][ncomp][npoints] doubles (floats with single != 0). */
typedef struct artemis_record_ctl {
  long long seen;    /* cycles ticked since the recorder was attached */
  long long cycle;   /* the run's cycle count after the last tick */
  long long rows;    /* rows in the buffers */
  long long slot;    /* the row the last tick opened; -1: that cycle is not recorded */
  long long dropped; /* due rows that found the buffers full (the caller sizes its batches so that this stays 0) */
} artemis_record_ctl_t;
typedef struct artemis_record_head {
  long long cycle;
  double time, dt; /* the time the row's values hold at; the next step's dt */
} artemis_record_head_t;

/* One thread: ++seen, ++cycle; the cycle is due if seen % every == 0.  A due cycle with rows < capacity opens slot = rows++
 * and stores head[slot] = {cycle, time, dt}; a due cycle with rows == capacity counts in `dropped`; every other outcome
 * leaves slot = -1.  time and dt are tstate_dev[0] and tstate_dev[1] (the device clock, after artemis_hip_advance_dt) when
 * tstate_dev is not NULL, else the two arguments.  ARTEMIS_HIP_EINVAL: every < 1, capacity < 1, null ctl_dev or head_dev. */
int artemis_hip_record_tick(void *ctl_dev, void *head_dev, const double *tstate_dev, double time, double dt, long every, long capacity,
                            void *stream);

/* artemis_hip_sample_fields of the same arguments into rows_dev + slot * ncomp * npoints, slot read from ctl_dev by the
 * kernel (one scalar load per wave); a workgroup returns at once when slot < 0 or slot >= capacity.  The same bits as
 * artemis_hip_sample_fields; ctl is only read, so the result does not depend on the launch shape.  The refusals of
 * artemis_hip_sample_fields, and capacity < 1 and null ctl_dev or rows_dev; npoints == 0 or no components: succeeds, touches
 * nothing. */
int artemis_hip_record_samples(const artemis_pack_t *p, long npoints, const int *loc_dev, const long *order_dev, int nsel, const int *sel,
                               int single, const void *ctl_dev, long capacity, void *rows_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ARTEMIS_HIP_SAMPLE_H_ */
