/* Recorded history integrals and n-body force sums: part of the C ABI of libartemis_hip.so, a sibling of artemis_hip_sample.h
 * (which it includes for the recorder's control block and tick).  A recorder of this kind appends, after a completed cycle
 * that is due, the volume integrals of the conserved variables -- over the whole pack and over up to seven index windows --
 * and, optionally, the n-body force sums to the row artemis_hip_record_tick opened.  Like artemis_hip_record_samples the
 * calls can be captured into a graph: nothing is read on the host, the row index is read from the control block when the
 * kernels run, there are no floating-point atomics and no last-block ticket.
 *
 * ---- definition (fixed in bits) ---------------------------------------------------------------------------------------------
 * nq = 6 ns_gas + 4 ns_dust quantities in the layout of artemis_hip_history_sums.  A row is integrals[1 + nwin][nq]:
 *   set 0      every interior zone of the pack: the bits artemis_hip_history_sums gives on the same pack at that moment (the
 *              same tiles, terms, reduction tree and number of workgroups -- GRID_CAP included);
 *   set 1 + w  the zones of window w, by the same pass and the same tree, a zone outside the window contributing nothing:
 *              a window that holds every zone has the bits of set 0, a window that holds none is +0.0 throughout.
 * A window is given per block as index ranges, window_zones[b][w] = {i0, i1, j0, j1, k0, k1}: half-open, relative to the
 * first interior zone of the block, i along x1; empty as i0 == i1.  The kernel compares indices only, never coordinates;
 * ranges that reach outside the block are harmless (zones outside the interior are never visited). */
#ifndef ARTEMIS_HIP_RECORD_H_
#define ARTEMIS_HIP_RECORD_H_

#include "artemis_hip_sample.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ARTEMIS_RECORD_MAX_WINDOWS 7

/* Bytes of scratch_dev for this pack and window count: one row of (1 + nwin) * nq partial sums per workgroup, the number of
 * workgroups being that of artemis_hip_history_sums (a function of the pack and GRID_CAP alone).  0 for what
 * artemis_hip_record_integrals refuses. */
size_t artemis_hip_record_integrals_scratch_bytes(const artemis_pack_t *p, int nwin);

/* The partial pass and the combine; the combine's output base is rows_dev + slot * (1 + nwin) * nq doubles, slot read from
 * ctl_dev (a uniform load); every workgroup of both launches returns at once for slot < 0 or slot >= capacity.
 * window_zones_dev: int[nblocks][nwin][6] on the device (may be NULL for nwin == 0); rows_dev: [capacity][1 + nwin][nq].
 * ARTEMIS_HIP_EINVAL, nothing touched: the refusals of artemis_hip_history_sums, nwin outside 0 .. 7, nwin > 0 without a
 * table, capacity < 1, null scratch_dev, ctl_dev or rows_dev, ctl_dev not aligned to 8 bytes. */
int artemis_hip_record_integrals(const artemis_pack_t *p, int nwin, const int *window_zones_dev, double *scratch_dev, const void *ctl_dev,
                                 long capacity, double *rows_dev, void *stream);

/* rows_dev[slot * n + q] = base_dev[q] + acc_dev[q] for q < n (n doubles: 7 per particle), plain vector stores: the one
 * addition the driver's flush performs (host rows + this rank's device accumulators), formed without flushing anything.
 * n == 0 succeeds and touches nothing.  ARTEMIS_HIP_EINVAL: n < 0, capacity < 1, a null pointer, ctl_dev not aligned. */
int artemis_hip_record_nbody(const double *base_dev, const double *acc_dev, long n, const void *ctl_dev, long capacity, double *rows_dev,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ARTEMIS_HIP_RECORD_H_ */
