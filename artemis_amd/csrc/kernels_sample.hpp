// Launchers of kernels_sample.hip (include/artemis_hip_sample.h): point location and point sampling of a pack's fields.
// A header of its own: kernels.hpp and the headers every kernel unit shares do not know this unit.
#pragma once
#include "../../include/artemis_hip_sample.h"
#include "kernels.hpp"

namespace artemis {
// the tick of a recorder and the sample of the row it opened (artemis_hip_record_tick / _record_samples)
void launch_record_tick(void *ctl, void *head, const double *tstate, double time, double dt, long every, long capacity, hipStream_t s);
void launch_record_samples(const PackView &P, long npoints, const int *loc, const long *order, const FieldSelection &S, bool single,
                           const void *ctl, long capacity, void *rows, hipStream_t s);
// loc[p] = {block, k, j, i} of points[p] by the table (locate_table.hpp); closed_hi: 3 doubles on the host
void launch_locate_points(const PackView &P, const void *table_dev, const double *closed_hi, long npoints, const double *points,
                          int *loc, hipStream_t s);
// out[c * npoints + p] of the selection at loc[p]; order: NULL or a permutation of the points (lane t serves order[t])
void launch_sample_fields(const PackView &P, long npoints, const int *loc, const long *order, const FieldSelection &S, bool single,
                          void *out, hipStream_t s);
} // namespace artemis
