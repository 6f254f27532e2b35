// Launchers of kernels_sample.hip (include/artemis_hip_sample.h): point location and point sampling of a pack's fields.
// A header of its own: kernels.hpp and the headers every kernel unit shares do not know this unit.
#pragma once
#include "kernels.hpp"

namespace artemis {
// loc[p] = {block, k, j, i} of points[p] by the table (locate_table.hpp); closed_hi: 3 doubles on the host
void launch_locate_points(const PackView &P, const void *table_dev, const double *closed_hi, long npoints, const double *points,
                          int *loc, hipStream_t s);
// out[c * npoints + p] of the selection at loc[p]; order: NULL or a permutation of the points (lane t serves order[t])
void launch_sample_fields(const PackView &P, long npoints, const int *loc, const long *order, const FieldSelection &S, bool single,
                          void *out, hipStream_t s);
} // namespace artemis
