// Launchers of the recorded history integrals and n-body force sums (kernels_history.hip; include/artemis_hip_record.h has
// the definition).  A header of its own: kernels.hpp reaches every kernel unit, and a line added there would give every
// object a new identity.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/artemis_hip_record.h"
#include "pack_view.hpp"

namespace artemis {

constexpr int RECORD_MAX_WINDOWS = 7;

// the partial pass (history_workgroups(P) workgroups, rows of (1 + nwin) * nq partial sums in scratch) and the combine into
// rows + slot * (1 + nwin) * nq, slot read from the control block on the device
void launch_record_integrals(const PackView &P, int nwin, const int *zones, double *scratch, const void *ctl, long capacity, double *rows,
                             hipStream_t s);
// rows[slot][q] = base[q] + acc[q], q < n
void launch_record_nbody(const double *base, const double *acc, long n, const void *ctl, long capacity, double *rows, hipStream_t s);

} // namespace artemis
