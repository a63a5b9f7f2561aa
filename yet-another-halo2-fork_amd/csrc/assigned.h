// assigned.h -- a witness of Assigned<F> cells to field elements (see assigned.hip).
#pragma once
#include "bn254.h"

namespace h2g {

// the size rule: denominators per first-level thread for nden of them (host only)
int assigned_per(size_t nden);
// what the kernels run with: 2, 4, 8 or 16
bool assigned_per_ok(int per);
// out[index[j]] = num[index[j]] * den[j]^-1 (0 for den[j] == 0), every other cell out = num.
// out == num: only the listed cells are touched.  index[j] >= ncells is skipped.  scratch >=
// nden Fr.  per: 0 = assigned_per(nden), else a value assigned_per_ok accepts.
hipError_t assigned_to_fr(const Fr* num, size_t ncells, const uint64_t* index, const Fr* den, size_t nden, Fr* out,
                          Fr* scratch, int per, hipStream_t st);

}  // namespace h2g
