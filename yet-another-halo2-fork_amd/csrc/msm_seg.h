// msm_seg.h -- many small independent MSMs in one launch (msm_seg.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bn254.h"

namespace h2g {

// out[s] = sum_{j in [seg_off[s], seg_off[s + 1])} scalars[j] * bases[index ? index[j] : j], affine
// (identity = zeros).  scalars: Montgomery Fr.  An index >= nbases contributes nothing (never read).
hipError_t msm_segmented(const G1Affine* bases, size_t nbases, const Fr* scalars, const uint32_t* index,
                         const uint32_t* seg_off, size_t nseg, G1Affine* out, hipStream_t st);

}  // namespace h2g
