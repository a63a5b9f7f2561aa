// gate_prog.h -- the expression-program interpreter shared by the kernels that evaluate
// compiled expressions row by row (prover_kernels.hip: evaluate_h, compress; check.hip).
// One wave per block; the program's value slots live in LDS as slot-major [slot][lane]
// 32-byte elements (conflict-free 16-byte accesses).
#pragma once
#include "fr_io.h"
#include "prover_kernels.h"

namespace h2g {

static constexpr int EH_T = 64;
static constexpr int EH_MAX_SLOTS = 24;

// run one program segment for row idx: Horner of its expression values with `factor`,
// starting from `acc`
__device__ __forceinline__ Fr run_prog(const int4* __restrict__ prog, int2 seg, const Fr* __restrict__ consts,
                                       const Fr* const* __restrict__ cols, const int* __restrict__ rots, uint64_t idx,
                                       uint64_t rot_scale, uint64_t mask, Fr factor, Fr* sl, int lane,
                                       Fr acc = Fr::zero()) {
  for (int pc = seg.x; pc < seg.x + seg.y; pc++) {
    const int4 in = prog[pc];
    Fr v;
    switch (in.x) {
      case G_LOAD: {
        const uint64_t j = (idx + (uint64_t)((int64_t)rots[in.z] * (int64_t)rot_scale)) & mask;
        v = ldf(cols[in.z] + j);
        break;
      }
      case G_CONST: v = ldf(consts + in.z); break;
      case G_ADD: v = sl[in.z * EH_T + lane] + sl[in.w * EH_T + lane]; break;
      case G_SUB: v = sl[in.z * EH_T + lane] - sl[in.w * EH_T + lane]; break;
      case G_MUL: v = sl[in.z * EH_T + lane] * sl[in.w * EH_T + lane]; break;
      case G_NEG: v = neg(sl[in.z * EH_T + lane]); break;
      default:  // G_HORNER
        acc = acc * factor + sl[in.z * EH_T + lane];
        continue;
    }
    sl[in.y * EH_T + lane] = v;
  }
  return acc;
}

}  // namespace h2g
