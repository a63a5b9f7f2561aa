// pairing_dev.h -- the device pairing check of pairing_dev.hip: for N inputs (L_i, R_i) and the
// two fixed G2 points of the verifier params, ok_i = [e(L_i, s_g2) == e(R_i, g2)], one launch.
#pragma once
#include <hip/hip_runtime.h>

#include "pairing.h"

namespace h2g {

// What the kernel reads besides its inputs; built on the host once per (g2, s_g2)
// (pairing_table_build) and uploaded.  No G2 arithmetic happens on the device.
struct PairingTable {
  Fq2 gamma[3][6];                  // gamma[n - 1][i]: (c w^i)^(p^n) = conj^n(c) gamma[n - 1][i] w^i
  LineCoeffs line[2][ATE_LINES];    // [0]: the lines of s_g2, [1]: of g2 (g2_line_table)
};

// false: a vertical line (a G2 point outside the r-torsion)
inline bool pairing_table_build(const G2Affine& g2, const G2Affine& s_g2, PairingTable* out) {
  std::vector<LineCoeffs> t;
  const G2Affine* q[2] = {&s_g2, &g2};
  for (int s = 0; s < 2; s++) {
    if (!g2_line_table(*q[s], &t) || t.size() != (size_t)ATE_LINES) return false;
    for (int i = 0; i < ATE_LINES; i++) out->line[s][i] = t[i];
  }
  for (int i = 0; i < 6; i++) {
    Fq12 x;
    for (auto& c : x.c) c = fq2_zero();
    x.c[i] = fq2_one();
    for (int n = 0; n < 3; n++) {
      x = fq12_frobenius(x);
      out->gamma[n][i] = x.c[i];
    }
  }
  return true;
}

// d_lr: count x (left, right) affine Montgomery G1 points, identity = zeros; d_ok: count x int32.
// d_miller / d_gt (either may be null): count x 6 Fq2, the Miller value and the final value
// (the exact final exponentiation's value raised to PAIRING_DEV_M, pairing_dev.hip).
// count >= 1.  Asynchronous on st.
hipError_t pairing_check_launch(const PairingTable* d_tab, const G1Affine* d_lr, size_t count, int32_t* d_ok,
                                Fq2* d_miller, Fq2* d_gt, hipStream_t st);

}  // namespace h2g
