// selfcheck.h -- kernels of the prover's self-checks (selfcheck.hip, H2G_SELFCHECK_ARGUMENTS):
// the assertions the reference makes under its `sanity-checks` feature while it builds each
// argument, restated from their formulas, on the arrays the stage already holds.  Failures
// go to a CheckSink (check.h) as {kind, index, row, 0}.  Let u = n - (blinding_factors + 1).
#pragma once
#include "check.h"

namespace h2g {

// record kinds of h2g_check_failure written here (include/h2g.h)
enum { SC_KIND_PERMUTATION = 6, SC_KIND_PRODUCT = 7, SC_KIND_PERMUTED = 8, SC_KIND_UNUSABLE_ROW = 9 };

// max_blocks > 0 caps the grid (test seam: several grid-stride passes at a few thousand rows)
unsigned selfcheck_grid(size_t rows, int max_blocks);

// A grand product z over rows [0, u] (plonk/lookup/prover.rs:269-305, shuffle/prover.rs:176-191):
//   z[0] = 1;  for i < u:  z[i+1] (den_a[i] + ca) (den_b[i] + cb) = z[i] (num_a[i] + ca) (num_b[i] + cb);
//   z[u] = 1 (only when `closing`).
// Lookups: num = (A, S) compressed, den = (A', S') permuted, ca = beta, cb = gamma.  num_b ==
// den_b == nullptr is the one-factor form of a shuffle: num_a = A, den_a = S, ca = gamma.
// A row failing any of its conditions gives ONE record {7, index, row}; row u only the closing one.
struct ProductCheckArgs {
  const Fr* z = nullptr;
  const Fr *num_a = nullptr, *num_b = nullptr, *den_a = nullptr, *den_b = nullptr;
  Fr ca, cb;
  uint64_t u = 0;
  bool closing = true;
  uint32_t index = 0;
  CheckSink sink;
};
hipError_t selfcheck_product(const ProductCheckArgs& a, int max_blocks, hipStream_t st);

// The permuted pair (plonk/lookup/prover.rs:475-488): for i < u, a[i] == s[i], or i > 0 and
// a[i] == a[i-1]; else {8, index, i}
hipError_t selfcheck_permuted(const Fr* a, const Fr* s, uint64_t u, uint32_t index, const CheckSink& sink,
                              int max_blocks, hipStream_t st);

// One column set's permutation product z (permutation/prover.rs:103-171; the reference asserts
// nothing here): z[0] = *first (nullptr: 1 -- set 0 starts at one, set j at set j - 1's z[u]);
// for i < u:  z[i+1] prod_c (v_c[i] + beta sigma_c[i] + gamma) = z[i] prod_c (v_c[i] + beta delta^c omega^i + gamma).
// c carries v, sigma AND beta_delta of up to PERM_MAXC columns; a wider set goes in several
// launches, the two partial products of a row carried in acc_l / acc_r (u elements each):
// `begin` starts them, `end` compares.  A failing row gives {6, index, row}.
struct PermCheckArgs {
  const Fr* z = nullptr;
  const Fr* first = nullptr;
  PermCols c;
  Fr beta, gamma;
  PowTable om;
  uint64_t u = 0;
  Fr *acc_l = nullptr, *acc_r = nullptr;
  bool begin = true, end = true;
  uint32_t index = 0;
  CheckSink sink;
};
hipError_t selfcheck_permutation(const PermCheckArgs& a, hipStream_t st);

// The advice as handed in (plonk/prover.rs:418-421): rows [u, n) of each listed (unblinded)
// column are zero; else {9, col_index[c], row}.  Up to SC_MAXC columns a launch.
constexpr int SC_MAXC = 32;
struct UnusableCols {
  const Fr* col[SC_MAXC];
  uint32_t index[SC_MAXC];
  int m = 0;
};
hipError_t selfcheck_unusable_rows(const UnusableCols& c, uint64_t u, uint64_t n, const CheckSink& sink,
                                   hipStream_t st);

}  // namespace h2g
