// selfcheck.hip -- the kernels of the prover's self-checks, for gfx950 (selfcheck.h).
//
//   selfcheck_product        a lookup's or shuffle's grand product   lookup/prover.rs:269-305,
//                                                                    shuffle/prover.rs:176-191
//   selfcheck_permutation    a column set's permutation product     permutation/prover.rs:103-171
//   selfcheck_permuted       the permuted input / table pair         lookup/prover.rs:475-488
//   selfcheck_unusable_rows  the advice's rows [u, n) as handed in   prover.rs:418-421
//
// Written as check_gates_kernel is (check.hip): a wave covers 64 consecutive rows, grid-stride
// under a capped grid; the failing lanes of a wave reserve their record slots with one atomic
// add (check_sink.h), which keeps the exact total once the buffer is full.  The field
// arithmetic is the Montgomery Fr of the product kernels these check (prover_kernels.hip,
// lk_den_kernel ...).  Counted from the code, not measured: a row costs 2 products and 3 loads
// (the permuted pair reads, a shuffle's product 4 and 4), 6 and 6 for a lookup's product, and
// 2 + 3 m and 3 + 2 m for a column set of m columns; at 32 bytes a load these kernels should be
// bound by memory, as the product kernels they follow are.
#include "selfcheck.h"
#include "check_sink.h"
#include "fr_io.h"

namespace h2g {

static constexpr int SC_T = 256;

unsigned selfcheck_grid(size_t rows, int max_blocks) {
  size_t g = (rows + SC_T - 1) / SC_T;
  const size_t cap = max_blocks > 0 ? (size_t)max_blocks : 256 * 16;
  return (unsigned)(g < cap ? (g ? g : 1) : cap);
}

__global__ void __launch_bounds__(SC_T) selfcheck_product_kernel(ProductCheckArgs a) {
  const Fr one = Fr::one();
  WaveSink w;
  for (uint64_t i = blockIdx.x * (uint64_t)SC_T + threadIdx.x; i <= a.u; i += (uint64_t)gridDim.x * SC_T) {
    const Fr zi = ldf(a.z + i);
    bool bad;
    if (i == a.u) {
      bad = a.closing && !(zi == one);
    } else {
      Fr l = ldf(a.z + i + 1) * (ldf(a.den_a + i) + a.ca);
      Fr r = zi * (ldf(a.num_a + i) + a.ca);
      if (a.num_b) {
        l = l * (ldf(a.den_b + i) + a.cb);
        r = r * (ldf(a.num_b + i) + a.cb);
      }
      bad = !(l == r) || (i == 0 && !(zi == one));
    }
    sink_push(a.sink, w, bad, SC_KIND_PRODUCT, a.index, (uint32_t)i);
  }
  sink_flush(a.sink, w);
}

hipError_t selfcheck_product(const ProductCheckArgs& a, int max_blocks, hipStream_t st) {
  if (!a.z || !a.num_a || !a.den_a || (a.num_b == nullptr) != (a.den_b == nullptr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(selfcheck_product_kernel, dim3(selfcheck_grid(a.u + 1, max_blocks)), dim3(SC_T), 0, st, a);
  return hipGetLastError();
}

__global__ void __launch_bounds__(SC_T) selfcheck_permuted_kernel(const Fr* __restrict__ a, const Fr* __restrict__ s,
                                                                  uint64_t u, uint32_t index, CheckSink sink) {
  WaveSink w;
  for (uint64_t i = blockIdx.x * (uint64_t)SC_T + threadIdx.x; i < u; i += (uint64_t)gridDim.x * SC_T) {
    const Fr ai = ldf(a + i);
    bool ok = ai == ldf(s + i);
    if (!ok && i > 0) ok = ai == ldf(a + i - 1);
    sink_push(sink, w, !ok, SC_KIND_PERMUTED, index, (uint32_t)i);
  }
  sink_flush(sink, w);
}

hipError_t selfcheck_permuted(const Fr* a, const Fr* s, uint64_t u, uint32_t index, const CheckSink& sink,
                              int max_blocks, hipStream_t st) {
  if (u == 0) return hipSuccess;
  hipLaunchKernelGGL(selfcheck_permuted_kernel, dim3(selfcheck_grid(u, max_blocks)), dim3(SC_T), 0, st, a, s, u,
                     index, sink);
  return hipGetLastError();
}

__global__ void __launch_bounds__(SC_T) selfcheck_permutation_kernel(PermCheckArgs a) {
  const uint64_t mask = (1ull << a.om.bits) - 1;
  WaveSink w;
  for (uint64_t i = blockIdx.x * (uint64_t)SC_T + threadIdx.x; i < a.u; i += (uint64_t)gridDim.x * SC_T) {
    const Fr zi = ldf(a.z + i);
    Fr l = a.begin ? ldf(a.z + i + 1) : ldf(a.acc_l + i);
    Fr r = a.begin ? zi : ldf(a.acc_r + i);
    const Fr wi = ldf(a.om.lo + (i & mask)) * ldf(a.om.hi + (i >> a.om.bits));
    for (int j = 0; j < a.c.m; j++) {
      const Fr v = ldf(a.c.v[j] + i) + a.gamma;
      l = l * (a.beta * ldf(a.c.sigma[j] + i) + v);
      r = r * (a.c.beta_delta[j] * wi + v);
    }
    if (!a.end) {  // (uniform: a wave of a launch that does not compare pushes nothing)
      stf(a.acc_l + i, l);
      stf(a.acc_r + i, r);
      continue;
    }
    bool bad = !(l == r);
    if (i == 0) bad = bad || !(zi == (a.first ? ldf(a.first) : Fr::one()));
    sink_push(a.sink, w, bad, SC_KIND_PERMUTATION, a.index, (uint32_t)i);
  }
  sink_flush(a.sink, w);
}

hipError_t selfcheck_permutation(const PermCheckArgs& a, hipStream_t st) {
  if (a.u == 0) return hipSuccess;
  if (a.c.m < 0 || a.c.m > PERM_MAXC || ((!a.begin || !a.end) && (!a.acc_l || !a.acc_r))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(selfcheck_permutation_kernel, dim3(selfcheck_grid(a.u, 0)), dim3(SC_T), 0, st, a);
  return hipGetLastError();
}

__global__ void __launch_bounds__(SC_T) selfcheck_unusable_kernel(UnusableCols c, uint64_t u, uint64_t n,
                                                                  CheckSink sink) {
  const uint64_t R = n - u, items = R * (uint64_t)c.m;
  WaveSink w;
  for (uint64_t j = blockIdx.x * (uint64_t)SC_T + threadIdx.x; j < items; j += (uint64_t)gridDim.x * SC_T) {
    const int k = (int)(j / R);
    const uint64_t row = u + j % R;
    sink_push(sink, w, !ldf(c.col[k] + row).is_zero(), SC_KIND_UNUSABLE_ROW, c.index[k], (uint32_t)row);
  }
  sink_flush(sink, w);
}

hipError_t selfcheck_unusable_rows(const UnusableCols& c, uint64_t u, uint64_t n, const CheckSink& sink,
                                   hipStream_t st) {
  if (c.m <= 0 || u >= n) return hipSuccess;
  if (c.m > SC_MAXC) return hipErrorInvalidValue;
  hipLaunchKernelGGL(selfcheck_unusable_kernel, dim3(selfcheck_grid((n - u) * (size_t)c.m, 0)), dim3(SC_T), 0, st, c,
                     u, n, sink);
  return hipGetLastError();
}

}  // namespace h2g
