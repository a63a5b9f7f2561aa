// check.hip -- the kernels of h2g_check_witness, for gfx950: a restatement of
// MockProver::verify (halo2_frontend/src/dev.rs:742-1166) for a complete witness.
//
//   check_gates           gate polynomials at every row       dev.rs:849-925
//   check_lookup_members  lookup inputs against their table   dev.rs:957-1052
//   check_sorted_equal    shuffle multisets                   dev.rs:1054-1112
//   check_copies          permutation copy constraints        dev.rs:1114-1142
//
// The lookup and shuffle checks compare expression tuples through their theta-compression
// (one field element per row, as the prover's own arguments do), with theta drawn from the
// caller's seed: PROBABILISTIC.  Two different m-tuples compress to the same value for at
// most m - 1 of the r values of theta, so over the n rows of an argument a wrong witness
// passes with probability about m n / r (r ~ 2^254).  Gates and copies are exact.
//
// Failures go to one record buffer: a wave reserves the slots of its failing lanes with one
// atomic add (ballot + popcount), which also keeps the exact total once the buffer is full;
// from then on a wave only counts, and adds its count once when it ends, so a witness that is
// wrong everywhere does not serialise on the counter.  Records are written with ordinary
// 16-byte vector stores.
#include "check.h"
#include "check_sink.h"
#include "fr_io.h"
#include "gate_prog.h"

namespace h2g {

static constexpr int CK_T = 256;

static unsigned check_grid(size_t n) {
  size_t g = (n + CK_T - 1) / CK_T;
  const size_t cap = 256 * 16;
  return (unsigned)(g < cap ? (g ? g : 1) : cap);
}

// ------------------------------------------------------------------ gates
// A wave covers 64 consecutive rows and loops over the gates' segments there (a gate's
// queries mostly repeat its neighbours', so the columns' lines are read once from HBM and
// again from the cache); grid-stride over the rows.  (One gate per blockIdx.y instead, as
// compress_batch_kernel's items: measured, rejected.)
__global__ void __launch_bounds__(EH_T) check_gates_kernel(GateCheckArgs a) {
  extern __shared__ uint4 ck_lds[];
  Fr* sl = reinterpret_cast<Fr*>(ck_lds);
  const int lane = threadIdx.x;
  const uint64_t mask = a.n - 1;
  WaveSink w;
  for (uint64_t i = blockIdx.x * (uint64_t)EH_T + lane; i < a.n; i += (uint64_t)gridDim.x * EH_T) {
    const uint32_t kind = i < a.u ? 1u : 2u;
    for (int g = 0; g < a.ngates; g++) {
      const Fr v = run_prog(a.prog, a.segs[g], a.consts, a.load_col, a.load_rot, i, 1, mask, Fr::zero(), sl, lane);
      sink_push(a.sink, w, !v.is_zero(), kind, (uint32_t)g, (uint32_t)i);
    }
  }
  sink_flush(a.sink, w);
}

hipError_t check_gates(const GateCheckArgs& a, hipStream_t st) {
  if (a.ngates <= 0 || a.n == 0) return hipSuccess;
  if (a.n_slots > EH_MAX_SLOTS) return hipErrorInvalidValue;
  const size_t lds = (size_t)(a.n_slots > 0 ? a.n_slots : 1) * EH_T * sizeof(Fr);
  size_t blocks = (a.n + EH_T - 1) / EH_T;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(check_gates_kernel, dim3((unsigned)blocks), dim3(EH_T), lds, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ lookups
__device__ __forceinline__ bool canon_eq(const CanonKey& a, const CanonKey& b) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a.l[i] ^ b.l[i];
  return x == 0;
}

__global__ void __launch_bounds__(CK_T) check_lookup_kernel(const Fr* __restrict__ in, const CanonKey* __restrict__ t,
                                                            size_t u, uint32_t index, CheckSink sink) {
  const CanonLess less;
  WaveSink w;
  for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r < u; r += (size_t)gridDim.x * blockDim.x) {
    const Fr c = to_canonical(ldf(in + r));
    CanonKey v;
#pragma unroll
    for (int j = 0; j < 8; j++) v.l[j] = c.l[j];
    size_t lo = 0, hi = u;  // lower_bound
    while (lo < hi) {
      const size_t mid = (lo + hi) >> 1;
      if (less(t[mid], v)) lo = mid + 1;
      else hi = mid;
    }
    const bool miss = !(lo < u && canon_eq(t[lo], v));
    sink_push(sink, w, miss, 3u, index, (uint32_t)r);
  }
  sink_flush(sink, w);
}

hipError_t check_lookup_members(const Fr* in, const CanonKey* t, size_t u, uint32_t index, const CheckSink& sink,
                                hipStream_t st) {
  if (u == 0) return hipSuccess;
  hipLaunchKernelGGL(check_lookup_kernel, dim3(check_grid(u)), dim3(CK_T), 0, st, in, t, u, index, sink);
  return hipGetLastError();
}

// ------------------------------------------------------------------ shuffles
__global__ void __launch_bounds__(CK_T) check_sorted_equal_kernel(const CanonKey* __restrict__ a,
                                                                  const CanonKey* __restrict__ b, size_t u,
                                                                  uint32_t* __restrict__ flag) {
  bool diff = false;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < u; i += (size_t)gridDim.x * blockDim.x)
    diff = diff || !canon_eq(a[i], b[i]);
  const unsigned long long m = __ballot(diff);  // one atomic per wave at most
  if (m && (int)(threadIdx.x & 63) == __ffsll(m) - 1) atomicOr(flag, 1u);
}

hipError_t check_sorted_equal(const CanonKey* a, const CanonKey* b, size_t u, uint32_t* flag, hipStream_t st) {
  if (u == 0) return hipSuccess;
  hipLaunchKernelGGL(check_sorted_equal_kernel, dim3(check_grid(u)), dim3(CK_T), 0, st, a, b, u, flag);
  return hipGetLastError();
}

// ------------------------------------------------------------------ copies
__global__ void __launch_bounds__(CK_T) check_copies_kernel(const Fr* const* __restrict__ cols, int off_fixed,
                                                            int off_instance, const int32_t* __restrict__ copies,
                                                            uint32_t count, CheckSink sink) {
  WaveSink w;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const int32_t* cp = copies + 6 * i;
    const int lt = cp[0], li = cp[1], lr = cp[2], rt = cp[3], ri = cp[4], rr = cp[5];
    const Fr* lc = cols[(lt == 0 ? 0 : (lt == 1 ? off_fixed : off_instance)) + li];
    const Fr* rc = cols[(rt == 0 ? 0 : (rt == 1 ? off_fixed : off_instance)) + ri];
    const Fr x = ldf(lc + lr), y = ldf(rc + rr);
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) d |= x.l[j] ^ y.l[j];
    sink_push(sink, w, d != 0, 5u, (uint32_t)i, (uint32_t)lr);
  }
  sink_flush(sink, w);
}

hipError_t check_copies(const Fr* const* cols, int off_fixed, int off_instance, const int32_t* copies, uint32_t count,
                        const CheckSink& sink, hipStream_t st) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(check_copies_kernel, dim3(check_grid(count)), dim3(CK_T), 0, st, cols, off_fixed, off_instance,
                     copies, count, sink);
  return hipGetLastError();
}

}  // namespace h2g
