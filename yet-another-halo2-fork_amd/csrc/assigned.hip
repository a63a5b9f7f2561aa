// assigned.hip -- the witness as the frontend holds it, evaluated on the device.
//
// Restates batch_invert_assigned (halo2_frontend/src/circuit.rs:363-404): the denominators
// of the Rational cells inverted in one batch, each numerator multiplied by its inverse
// (Assigned::evaluate, halo2_frontend/src/plonk/assigned.rs:352-364; x / 0 = 0 as
// assigned.rs:280-295 and ff's BatchInvert, which skips zeros).  The wire form is dense
// numerators (Assigned::numerator(), 0 for Zero) plus a sparse list (cell index,
// denominator) of the Rational cells, strictly increasing by cell.
//
// The denominators arrive contiguous, so the inversion is poly.hip's three-level Montgomery
// trick over den[0..nden) with the prefixes in scratch: forward pass, the thread totals
// inverted by poly_inv_regs, and a backward pass that does not write the inverses out:
// the thread that holds den[j]^-1 in registers loads index[j] and num[index[j]] and stores
// the product at out[index[j]].  Against h2g_fr_batch_invert_dev plus a gather-multiply
// kernel that saves the inverses' round trip (nden x 64 B) and a launch, and `den` stays
// as it came.  The numerator accesses are 32-byte gathers at the caller's stride, two
// 16-byte accesses each (ldf / stf).
#include "assigned.h"

#include "../../include/h2g.h"
#include "fr_io.h"
#include "poly.h"
#include "runtime.h"

namespace h2g {
namespace {

constexpr int PT = 256;

// poly.hip's inv_fwd_kernel over read-only denominators: thread t walks {t + kT}, storing
// the running product before each element; slot t takes the thread's total
__global__ void __launch_bounds__(PT) asg_fwd_kernel(const Fr* __restrict__ den, Fr* __restrict__ pref, size_t n,
                                                     size_t T) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= T) return;
  Fr acc = Fr::one();
  {
    const Fr x = ldf(den + t);
    if (!x.is_zero()) acc = x;
  }
  for (size_t i = t + T; i < n; i += T) {
    stf(pref + i, acc);
    const Fr x = ldf(den + i);
    if (!x.is_zero()) acc = acc * x;
  }
  stf(pref + t, acc);
}

struct AsgItem {  // one listed cell as the backward pass reads it
  Fr x, p, nm;
  uint64_t c;
};
__device__ __forceinline__ AsgItem asg_load(const Fr* __restrict__ den, const Fr* __restrict__ pref,
                                            const uint64_t* __restrict__ index, const Fr* num, size_t ncells,
                                            size_t i, bool first) {
  AsgItem it;
  it.x = ldf(den + i);
  it.c = index[i];
  it.p = first ? Fr::one() : ldf(pref + i);  // slot t holds 1 / P_t, not a prefix
  it.nm = it.c < ncells ? ldf(num + it.c) : Fr::zero();
  return it;
}

// from 1 / P_t (pref[t]) back down the thread's subset: 1 / x_i = (1 / P) * prefix_i,
// 1 / P *= x_i; the inverse leaves the thread only as out[index[i]] = num[index[i]] / x_i.
// The next element's loads (none depends on the running inverse) are issued before this
// element's products.  num may be out: a cell is read and written by the one thread that
// has its list entry.
__global__ void __launch_bounds__(PT) asg_bwd_kernel(const Fr* __restrict__ den, const Fr* __restrict__ pref,
                                                     const uint64_t* __restrict__ index, const Fr* num, Fr* out,
                                                     size_t ncells, size_t n, size_t T) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= T) return;
  Fr iv = ldf(pref + t);
  size_t i = t + (n - 1 - t) / T * T;  // the thread's last element (t < T <= n)
  AsgItem cur = asg_load(den, pref, index, num, ncells, i, i == t);
  for (;;) {
    const bool more = i > t;
    AsgItem nxt = cur;
    if (more) nxt = asg_load(den, pref, index, num, ncells, i - T, i - T == t);
    Fr r = Fr::zero();
    if (!cur.x.is_zero()) {  // every entry takes its place in the chain, listed cell in range or not
      r = more ? iv * cur.p : iv;
      iv = iv * cur.x;
      r = cur.nm * r;
    }
    if (cur.c < ncells) stf(out + cur.c, r);
    if (!more) break;
    i -= T;
    cur = nxt;
  }
}

}  // namespace

int assigned_per(size_t nden) {
  // poly_batch_invert_multi's rule for one array: 16 once that gives 2^18 threads, fewer below
  size_t per = 16;
  while (per > 2 && nden / per < ((size_t)1 << 18)) per >>= 1;
  return (int)per;
}

bool assigned_per_ok(int per) { return per == 2 || per == 4 || per == 8 || per == 16; }

hipError_t assigned_to_fr(const Fr* num, size_t ncells, const uint64_t* index, const Fr* den, size_t nden, Fr* out,
                          Fr* scratch, int per, hipStream_t st) {
  if (ncells == 0) return hipSuccess;
  if (out != num) {
    hipError_t e = hipMemcpyAsync(out, num, ncells * sizeof(Fr), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return e;
  }
  if (nden == 0) return hipSuccess;
  if (per == 0) per = assigned_per(nden);
  if (!assigned_per_ok(per)) return hipErrorInvalidValue;
  const size_t T = (nden + (size_t)per - 1) / (size_t)per;
  const unsigned blk = (unsigned)((T + PT - 1) / PT);
  hipLaunchKernelGGL(asg_fwd_kernel, dim3(blk), dim3(PT), 0, st, den, scratch, nden, T);
  hipError_t e = poly_inv_regs(scratch, T, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(asg_bwd_kernel, dim3(blk), dim3(PT), 0, st, den, (const Fr*)scratch, index, num, out, ncells,
                     nden, T);
  return hipGetLastError();
}

}  // namespace h2g

using namespace h2g;
using namespace h2g::rt;

#define NEED_DEV_ASG()                                                \
  std::lock_guard<std::recursive_mutex> _lk(g_mu);                    \
  Device* d = cur();                                                  \
  if (!d) return fail(H2G_ERR_STATE, "h2g_init has not been called"); \
  HIPCHK(hipSetDevice(d->id));

namespace {

// a grow-only buffer to `bytes`; a failed growth has released the old allocation first
// (DevArr::grow), so nothing is left allocated
int asg_ensure(DevBuf& b, size_t bytes, const char* what) {
  const hipError_t e = b.ensure(bytes);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    return fail(H2G_ERR_NOMEM, std::string("assigned_to_fr: no device memory for ") + std::to_string(bytes) +
                                   " bytes of " + what);
  }
  HIPCHK(e);
  return H2G_OK;
}

int asg_dev_entry(const void* d_num, size_t ncells, const void* d_index, const void* d_den, size_t nden, void* d_out,
                  int per, void* stream) {
  if (ncells == 0) return H2G_OK;
  if (!d_num || !d_out || (nden && (!d_index || !d_den))) return fail(H2G_ERR_ARG, "assigned_to_fr: null pointer");
  if (((uintptr_t)d_num | (uintptr_t)d_out | (uintptr_t)d_index | (uintptr_t)d_den) & 15)
    return fail(H2G_ERR_ARG, "assigned_to_fr: device arrays must be 16-byte aligned");
  if (per != 0 && !assigned_per_ok(per)) return fail(H2G_ERR_ARG, "debug_assigned_to_fr: per must be 0, 2, 4, 8 or 16");
  NEED_DEV_ASG();
  RCCHK(asg_ensure(d->work, nden * sizeof(Fr) + 32, "scratch"));
  HIPCHK(assigned_to_fr((const Fr*)d_num, ncells, (const uint64_t*)d_index, (const Fr*)d_den, nden, (Fr*)d_out,
                        d->work.as<Fr>(), per, pick_stream(d, stream)));
  return H2G_OK;
}

}  // namespace

extern "C" {

int h2g_assigned_to_fr_dev(const void* d_num, size_t ncells, const void* d_index, const void* d_den, size_t nden,
                           void* d_out, void* stream) {
  return asg_dev_entry(d_num, ncells, d_index, d_den, nden, d_out, 0, stream);
}

int h2g_debug_assigned_to_fr_dev(const void* d_num, size_t ncells, const void* d_index, const void* d_den, size_t nden,
                                 void* d_out, int per, void* stream) {
  return asg_dev_entry(d_num, ncells, d_index, d_den, nden, d_out, per, stream);
}

int h2g_debug_assigned_per(size_t nden, int* per) {
  if (!per) return fail(H2G_ERR_ARG, "debug_assigned_per: null argument");
  *per = assigned_per(nden);
  return H2G_OK;
}

int h2g_assigned_to_fr(const uint64_t* num, size_t ncells, const uint64_t* index, const uint64_t* den, size_t nden,
                       uint64_t* out) {
  if (ncells == 0) return H2G_OK;
  if (!num || !out || (nden && (!index || !den))) return fail(H2G_ERR_ARG, "assigned_to_fr: null pointer");
  for (size_t j = 0; j < nden; j++) {
    if (index[j] >= ncells)
      return fail(H2G_ERR_ARG, "assigned_to_fr: index[" + std::to_string(j) + "] = " + std::to_string(index[j]) +
                                   " is not below ncells = " + std::to_string(ncells));
    if (j && index[j] <= index[j - 1])
      return fail(H2G_ERR_ARG, "assigned_to_fr: index[" + std::to_string(j) + "] = " + std::to_string(index[j]) +
                                   " does not exceed index[" + std::to_string(j - 1) + "] = " +
                                   std::to_string(index[j - 1]) + " (the list must be strictly increasing)");
  }
  if (nden == 0) {  // a witness without divisions: a copy, or nothing in place
    if (out != num) std::memmove(out, num, ncells * sizeof(Fr));
    return H2G_OK;
  }
  NEED_DEV_ASG();
  hipStream_t st = d->stream;
  // b: the cells (converted in place), a: the denominators, c: the indices
  RCCHK(asg_ensure(d->b, ncells * sizeof(Fr) + 32, "the cells"));
  RCCHK(asg_ensure(d->a, nden * sizeof(Fr) + 32, "the denominators"));
  RCCHK(asg_ensure(d->c, nden * sizeof(uint64_t) + 32, "the indices"));
  HIPCHK(hipMemcpyAsync(d->b.p, num, ncells * sizeof(Fr), hipMemcpyHostToDevice, st));
  if (nden) {
    HIPCHK(hipMemcpyAsync(d->a.p, den, nden * sizeof(Fr), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d->c.p, index, nden * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  }
  RCCHK(h2g_assigned_to_fr_dev(d->b.p, ncells, d->c.p, d->a.p, nden, d->b.p, nullptr));
  HIPCHK(hipMemcpyAsync(out, d->b.p, ncells * sizeof(Fr), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return H2G_OK;
}

}  // extern "C"
