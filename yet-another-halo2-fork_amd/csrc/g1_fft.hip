// g1_fft.hip -- g_to_lagrange on the device (halo2_backend/src/arithmetic.rs:30-54): the
// monomial SRS g_j = [s^j] G to the Lagrange basis, an inverse FFT whose elements are G1
// points (h2g_g1_to_lagrange*, and through it h2g_params_from_parts / _downsize).
//
// g1_fft.h has the shape, the index arithmetic and the butterfly (all host-checkable); this
// file has the launches: the twiddle table, the bit-reversal swaps, one launch per stage and
// the n^-1 scaling.  A stage is n/2 independent ~254-bit double-and-add chains, the scaling n
// more: (k/2 + 1) 2^k chains in all, minus the twiddle-1 butterflies.  The compiler reports
// for both forms of the stage kernel 149 VGPRs, no spills, no LDS, 3 waves per SIMD, and for
// the scaling 125 VGPRs, no spills, 4 waves per SIMD.  Measured: k = 22 in 1.43 s, 35 M
// chains/s ("Downsizing the params").
#include "g1_fft.h"

#include "prover_state.h"

namespace h2g {
namespace {
using prv::Pool;

// tw[x] = omega^-x in canonical form, x < count, from the two-level power table
__global__ void __launch_bounds__(256) g1fft_twiddle_kernel(PowTable om, uint64_t count, Fr* __restrict__ tw) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= count) return;
  const uint64_t mask = (1ull << om.bits) - 1;
  tw[x] = to_canonical(om.lo[x & mask] * om.hi[x >> om.bits]);
}

__global__ void __launch_bounds__(256) g1fft_bitrev_kernel(G1Affine* __restrict__ p, uint32_t k) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1ull << k)) return;
  const uint64_t r = g1fft_bitrev(i, k);
  if (i < r) {
    const G1Affine a = p[i], b = p[r];
    p[i] = b;
    p[r] = a;
  }
}

template <bool UNIFORM>
__global__ void __launch_bounds__(G1FFT_WAVE) g1fft_stage_kernel(G1Affine* __restrict__ p, const Fr* __restrict__ tw,
                                                                 uint32_t k, uint32_t s) {
  const uint64_t t0 = (uint64_t)blockIdx.x * G1FFT_WAVE, t = t0 + threadIdx.x;
  if (t >= (1ull << (k - 1))) return;
  g1fft_stage_one(p, tw, k, s, UNIFORM ? t0 : t, t);
}

__global__ void __launch_bounds__(G1FFT_WAVE) g1fft_scale_kernel(G1Affine* __restrict__ p, uint32_t k, Fr ninv) {
  const uint64_t i = (uint64_t)blockIdx.x * G1FFT_WAVE + threadIdx.x;
  if (i >= (1ull << k)) return;
  p[i] = g1fft_scale(p[i], ninv);
}

unsigned blocks_for(uint64_t threads, unsigned per) { return (unsigned)((threads + per - 1) / per); }
}  // namespace

int g1_to_lagrange(const G1Affine* d_g, uint32_t k, G1Affine* d_out, hipStream_t st) {
  using namespace rt;
  const uint64_t n = 1ull << k;
  if (d_out != d_g) HIPCHK(hipMemcpyAsync(d_out, d_g, n * sizeof(G1Affine), hipMemcpyDeviceToDevice, st));
  if (k == 0) {  // L_0 = g_0
    HIPCHK(hipStreamSynchronize(st));
    return H2G_OK;
  }
  Pool tmp;  // released on every return below
  const uint64_t ntw = n / 2;
  Fr* tw = nullptr;
  if (tmp.get((void**)&tw, ntw * sizeof(Fr)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(st);
    return fail(H2G_ERR_NOMEM, "g1_to_lagrange: no device memory for " + std::to_string(ntw * sizeof(Fr)) +
                                   " bytes of twiddles");
  }
  Fr omega = root_of_unity();
  for (uint32_t i = k; i < FR_S; i++) omega = sqr(omega);
  const Fr omega_inv = inv(omega);
  PowTable om;
  RCCHK(build_pow_table(tmp, omega_inv, (int)k - 1, &om, st));
  hipLaunchKernelGGL(g1fft_twiddle_kernel, dim3(blocks_for(ntw, 256)), dim3(256), 0, st, om, ntw, tw);
  hipLaunchKernelGGL(g1fft_bitrev_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, d_out, k);
  const dim3 grid(blocks_for(n / 2, G1FFT_WAVE)), block(G1FFT_WAVE);
  for (uint32_t s = 1; s <= k; s++) {
    if (g1fft_stage_uniform(k, s))
      hipLaunchKernelGGL(g1fft_stage_kernel<true>, grid, block, 0, st, d_out, (const Fr*)tw, k, s);
    else
      hipLaunchKernelGGL(g1fft_stage_kernel<false>, grid, block, 0, st, d_out, (const Fr*)tw, k, s);
  }
  const Fr ninv = to_canonical(inv(from_u64<FrParams>(n)));
  hipLaunchKernelGGL(g1fft_scale_kernel, dim3(blocks_for(n, G1FFT_WAVE)), block, 0, st, d_out, k, ninv);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return H2G_OK;
}
}  // namespace h2g

using namespace h2g;
using namespace h2g::rt;

extern "C" {

int h2g_g1_to_lagrange_dev(const void* d_g, uint32_t k, void* d_out, void* stream) {
  NEED_DEV_P();
  if (!d_g || !d_out || k > G1FFT_MAX_K) return fail(H2G_ERR_ARG, "g1_to_lagrange_dev: null pointer or k > 27");
  return g1_to_lagrange((const G1Affine*)d_g, k, (G1Affine*)d_out, pick_stream(d, stream));
}

int h2g_g1_to_lagrange(const uint64_t* g, uint32_t k, uint64_t* out) {
  NEED_DEV_P();
  if (!g || !out || k > G1FFT_MAX_K) return fail(H2G_ERR_ARG, "g1_to_lagrange: null pointer or k > 27");
  const size_t bytes = ((size_t)1 << k) * sizeof(G1Affine);
  prv::Pool tmp;
  G1Affine* p = nullptr;
  if (tmp.get((void**)&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(H2G_ERR_NOMEM, "g1_to_lagrange: no device memory for the points");
  }
  HIPCHK(hipMemcpyAsync(p, g, bytes, hipMemcpyHostToDevice, d->stream));
  RCCHK(g1_to_lagrange(p, k, p, d->stream));
  HIPCHK(hipMemcpy(out, p, bytes, hipMemcpyDeviceToHost));
  return H2G_OK;
}

}  // extern "C"
