// msm_seg.hip -- segmented small MSM: nseg independent sums of a few to a few thousand
// terms each, one launch, one affine result per segment (h2g_msm_segmented*).
//
// The Pippenger path (msm.hip) spends a partition, a bucket set and a reduction on ONE sum
// of 2^19..2^24 points.  A batch verifier has the opposite shape: two ~10^2-term sums per
// proof over bases that many proofs share (the verifying key's commitments), so the input is
// CSR over one base array and one workgroup serves one segment:
//   - lane t takes terms t, t + SEG_T, ... of its segment: scalar out of Montgomery form,
//     MSB-first double-and-add from the scalar's top set bit (xyzz_dbl + xyzz_madd on the
//     affine base), partial sums added per lane;
//   - the SEG_T partial sums are added by a tree in LDS (SEG_T x 128 B = 16 KiB);
//   - lane 0 converts to affine (one inversion) and stores 64 B.
// Every addition goes through the complete case analysis of xyzz_madd / xyzz_add (either
// operand the identity, P + P -> doubling, P + (-P) -> identity), on fully reduced
// coordinates, so the result is exact for every input: zero scalars, identity bases, a base
// listed twice, a base with its negation.  8 x 32-bit limbs (bn254.h): a call's floor is the
// 254 dependent doublings of one lane (~4 ms), not issue; the compiler reports 161 VGPRs, no
// spills and 3 waves per SIMD.  Two 64-lane waves per group keep a ~100-term segment at one
// term per lane.  Measured: 1024 segments x 128 terms in 9.4 ms.
#include "msm_seg.h"

#include "runtime.h"

namespace h2g {
namespace {
constexpr int SEG_T = 128;

__global__ void __launch_bounds__(SEG_T) msm_segmented_kernel(const G1Affine* __restrict__ bases, uint32_t nbases,
                                                              const Fr* __restrict__ scalars,
                                                              const uint32_t* __restrict__ index,
                                                              const uint32_t* __restrict__ seg_off,
                                                              G1Affine* __restrict__ out) {
  __shared__ G1xyzz sh[SEG_T];
  const uint32_t seg = blockIdx.x, tid = threadIdx.x;
  const uint32_t lo = seg_off[seg], hi = seg_off[seg + 1];
  G1xyzz sum = G1xyzz::identity();
  for (uint64_t j = (uint64_t)lo + tid; j < hi; j += SEG_T) {
    const uint32_t bi = index ? index[j] : (uint32_t)j;
    if (bi >= nbases) continue;
    const G1Affine b = bases[bi];
    const Fr s = to_canonical(scalars[j]);
    if (b.is_identity() || s.is_zero()) continue;
    int top = 7;
    while (s.l[top] == 0) top--;
    int bit = 31 - __clz(s.l[top]);
    G1xyzz acc = G1xyzz::from_affine(b);  // the top set bit
    for (int i = top; i >= 0; i--) {
      const uint32_t w = s.l[i];
      for (int k = (i == top ? bit - 1 : 31); k >= 0; k--) {
        acc = xyzz_dbl(acc);
        if ((w >> k) & 1u) acc = xyzz_madd(acc, b);
      }
    }
    sum = xyzz_add(sum, acc);
  }
  sh[tid] = sum;
  __syncthreads();
  for (uint32_t s = SEG_T / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = xyzz_add(sh[tid], sh[tid + s]);
    __syncthreads();
  }
  if (tid == 0) out[seg] = xyzz_to_affine(sh[0]);
}
}  // namespace

hipError_t msm_segmented(const G1Affine* bases, size_t nbases, const Fr* scalars, const uint32_t* index,
                         const uint32_t* seg_off, size_t nseg, G1Affine* out, hipStream_t st) {
  if (nseg == 0) return hipSuccess;
  hipLaunchKernelGGL(msm_segmented_kernel, dim3((unsigned)nseg), dim3(SEG_T), 0, st, bases, (uint32_t)nbases, scalars,
                     index, seg_off, out);
  return hipGetLastError();
}
}  // namespace h2g

using namespace h2g;
using namespace h2g::rt;

#define NEED_DEV_SEG()                                                \
  std::lock_guard<std::recursive_mutex> _lk(g_mu);                    \
  Device* d = cur();                                                  \
  if (!d) return fail(H2G_ERR_STATE, "h2g_init has not been called"); \
  HIPCHK(hipSetDevice(d->id));

extern "C" {

int h2g_msm_segmented_dev(const void* d_bases, size_t nbases, const void* d_scalars, const uint32_t* d_index,
                          const uint32_t* d_seg_off, size_t nseg, void* d_out_affine, void* stream) {
  NEED_DEV_SEG();
  if (nseg == 0) return H2G_OK;
  if (!d_seg_off || !d_out_affine) return fail(H2G_ERR_ARG, "msm_segmented_dev: null pointer");
  if (nbases >= (1ull << 32) || nseg >= (1ull << 31)) return fail(H2G_ERR_ARG, "msm_segmented_dev: too many bases or segments");
  HIPCHK(msm_segmented((const G1Affine*)d_bases, nbases, (const Fr*)d_scalars, d_index, d_seg_off, nseg,
                       (G1Affine*)d_out_affine, pick_stream(d, stream)));
  return H2G_OK;
}

int h2g_msm_segmented(const uint64_t* bases, size_t nbases, const uint64_t* scalars, const uint32_t* index,
                      const uint32_t* seg_off, size_t nseg, uint64_t* out_affine) {
  NEED_DEV_SEG();
  if (nseg == 0) return H2G_OK;
  if (!seg_off || !out_affine) return fail(H2G_ERR_ARG, "msm_segmented: null pointer");
  if (nbases >= (1ull << 32) || nseg >= (1ull << 31)) return fail(H2G_ERR_ARG, "msm_segmented: too many bases or segments");
  for (size_t s = 0; s < nseg; s++)
    if (seg_off[s] > seg_off[s + 1]) return fail(H2G_ERR_ARG, "msm_segmented: segment offsets must not decrease");
  const size_t first = seg_off[0], nnz = seg_off[nseg];
  if (nnz && (!scalars || !bases)) return fail(H2G_ERR_ARG, "msm_segmented: null input");
  if (index) {
    for (size_t j = first; j < nnz; j++)
      if (index[j] >= nbases) return fail(H2G_ERR_ARG, "msm_segmented: base index out of range");
  } else if (nnz > nbases) {
    return fail(H2G_ERR_ARG, "msm_segmented: more terms than bases");
  }
  hipStream_t st = d->stream;
  // one allocation: bases | scalars | out | index | offsets (64-B aligned parts)
  auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
  const size_t o_sc = up(nbases * 64), o_out = o_sc + up(nnz * 32), o_ix = o_out + up(nseg * 64),
               o_off = o_ix + up(nnz * 4), total = o_off + up((nseg + 1) * 4);
  HIPCHK(d->work.ensure(total + 64));
  uint8_t* w = d->work.as<uint8_t>();
  if (nbases) HIPCHK(hipMemcpyAsync(w, bases, nbases * 64, hipMemcpyHostToDevice, st));
  if (nnz) HIPCHK(hipMemcpyAsync(w + o_sc, scalars, nnz * 32, hipMemcpyHostToDevice, st));
  if (index && nnz) HIPCHK(hipMemcpyAsync(w + o_ix, index, nnz * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(w + o_off, seg_off, (nseg + 1) * 4, hipMemcpyHostToDevice, st));
  HIPCHK(msm_segmented((const G1Affine*)w, nbases, (const Fr*)(w + o_sc), index ? (const uint32_t*)(w + o_ix) : nullptr,
                       (const uint32_t*)(w + o_off), nseg, (G1Affine*)(w + o_out), st));
  HIPCHK(hipMemcpyAsync(out_affine, w + o_out, nseg * 64, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return H2G_OK;
}

}  // extern "C"
