// g1_fft.h -- the G1 group FFT behind g_to_lagrange (halo2_backend/src/arithmetic.rs:30-54):
//   L_i = [n^-1] sum_j [omega^(-ij)] g_j,   n = 2^k, natural order in and out.
//
// Shape: radix-2 decimation in time, in place on n affine points.
//   1. the points are permuted by bit reversal (pair swaps; the permutation is an involution);
//   2. stage s = 1 .. k joins blocks of m = 2^s points: butterfly (lo, hi = lo + m/2) becomes
//      (lo + [w] hi, lo - [w] hi) with w = omega^-(j n/m), j = lo mod m/2.  One thread per
//      butterfly, one launch per stage.  Butterfly t of the n/2 of a stage is
//          j = t >> (k - s),  block = t mod 2^(k-s),  lo = block m + j,
//      so butterflies that share a twiddle are consecutive in t: wherever a twiddle serves at
//      least G1FFT_WAVE butterflies (s <= k - 6) a whole 64-lane wave has ONE scalar, which it
//      reads through the wave's first t (scalar loads, scalar branches on the scalar's bits,
//      no divergence in the conditional addition).  The last stages (s > k - 6) read one
//      twiddle per lane.  The mapping is the same in both forms; only the t whose twiddle is
//      read differs (g1fft_stage_uniform).
//      [w] hi is the MSB-first double-and-add chain from the scalar's top set bit
//      (msm_seg.hip's), so the twiddle 1 -- all of stage 1, butterfly group j = 0 of every
//      stage -- costs no group operation;
//   3. every point is multiplied by n^-1 (one scalar for the whole launch).
// Between stages the points are AFFINE (64 B): a chain step is xyzz_dbl + the mixed
// xyzz_madd (9 + 10 products) instead of the general xyzz_add (14), and the two results of a
// butterfly share one field inversion (~15 K uniform operations against the chain's ~10^6).
// Every addition goes through the complete case analysis of xyzz_madd (either operand the
// identity, P + P, P + (-P)) on fully reduced coordinates, and the stored points are affine,
// hence unique: the output is exact for every input.
//
// Everything a kernel indexes with, and the butterfly itself, is H2G_HD here, so that
// tests/native/g1_fft_host.cpp runs the same transform on the host, stage by stage, in the
// kernels' order and mapping.  All indices are 64-bit (k <= 27).
//
// Scratch of one call (a Pool local to the call, released before it returns):
//   twiddles omega^-x, x < n/2, canonical:  16 * 2^k bytes  (32 B at k = 0, 1)
//   the two-level power table they come from: 32 * (2^ceil((k-1)/2) + 2^floor((k-1)/2)) bytes
// and no point storage: the transform runs in d_out.
#pragma once
#include "bn254.h"

namespace h2g {

constexpr uint32_t G1FFT_WAVE = 64;  // threads per block of a stage launch = one wave
constexpr uint32_t G1FFT_MAX_K = 27;

// the low k bits of i, reversed
H2G_HD uint64_t g1fft_bitrev(uint64_t i, uint32_t k) {
  uint64_t r = 0;
  for (uint32_t b = 0; b < k; b++) r |= ((i >> b) & 1ull) << (k - 1 - b);
  return r;
}

// stage s of k (1 <= s <= k): does every wave of G1FFT_WAVE consecutive butterflies share
// one twiddle?
H2G_HD bool g1fft_stage_uniform(uint32_t k, uint32_t s) { return k - s >= 6; }
// butterfly t (< n/2) of stage s: index of its twiddle in the table of omega^-x, x < n/2
H2G_HD uint64_t g1fft_twiddle_index(uint64_t t, uint32_t k, uint32_t s) { return (t >> (k - s)) << (k - s); }
// ... and of its first point; the partner is g1fft_half(s) above it
H2G_HD uint64_t g1fft_lo_index(uint64_t t, uint32_t k, uint32_t s) {
  const uint64_t block = t & ((1ull << (k - s)) - 1);
  return (block << s) + (t >> (k - s));
}
H2G_HD uint64_t g1fft_half(uint32_t s) { return 1ull << (s - 1); }

// [s] b for a canonical scalar s: MSB-first double-and-add from the top set bit.  The scalar
// is shifted left through bit 255 one bit per step, so its limbs are only ever indexed by
// constants: they stay in registers (scalar ones where s is wave-uniform), not in memory.
H2G_HD void g1fft_shl1(uint32_t l[8]) {
#pragma unroll
  for (int i = 7; i > 0; i--) l[i] = (l[i] << 1) | (l[i - 1] >> 31);
  l[0] <<= 1;
}
H2G_HD G1xyzz g1fft_mul(const G1Affine& b, const Fr& s) {
  if (b.is_identity() || s.is_zero()) return G1xyzz::identity();
  uint32_t l[8];
#pragma unroll
  for (int i = 0; i < 8; i++) l[i] = s.l[i];
  int bits = 256;  // bits of s from its top set bit down
  while (!(l[7] >> 31)) {
    g1fft_shl1(l);
    bits--;
  }
  G1xyzz acc = G1xyzz::from_affine(b);  // the top set bit
  for (int i = 1; i < bits; i++) {
    g1fft_shl1(l);
    acc = xyzz_dbl(acc);
    if (l[7] >> 31) acc = xyzz_madd(acc, b);
  }
  return acc;
}

// the wave-uniform divsteps inversion on the device, the binary GCD on the host: the same value
H2G_HD Fq g1fft_inv(const Fq& a) {
#ifdef __HIP_DEVICE_COMPILE__
  return inv_by(a);
#else
  return inv(a);
#endif
}

H2G_HD G1Affine g1fft_to_affine(const G1xyzz& p) {
  G1Affine r;
  if (p.is_identity()) {
    r.x = Fq::zero();
    r.y = Fq::zero();
    return r;
  }
  const Fq i = g1fft_inv(p.ZZ * p.ZZZ);
  r.x = p.X * (i * p.ZZZ);
  r.y = p.Y * (i * p.ZZ);
  return r;
}

// two points with one inversion (Montgomery's trick; an identity contributes the factor 1)
H2G_HD void g1fft_pair_to_affine(const G1xyzz& p, const G1xyzz& q, G1Affine* pa, G1Affine* qa) {
  const bool pi = p.is_identity(), qi = q.is_identity();
  const Fq dp = pi ? Fq::one() : p.ZZ * p.ZZZ;
  const Fq dq = qi ? Fq::one() : q.ZZ * q.ZZZ;
  const Fq i = g1fft_inv(dp * dq);
  const Fq ip = i * dq, iq = i * dp;  // 1 / (ZZ ZZZ) of p, of q
  pa->x = pi ? Fq::zero() : p.X * (ip * p.ZZZ);
  pa->y = pi ? Fq::zero() : p.Y * (ip * p.ZZ);
  qa->x = qi ? Fq::zero() : q.X * (iq * q.ZZZ);
  qa->y = qi ? Fq::zero() : q.Y * (iq * q.ZZ);
}

// (a, b) <- (a + [w] b, a - [w] b)
H2G_HD void g1fft_butterfly(G1Affine* pa, G1Affine* pb, const Fr& w) {
  const G1xyzz t = g1fft_mul(*pb, w);
  const G1Affine a = *pa;
  const G1xyzz sum = xyzz_madd(t, a);
  const G1xyzz dif = xyzz_madd(xyzz_neg(t), a);
  g1fft_pair_to_affine(sum, dif, pa, pb);
}

// butterfly t of stage s on p[0 .. 2^k), with the twiddle of butterfly t_tw: t itself, or the
// first butterfly of t's wave where g1fft_stage_uniform(k, s) says they are equal
H2G_HD void g1fft_stage_one(G1Affine* p, const Fr* tw, uint32_t k, uint32_t s, uint64_t t_tw, uint64_t t) {
  const Fr w = tw[g1fft_twiddle_index(t_tw, k, s)];
  const uint64_t lo = g1fft_lo_index(t, k, s);
  g1fft_butterfly(p + lo, p + lo + g1fft_half(s), w);
}

// the final scaling: [n^-1] p, n^-1 canonical
H2G_HD G1Affine g1fft_scale(const G1Affine& p, const Fr& ninv) { return g1fft_to_affine(g1fft_mul(p, ninv)); }

// g_to_lagrange on device points; d_out may equal d_g.  Runs on `st` and returns after the
// work has completed (the scratch is released before returning).  An H2G_* code.
int g1_to_lagrange(const G1Affine* d_g, uint32_t k, G1Affine* d_out, hipStream_t st);

}  // namespace h2g
