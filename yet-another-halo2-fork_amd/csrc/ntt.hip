// ntt.hip -- register-resident radix-2^m NTT over BN254 Fr for gfx950.
//
// Computes exactly what halo2curves' best_fft computes (natural order in,
// natural order out, y_k = sum_i a_i w^(ik)), as called by
// EvaluationDomain (halo2_backend/src/poly/domain.rs:220, 238, 275, 344),
// plus the fused pre/post maps of coeff_to_extended / extended_to_coeff /
// lagrange_to_coeff (domain.rs:216-293).
//
// Decomposition: N = N_0 * N_1 * ... * N_{P-1}, every N_p = 2^m_p with
// 3 <= m_p <= 6 and the last pass 2^6.  With i = i_low + (L_p/N_p) i_p, pass p
// runs the size-N_p DFT over i_p, then multiplies by w^{(N/L_p) i_low k_p}, in
// place; the last pass reads contiguous runs and writes natural order (digit
// reversal folded into its store).  Each pass touches HBM once (64 B/element).
//
// One wavefront owns CPW = 64 / 2^(m-3) adjacent columns; every lane holds 8
// elements of one column in registers.  A 2^m-point DIF = one in-register
// radix-8 round on the top 3 index bits, (m-3) lane<->register bit swaps by
// v_permlane32_swap / v_permlane16_swap / a DPP row rotation (no LDS, no barriers), and a
// second in-register round on the low m-3 bits.  Global accesses are runs of >= 8 x 32 B
// across the lanes of one instruction.  Inter-pass twiddles are streamed from per-pass tables
// (NttTables::pass_tw), built once from a 2-level table w^E = lo[E mod 2^b] * hi[E >> b].
#include <algorithm>
#include <type_traits>

#include "ntt.h"
#include "f29.h"

namespace h2g {

static constexpr int NTT_WAVES = 4;  // waves per block (independent; no block barriers after the table)
static constexpr int NTT_THREADS = 64 * NTT_WAVES;
#ifndef NTT_MIN_WAVES
#define NTT_MIN_WAVES 2  // waves per SIMD the register allocation must admit
#endif
// 2^6 passes fit 168 VGPRs without spilling -> 3 waves per SIMD (512 / 168);
// the smaller passes would spill at 168 and stay at 2.
template <int M>
struct NttPassWaves {
  static constexpr int value = M == 6 ? 3 : NTT_MIN_WAVES;
};

__device__ __forceinline__ Fr ld_fr(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  Fr r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
__device__ __forceinline__ void st_fr(Fr* p, const Fr& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

__device__ __forceinline__ Fr twiddle(const NttTables& t, uint64_t e) {
  return t.lo[e & ((1ull << t.b) - 1)] * t.hi[e >> t.b];
}

// y mod 3 for 64-bit y with 32-bit arithmetic (2^32 = 1 mod 3)
__device__ __forceinline__ uint32_t mod3(uint64_t y) {
  return ((uint32_t)(y >> 32) % 3u + (uint32_t)y % 3u) % 3u;
}

__device__ __forceinline__ uint32_t brev_bits(uint32_t x, int m) { return __brev(x) >> (32 - m); }

// ---------------------------------------------------------------------------
// The passes run in 9 x 29-bit limbs (f29.h).  The transform is linear, so the
// stored integers move in and out by repacking only (f29.h: raw29 / pack29) and the
// constants -- twiddles, coset powers, scales -- are F29 elements (the pass tables are
// built in that form, storage_to_f29_packed).  Products are f29.h's carry-free REDC.
// Value bounds (tools/f29_bounds.py, "ntt"): stored values < 3 M; stage s of a pass
// subtracts with K_s = 2^(s+2) M (>= the stage's input bound with a top-limb margin), so
// after 6 stages every value is < 254 M < 2^262 and the closing product (pass twiddle or
// epilogue constant, < M) brings it back below 2.6 M; the last pass reduces to [0, M).

__device__ __forceinline__ F29 ld29(const Fr* p) { return raw29(ld_fr(p)); }
__device__ __forceinline__ void st29(Fr* p, const F29& v) { st_fr(p, pack29<FrParams>(v)); }
__device__ __forceinline__ F29 sel29(int c, const F29& a, const F29& b) {
  F29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}
// compile-time loop: f(std::integral_constant<int, I>) for I in [I0, N) -- for loops over
// whole products, which `#pragma unroll` may leave rolled (x[] is then indexed at run time
// and moves to scratch)
template <int I, int N, class F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    sfor<I + 1, N>(f);
  }
}

// The passes' products are the single-chain block forms of f29.h: two independent products
// as one pair block (mul29_pair, their chains alternate), a lone one as the single block.

// a - b + K_s M for stage s: K_s = 2^(s+2)
template <int S>
__device__ __forceinline__ F29 nsub29(const F29& a, const F29& b) {
  return sub29<FrParams, (4u << S), 29>(a, b);
}

// In-register DIF of 2^M-point columns.  Lane = c + CPW * rg; register q of the
// lane initially holds row r = rg + LPC * q.  `w[j] = w_{2^M}^j`, j < 2^(M-1).
// After run(), register q holds DIF position rpos(q, rg) (output index
// k = bitrev_M(rpos)).  The stages are templates: unrolled loops over whole products were
// left rolled by the compiler, and a rolled stage loop indexes x[] at run time (x[] then
// lives in scratch).
template <int M>
struct WaveDif29 {
  static constexpr int LPC = 1 << (M - 3);  // lanes per column
  static constexpr int CPW = 64 / LPC;      // columns per wave
  // register index of butterfly p < 4 of a stage on register bit T (its partner: + 2^T)
  static constexpr int qof(int p, int T) { return ((p >> T) << (T + 1)) | (p & ((1 << T) - 1)); }
  template <int T>  // round A, row bit M-3+T (stage 2 - T)
  __device__ static __forceinline__ void stage_a(F29 x[8], const F29* w, int rg) {
    constexpr int htlog = (M - 3) + T;
    F29 d[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int q = qof(p, T);
      const F29 a = x[q], b = x[q + (1 << T)];
      x[q] = norm29(add29(a, b));
      d[p] = nsub29<2 - T>(a, b);
    }
    // the four products are independent: two pair blocks
    sfor<0, 2>([&](auto hc) {
      constexpr int p0 = 2 * decltype(hc)::value, p1 = p0 + 1;
      const int j0 = rg + (p0 & ((1 << T) - 1)) * LPC, j1 = rg + (p1 & ((1 << T) - 1)) * LPC;
      mul29_pair<FrParams>(x[qof(p0, T) + (1 << T)], x[qof(p1, T) + (1 << T)], d[p0], w[j0 << (M - 1 - htlog)], d[p1],
                   w[j1 << (M - 1 - htlog)]);
    });
    if constexpr (T > 0) stage_a<T - 1>(x, w, rg);
  }
  // register bit B <-> lane bit: the lower lane's high register changes places with the
  // upper lane's low register.  Lane distances 32 and 16 are exactly v_permlane32_swap /
  // v_permlane16_swap (vdst = the low register: its upper lanes or odd rows swap with the
  // lower lanes or even rows of src); distance 8 (M = 6 only) is a select, a DPP rotation
  // of the row by 8 and a select.  No LDS traffic.
  template <int B>
  __device__ static __forceinline__ void swap_bits(F29 x[8], int rg) {
    if constexpr (B < M - 3) {
      constexpr int dist = CPW << B;
      const int lb = (rg >> B) & 1;
#pragma unroll
      for (int p = 0; p < 4; p++) {
        const int q = qof(p, B);
        if constexpr (dist >= 16) {
#pragma unroll
          for (int i = 0; i < 9; i++) {
            const auto r = dist == 32 ? __builtin_amdgcn_permlane32_swap(x[q].l[i], x[q | (1 << B)].l[i], false, false)
                                      : __builtin_amdgcn_permlane16_swap(x[q].l[i], x[q | (1 << B)].l[i], false, false);
            x[q].l[i] = r[0];
            x[q | (1 << B)].l[i] = r[1];
          }
        } else {
          static_assert(dist == 8, "lane distance of a register/lane bit swap");
          const F29 lo_v = x[q], hi_v = x[q | (1 << B)];
          const F29 send = sel29(lb, lo_v, hi_v);
          F29 recv;
#pragma unroll
          for (int i = 0; i < 9; i++)
            recv.l[i] =
                (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send.l[i], 0x128 /* row_ror:8 */, 0xf, 0xf, false);
          x[q] = sel29(lb, recv, lo_v);
          x[q | (1 << B)] = sel29(lb, hi_v, recv);
        }
      }
      swap_bits<B + 1>(x, rg);
    }
  }
  template <int T>  // round B, row bit T (stage 3 + M - 4 - T)
  __device__ static __forceinline__ void stage_b(F29 x[8], const F29* w) {
    if constexpr (T >= 0) {
      constexpr int S = 3 + (M - 4 - T);
      F29 d[4];
#pragma unroll
      for (int p = 0; p < 4; p++) {
        const int q = qof(p, T);
        const F29 a = x[q], b = x[q + (1 << T)];
        x[q] = norm29(add29(a, b));
        d[p] = nsub29<S>(a, b);
      }
      // butterfly p takes twiddle j = p mod 2^T, none for j = 0: T = 0 has no product,
      // T = 1 has p = 1, 3 (a pair), T = 2 has p = 1, 2 (a pair) and p = 3
      constexpr int hi = 1 << T;
      x[qof(0, T) + hi] = norm29(d[0]);
      if constexpr (T == 0) {
        x[qof(1, T) + hi] = norm29(d[1]);
        x[qof(2, T) + hi] = norm29(d[2]);
        x[qof(3, T) + hi] = norm29(d[3]);
      } else if constexpr (T == 1) {
        x[qof(2, T) + hi] = norm29(d[2]);
        const F29 w1 = w[1 << (M - 1 - T)];
        mul29_pair<FrParams>(x[qof(1, T) + hi], x[qof(3, T) + hi], d[1], w1, d[3], w1);
      } else {
        static_assert(T == 2, "round B has at most three stages");
        mul29_pair<FrParams>(x[qof(1, T) + hi], x[qof(2, T) + hi], d[1], w[1 << (M - 1 - T)], d[2],
                             w[2 << (M - 1 - T)]);
        x[qof(3, T) + hi] = mul29_acc<FrParams>(d[3], w[3 << (M - 1 - T)]);
      }
      stage_b<T - 1>(x, w);
    }
  }
  __device__ static __forceinline__ void run(F29 x[8], const F29* w, int rg) {
    stage_a<2>(x, w, rg);
    if constexpr (M > 3) {
      // A lane swap must not read a register within two wait states of its write, and the
      // compiler counts them only for its own instructions.  A product block's last write is
      // its top limb (the closing move), so the top limbs of round A's last products pass
      // through two states here, once; every other limb is written earlier in its block
      // (tests/test_ntt_inst_count_cpu.py checks the emitted code for it).
      asm("s_nop 1" : "+v"(x[1].l[8]), "+v"(x[3].l[8]), "+v"(x[5].l[8]), "+v"(x[7].l[8]));
      swap_bits<0>(x, rg);
    }
    stage_b<M - 4>(x, w);
  }

  // DIF position held by register q of lane rg after run()
  __device__ static __forceinline__ uint32_t rpos(int q, int rg) {
    constexpr int LB = M - 3;
    const uint32_t lowmask = (1u << LB) - 1;
    const uint32_t lo = (uint32_t)q & lowmask;                              // row bits < LB
    const uint32_t mid = (uint32_t)rg & lowmask;                            // row bits LB..2LB-1
    const uint32_t hi = ((uint32_t)q >> LB) << LB;                          // untouched register bits
    return lo + ((mid | hi) << LB);
  }
};

// the constants of one launch in F29 form (host-converted)
struct NttConst29 {
  F29 z1, z2;      // input coset powers (pass 0)
  F29 mul[3];      // epilogue multiplier per y mod 3 (last pass), one29 when none
};

// The geometric input twist of a first pass (NttArgs::in_twist): x_j = src[j] gamma^j with
// gamma = zeta g (zeta^3 = 1, so zeta^(j mod 3) = zeta^j).  A lane's eight inputs sit
// 2^(L-3) apart, so it forms gamma^j for its first one -- g^j from the caller's two-level
// power table (root^(mul j)), times the zeta power -- and walks to the others with one
// product by `step` = gamma^(2^(L-3)) each.  No table of n factors per g.
struct NttTwist29 {
  const Fr* lo;    // root^i, i < 2^bits
  const Fr* hi;    // root^(i 2^bits)
  int bits;
  uint64_t mul;    // g = root^mul
  uint64_t mask;   // the root's order - 1
  F29 step;
};

// (Inter-pass twiddles formed in the pass from the two-level table -- one product and two
// L2-resident loads per element -- instead of streamed from pass_tw, 32 B of HBM per
// element: measured, rejected.)
// TWIST is a compile-time variant (the first pass, out of place: first = 1, lrem = L): the
// plain instantiations hold nothing of it, their `twist` is an empty struct.
struct NttNoTwist {};
template <bool TWIST>
using NttTwistArg29 = std::conditional_t<TWIST, NttTwist29, NttNoTwist>;
template <int M, bool TWIST = false>
__global__ void __launch_bounds__(NTT_THREADS, NttPassWaves<M>::value)
ntt_pass29_kernel(Fr* data, NttIo io, int first, uint64_t n_in, NttTables tab, const Fr* __restrict__ ptw, int L,
                  int lrem, int distribute, NttConst29 k29, NttTwistArg29<TWIST> twist) {
  using D = WaveDif29<M>;
  data += (uint64_t)blockIdx.y << L;
  const Fr* in = first ? io.src[blockIdx.y] : nullptr;
  __shared__ F29 w[1 << (M - 1)];
  for (int j = threadIdx.x; j < (1 << (M - 1)); j += blockDim.x) w[j] = ld29(tab.root64 + (j << (6 - M)));
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * NTT_WAVES + (threadIdx.x >> 6);
  if (wave >= (1ull << L) / ((1ull << M) * D::CPW)) return;
  const uint64_t S = 1ull << (lrem - M);
  const uint64_t groups = S / D::CPW;
  const uint64_t q = wave / groups;
  const uint64_t g = wave % groups;
  const uint64_t base = (q << lrem) + g * D::CPW;
  const int c = lane % D::CPW, rg = lane / D::CPW;
  F29 x[8];
  if constexpr (TWIST) {
    // f = gamma^pos of register 0: to29 of the storage-form power is its F29 element (an
    // integer < 32 M, a valid factor); every later f is a product, < 1.2 M, and so is
    // every input (stored values < 3 M hold).  The loads go first, the chain under them.
    const uint64_t p0 = base + c + (uint64_t)rg * S;
    const uint64_t e = (twist.mul * p0) & twist.mask;
    const uint32_t md = mod3(p0);
    F29 f = mul29<FrParams>(to29(twist.lo[e & ((1ull << twist.bits) - 1)] * twist.hi[e >> twist.bits]),
                            sel29(md == 1, k29.z1, sel29(md == 2, k29.z2, one29v<FrParams>())));
    sfor<0, 8>([&](auto qc) {
      constexpr int qq = decltype(qc)::value;
      const uint64_t pos = p0 + (uint64_t)(D::LPC * qq) * S;
      F29 v;
#pragma unroll
      for (int i = 0; i < 9; i++) v.l[i] = 0;
      if (pos < n_in) v = mul29<FrParams>(ld29(in + pos), f);
      x[qq] = v;
      if constexpr (qq < 7) f = mul29<FrParams>(f, twist.step);
    });
  } else {
    sfor<0, 8>([&](auto qc) {
      constexpr int qq = decltype(qc)::value;
      const uint64_t pos = base + c + (uint64_t)(rg + D::LPC * qq) * S;
      if (in) {
        F29 v;
#pragma unroll
        for (int i = 0; i < 9; i++) v.l[i] = 0;
        if (pos < n_in) {
          v = ld29(in + pos);
          if (distribute) {
            const uint32_t md = mod3(pos);
            if (md) v = mul29<FrParams>(v, sel29(md == 1, k29.z1, k29.z2));
          }
        }
        x[qq] = v;
      } else {
        x[qq] = ld29(data + pos);
      }
    });
  }
  D::run(x, w, rg);
  const uint64_t ilow = g * D::CPW + c;
  sfor<0, 4>([&](auto qc) {
    constexpr int q0 = 2 * decltype(qc)::value, q1 = q0 + 1;
    const uint32_t k0 = brev_bits(D::rpos(q0, rg), M), k1 = brev_bits(D::rpos(q1, rg), M);
    F29 y0, y1;
    mul29_pair<FrParams>(y0, y1, x[q0], ld29(ptw + (uint64_t)k0 * S + ilow), x[q1],
                         ld29(ptw + (uint64_t)k1 * S + ilow));
    st29(data + base + c + (uint64_t)k0 * S, y0);
    st29(data + base + c + (uint64_t)k1 * S, y1);
  });
}

// Persistent variant of ntt_pass29_kernel for the passes after the first: a wave walks
// column groups item, item + stride, ... and loads the next group's elements before it
// transforms the current one, so a SIMD's VALU work is not held up by its waves' loads all
// arriving at once (one launch round of the plain kernel loads, then computes, then stores).
template <int M>
__global__ void __launch_bounds__(NTT_THREADS, 2)
ntt_pass29p_kernel(Fr* data, NttTables tab, const Fr* __restrict__ ptw, int L, int lrem, uint64_t items) {
  using D = WaveDif29<M>;
  data += (uint64_t)blockIdx.y << L;
  __shared__ F29 w[1 << (M - 1)];
  for (int j = threadIdx.x; j < (1 << (M - 1)); j += blockDim.x) w[j] = ld29(tab.root64 + (j << (6 - M)));
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * NTT_WAVES;
  uint64_t item = (uint64_t)blockIdx.x * NTT_WAVES + (threadIdx.x >> 6);
  if (item >= items) return;
  const uint64_t S = 1ull << (lrem - M);
  const uint64_t groups = S / D::CPW;
  const int c = lane % D::CPW, rg = lane / D::CPW;
  Fr nx[8];
  auto fetch = [&](uint64_t it) {
    const uint64_t b = ((it / groups) << lrem) + (it % groups) * D::CPW;
    sfor<0, 8>([&](auto qc) {
      constexpr int qq = decltype(qc)::value;
      const uint64_t pos = b + c + (uint64_t)(rg + D::LPC * qq) * S;
      nx[qq] = ld_fr(data + pos);
    });
  };
  fetch(item);
  for (;;) {
    const uint64_t cur = item;
    const uint64_t base = ((cur / groups) << lrem) + (cur % groups) * D::CPW;
    F29 x[8];
    sfor<0, 8>([&](auto qc) {
      constexpr int qq = decltype(qc)::value;
      x[qq] = raw29(nx[qq]);
    });
    item += stride;
    const bool more = item < items;
    if (more) fetch(item);
    __builtin_amdgcn_sched_barrier(0);  // the prefetch issues before the transform, the twiddle loads after it
    D::run(x, w, rg);
    __builtin_amdgcn_sched_barrier(0);
    const uint64_t ilow = (cur % groups) * D::CPW + c;
    sfor<0, 4>([&](auto qc) {
      constexpr int q0 = 2 * decltype(qc)::value, q1 = q0 + 1;
      const uint32_t k0 = brev_bits(D::rpos(q0, rg), M), k1 = brev_bits(D::rpos(q1, rg), M);
      F29 y0, y1;
      mul29_pair<FrParams>(y0, y1, x[q0], ld29(ptw + (uint64_t)k0 * S + ilow), x[q1],
                         ld29(ptw + (uint64_t)k1 * S + ilow));
      st29(data + base + c + (uint64_t)k0 * S, y0);
      st29(data + base + c + (uint64_t)k1 * S, y1);
    });
    if (!more) break;
  }
}

// First pass of 2^3 points when at most the first two of every column's eight inputs are
// nonzero (n_in <= N / 4: a coset extension by 4 or more, coeff_to_extended of a degree-5
// circuit): y_k = x_0 + w_8^k x_1 (w_8^(k+4) = -w_8^k), two loads and three products per
// column instead of eight loads and the twelve products of the 8-point DIF.  One lane per
// column; outputs < 1.04 M.
__global__ void __launch_bounds__(NTT_THREADS)
ntt_first_sparse29_kernel(Fr* data, NttIo io, uint64_t n_in, NttTables tab, const Fr* __restrict__ ptw, int L,
                          int distribute, NttConst29 k29) {
  data += (uint64_t)blockIdx.y << L;
  const Fr* in = io.src[blockIdx.y];
  const uint64_t S = 1ull << (L - 3);
  const uint64_t col = (uint64_t)blockIdx.x * NTT_THREADS + threadIdx.x;
  if (col >= S) return;
  F29 x[2];
  sfor<0, 2>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const uint64_t pos = col + (uint64_t)j * S;
    F29 v;
#pragma unroll
    for (int i = 0; i < 9; i++) v.l[i] = 0;
    if (pos < n_in) {
      v = ld29(in + pos);
      if (distribute) {
        const uint32_t md = mod3(pos);
        if (md) v = mul29<FrParams>(v, sel29(md == 1, k29.z1, k29.z2));
      }
    }
    x[j] = v;
  });
  F29 y[8];
  sfor<0, 4>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const F29 pj = j == 0 ? x[1] : mul29<FrParams>(x[1], ld29(tab.root64 + 8 * j));
    y[j] = norm29(add29(x[0], pj));
    y[j + 4] = sub29<FrParams, 4, 29>(x[0], pj);
  });
  sfor<0, 8>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    st29(data + col + (uint64_t)k * S, mul29<FrParams>(y[k], ld29(ptw + (uint64_t)k * S + col)));
  });
}

int ntt_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                   hipSuccess || cus <= 0)
      cus = 256;
  }
  return cus;
}

#ifndef NTT_LAST_WAVES  // waves per SIMD of the untruncated last pass (142 VGPRs: 3 without spilling)
#define NTT_LAST_WAVES 3
#endif
// TRUNC: out_len < N (extended_to_coeff's truncation) -- the stores are predicated per
// element; without it every element is stored and the epilogue has no branches
// ONE: the epilogue constant is one for every y (no scale left, no output distribution) --
// the values (< 256 M) are brought to [0, M) by reduce29 and one conditional subtraction
// instead of a product
template <bool TRUNC, bool ONE>
__global__ void __launch_bounds__(NTT_THREADS, TRUNC ? NTT_MIN_WAVES : NTT_LAST_WAVES)
ntt_last29_kernel(const Fr* data, NttIo io, uint64_t out_len, NttTables tab, int L, NttPlanLg plan,
                  NttConst29 k29) {
  constexpr int M = 6;
  data += (uint64_t)blockIdx.y << L;
  Fr* out = io.dst[blockIdx.y];
  using D = WaveDif29<M>;
  __shared__ F29 w[1 << (M - 1)];
  for (int j = threadIdx.x; j < (1 << (M - 1)); j += blockDim.x) w[j] = ld29(tab.root64 + (j << (6 - M)));
  __syncthreads();
  const int* lgs = plan.lg;
  const int P = plan.p;
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * NTT_WAVES + (threadIdx.x >> 6);
  if (wave >= (1ull << L) / ((1ull << M) * D::CPW)) return;
  const int l0 = lgs[0];
  const uint64_t groups = (1ull << l0) / D::CPW;
  const uint64_t midx = wave / groups;
  const uint64_t g = wave % groups;
  uint64_t mid_nat = 0;
  {
    uint64_t rem = midx;
    int wbits_tail = L - M;
#pragma unroll
    for (int p = NTT_MAX_PASSES - 2; p >= 1; p--) {
      if (p > P - 2) continue;
      const int lgp = lgs[p];
      const uint64_t dig = rem & ((1ull << lgp) - 1);
      rem >>= lgp;
      wbits_tail -= lgp;
      mid_nat |= dig << wbits_tail;
    }
  }
  const int c = lane % D::CPW, rg = lane / D::CPW;
  const uint64_t k0 = g * D::CPW + c;
  const uint64_t colbase = k0 * (1ull << (L - l0)) + (midx << M);
  F29 x[8];
  sfor<0, 8>([&](auto qc) {
    constexpr int qq = decltype(qc)::value;
    x[qq] = ld29(data + colbase + rg + D::LPC * qq);
  });
  D::run(x, w, rg);
  const uint64_t kstride = 1ull << (L - M);
  auto yof = [&](int qq) { return k0 + mid_nat + (uint64_t)brev_bits(D::rpos(qq, rg), M) * kstride; };
  if constexpr (ONE) {
    sfor<0, 8>([&](auto qc) {
      constexpr int qq = decltype(qc)::value;
      const uint64_t y = yof(qq);
      if (!TRUNC || y < out_len) st29(out + y, sub_m_if_ge29<FrParams>(reduce29<FrParams>(x[qq])));
    });
  } else {
    // the epilogue constant (scale and / or zeta power) also brings the value below 2.6 M;
    // two conditional subtractions reach [0, M).  The products go in pairs; where only one
    // element of a pair is stored, the other's product is discarded.
    auto kof = [&](uint64_t y) {
      const uint32_t md = mod3(y);
      return sel29(md == 1, k29.mul[1], sel29(md == 2, k29.mul[2], k29.mul[0]));
    };
    sfor<0, 4>([&](auto qc) {
      // registers q and q + 4 hold outputs N / 8 apart (q's bits are y's top three), so a pair
      // lies on one side of a truncation at a multiple of N / 4 and at most an eighth of the
      // outputs sits in pairs that straddle another one
      constexpr int q0 = decltype(qc)::value, q1 = q0 + 4;
      const uint64_t y0 = yof(q0), y1 = yof(q1);
      if (!TRUNC || y0 < out_len || y1 < out_len) {  // a pair wholly behind the truncation: no product
        F29 v0, v1;
        mul29_pair<FrParams>(v0, v1, x[q0], kof(y0), x[q1], kof(y1));
        if (!TRUNC || y0 < out_len) st29(out + y0, sub_m_if_ge29<FrParams>(sub_m_if_ge29<FrParams>(v0)));
        if (!TRUNC || y1 < out_len) st29(out + y1, sub_m_if_ge29<FrParams>(sub_m_if_ge29<FrParams>(v1)));
      }
    });
  }
}

// ---------------------------------------------------------------------------
// Whole transform in one block (N <= 2^NTT_SMALL_MAX_LOG), radix-2 DIF in LDS.
// The geometric input twist here (NttArgs::in_twist, cf. NttTwist29): thread i walks
// i, i + 256, ... with one product by step = gamma^256 each.
struct NttTwistFr {
  const Fr* lo;
  const Fr* hi;
  int bits;
  uint64_t mul, mask;
  Fr step;
};
template <bool TWIST>
using NttTwistArgFr = std::conditional_t<TWIST, NttTwistFr, NttNoTwist>;
template <bool TWIST>
__global__ void __launch_bounds__(256)
ntt_small_kernel(NttIo io, uint64_t n_in, uint64_t out_len, NttTables tab, int L,
                 int in_distribute, Fr iz1, Fr iz2, int has_scale, Fr scale, int out_distribute,
                 Fr oz1, Fr oz2, NttTwistArgFr<TWIST> tw) {
  const Fr* src = io.src[blockIdx.x];
  Fr* out = io.dst[blockIdx.x];
  extern __shared__ __align__(16) unsigned char smem_raw[];
  Fr* s = reinterpret_cast<Fr*>(smem_raw);
  const int N = 1 << L;
  Fr* w = s + N;
  for (int j = threadIdx.x; j < N / 2; j += blockDim.x) w[j] = twiddle(tab, (uint64_t)j);
  if constexpr (TWIST) {
    if ((int)threadIdx.x < N) {
      const uint64_t e = (tw.mul * threadIdx.x) & tw.mask;
      Fr f = tw.lo[e & ((1ull << tw.bits) - 1)] * tw.hi[e >> tw.bits];
      const int md = threadIdx.x % 3;
      if (md == 1) f = f * iz1;
      else if (md == 2) f = f * iz2;
      for (int i = threadIdx.x; i < N; i += blockDim.x) {
        s[i] = (uint64_t)i < n_in ? ld_fr(src + i) * f : Fr::zero();
        f = f * tw.step;
      }
    }
  } else {
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
      Fr v = Fr::zero();
      if ((uint64_t)i < n_in) {
        v = ld_fr(src + i);
        if (in_distribute) {
          const int md = i % 3;
          if (md == 1) v = v * iz1;
          else if (md == 2) v = v * iz2;
        }
      }
      s[i] = v;
    }
  }
  __syncthreads();
  for (int hlog = L - 1; hlog >= 0; hlog--) {
    const int h = 1 << hlog;
    for (int t = threadIdx.x; t < N / 2; t += blockDim.x) {
      const int j = t & (h - 1);
      const int i = ((t >> hlog) << (hlog + 1)) + j;
      const Fr a = s[i], b = s[i + h];
      s[i] = a + b;
      s[i + h] = (a - b) * w[j << (L - 1 - hlog)];
    }
    __syncthreads();
  }
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    if ((uint64_t)k >= out_len) continue;
    Fr v = s[L > 0 ? brev_bits((uint32_t)k, L) : 0];
    if (has_scale) v = v * scale;
    if (out_distribute) {
      const int md = k % 3;
      if (md == 1) v = v * oz1;
      else if (md == 2) v = v * oz2;
    }
    st_fr(out + k, v);
  }
}

// ---------------------------------------------------------------------------
// Twiddle tables: lo[j] = w^j (j < 2^b), hi[j] = w^(j 2^b) (j < 2^(L-b)).
__global__ void ntt_tables_kernel(Fr* lo, Fr* hi, Fr w, int b, int L) {
  const uint64_t nlo = 1ull << b, nhi = 1ull << (L - b);
  const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (t < nlo) lo[t] = pow_u64(w, t);
  if (t < nhi) {
    Fr wb = w;
    for (int i = 0; i < b; i++) wb = sqr(wb);
    hi[t] = pow_u64(wb, t);
  }
}

// w_64^j = w^(j 2^(L - 6)), j < 32, as packed F29 elements (the F29 passes' LDS twiddles)
__global__ void ntt_root64_kernel(Fr* out, NttTables tab, int L) {
  const int j = threadIdx.x;
  if (j < 32) out[j] = storage_to_f29_packed<FrParams>(twiddle(tab, (uint64_t)j << (L - 6)));
}

// pass table: t = k * S + i_low over [0, 2^lrem): w^(i_low k 2^(L - lrem)), packed F29
__global__ void ntt_pass_tw_kernel(Fr* out, NttTables tab, int L, int lrem, int M, int fold) {
  const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (t >= (1ull << lrem)) return;
  const uint64_t S = 1ull << (lrem - M);
  const uint64_t k = t / S, ilow = t % S;
  Fr v = twiddle(tab, (ilow * k) << (L - lrem));
  if (fold) v = v * tab.fold;  // the first pass carries the transform's scale
  out[t] = storage_to_f29_packed<FrParams>(v);  // the passes' form
}

// ---------------------------------------------------------------------------
// Host side

void ntt_split(int L, int* P, int lg[NTT_MAX_PASSES]) {
  if (L <= NTT_SMALL_MAX_LOG) {
    *P = 1;
    lg[0] = L;
    return;
  }
  int p = (L + 5) / 6;
  const int R = L - 6 * (p - 1);
  int i = 0;
  // the short pass goes first (second, or two 5-bit passes for a 4-bit one: measured, rejected)
  if (R >= 3) {
    lg[i++] = R;
  } else {  // borrow 3 bits so every pass has 3..6 bits
    lg[i++] = 3;
    lg[i++] = R + 3;
  }
  while (i < p) lg[i++] = 6;
  *P = p;
}

hipError_t ntt_build_tables(NttTables* t, const Fr& omega, int L, hipStream_t st, const Fr& fold) {
  t->L = L;
  t->fold = fold;
  t->fold_inv = inv(fold);
  t->b = (L + 1) / 2;
  if (t->b < 1) t->b = 1;
  const uint64_t nlo = 1ull << t->b, nhi = 1ull << (L > t->b ? L - t->b : 0);
  hipError_t e = hipMalloc(&t->lo, nlo * sizeof(Fr));
  if (e != hipSuccess) return e;
  e = hipMalloc(&t->hi, (nhi > 0 ? nhi : 1) * sizeof(Fr));
  if (e != hipSuccess) return e;
  const uint64_t mx = nlo > nhi ? nlo : nhi;
  const int bs = 256;
  hipLaunchKernelGGL(ntt_tables_kernel, dim3((unsigned)((mx + bs - 1) / bs)), dim3(bs), 0, st, t->lo, t->hi,
                     omega, t->b, L < t->b ? t->b : L);
  e = hipGetLastError();
  if (e != hipSuccess || L <= NTT_SMALL_MAX_LOG) return e;
  int P, lg[NTT_MAX_PASSES];
  ntt_split(L, &P, lg);
  uint64_t total = 0;
  int lrem = L;
  for (int p = 0; p < P - 1; p++) {
    t->pass_off[p] = total;
    total += 1ull << lrem;
    lrem -= lg[p];
  }
  e = hipMalloc(&t->pass_tw, (total ? total : 1) * sizeof(Fr));
  if (e != hipSuccess) return e;
  e = hipMalloc(&t->root64, 32 * sizeof(Fr));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ntt_root64_kernel, dim3(1), dim3(32), 0, st, t->root64, *t, L);
  lrem = L;
  for (int p = 0; p < P - 1; p++) {
    const uint64_t cnt = 1ull << lrem;
    hipLaunchKernelGGL(ntt_pass_tw_kernel, dim3((unsigned)((cnt + bs - 1) / bs)), dim3(bs), 0, st,
                       t->pass_tw + t->pass_off[p], *t, L, lrem, lg[p], p == 0 ? 1 : 0);
    lrem -= lg[p];
  }
  return hipGetLastError();
}

void ntt_free_tables(NttTables* t) {
  if (t->lo) (void)hipFree(t->lo);
  if (t->hi) (void)hipFree(t->hi);
  if (t->pass_tw) (void)hipFree(t->pass_tw);
  if (t->root64) (void)hipFree(t->root64);
  t->lo = t->hi = t->pass_tw = t->root64 = nullptr;
}

hipError_t ntt_init_attributes() {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ntt_small_kernel<false>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&ntt_small_kernel<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

// ntt_run's decisions (ntt.h NttPlan).  Every pass has N / 512 wave items per transform: a
// wave owns CPW = 64 / 2^(M-3) columns of 2^M points.
static_assert(8 * WaveDif29<3>::CPW == 512 && 16 * WaveDif29<4>::CPW == 512 && 32 * WaveDif29<5>::CPW == 512 &&
                  64 * WaveDif29<6>::CPW == 512,
              "a wave item is 512 elements");

bool ntt_plan(int L, uint64_t n_in, uint64_t out_len, int count, int in_twist, int cus, bool epilogue_one,
              NttPlan* out) {
  NttPlan pl;
  if (L < 0 || L > 28 || !out) return false;
  const uint64_t N = 1ull << L;
  const int B = count < 1 ? 1 : count;
  if (B > NTT_MAX_BATCH) return false;
  pl.batch = B;
  ntt_split(L, &pl.lg.p, pl.lg.lg);
  const int P = pl.lg.p;
  const int* lg = pl.lg.lg;
  if (P == 1) {
    pl.first = NTT_FIRST_ONE_BLOCK;
    pl.first_grid = (unsigned)B;
    *out = pl;
    return true;
  }
  if (P > NTT_MAX_PASSES || lg[P - 1] != 6) return false;
  for (int p = 0; p < P; p++)
    if (lg[p] < 3 || lg[p] > 6) return false;
  pl.items = N / 512;
  pl.blocks = (unsigned)((pl.items + NTT_WAVES - 1) / NTT_WAVES);
  if (in_twist) {
    pl.first = NTT_FIRST_TWISTED;
    pl.first_grid = pl.blocks;
  } else if (lg[0] == 3 && n_in <= (N >> 2)) {
    pl.first = NTT_FIRST_SPARSE;
    pl.first_grid = (unsigned)(((N >> 3) + NTT_THREADS - 1) / NTT_THREADS);
  } else {
    pl.first = NTT_FIRST_PLAIN;
    pl.first_grid = pl.blocks;
  }
  // the passes after the first: two 4-wave blocks per CU over the whole batch, every wave several groups
  const uint64_t want = (uint64_t)(cus > 0 ? cus : 0) * 2 / (uint64_t)B;
  const unsigned pb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(pl.blocks, want));
  for (int p = 1; p < P - 1; p++) pl.pgrid[p] = pb;
  pl.trunc = (out_len ? out_len : N) < N;
  pl.one = epilogue_one;
  *out = pl;
  return true;
}

// the twisted first pass: never the sparse kernel (n_in = N), never a later pass
template <int M>
static void launch_pass_tw(const NttArgs& a, const NttIo& io, const NttPlan& pl, int L, const NttConst29& k29,
                           const NttTwist29& tw, hipStream_t st) {
  hipLaunchKernelGGL((ntt_pass29_kernel<M, true>), dim3(pl.first_grid, (unsigned)pl.batch), dim3(NTT_THREADS), 0, st,
                     a.work, io, 1, a.n_in, a.tab, (const Fr*)(a.tab.pass_tw + a.tab.pass_off[0]), L, L, 1, k29, tw);
}

template <int M>
static void launch_pass(const NttArgs& a, const NttIo& io, const NttPlan& pl, int p, int L, int lrem,
                        const NttConst29& k29, hipStream_t st) {
  const int first = p == 0;
  const uint64_t n_in = first ? a.n_in : 0;
  const int dist = first ? a.in_distribute : 0;
  const unsigned B = (unsigned)pl.batch;
  if (first && pl.first == NTT_FIRST_SPARSE) {
    hipLaunchKernelGGL(ntt_first_sparse29_kernel, dim3(pl.first_grid, B), dim3(NTT_THREADS), 0, st, a.work, io, n_in,
                       a.tab, (const Fr*)(a.tab.pass_tw + a.tab.pass_off[p]), L, dist, k29);
    return;
  }
  if (!first) {
    hipLaunchKernelGGL(ntt_pass29p_kernel<M>, dim3(pl.pgrid[p], B), dim3(NTT_THREADS), 0, st, a.work, a.tab,
                       (const Fr*)(a.tab.pass_tw + a.tab.pass_off[p]), L, lrem, pl.items);
    return;
  }
  hipLaunchKernelGGL((ntt_pass29_kernel<M, false>), dim3(pl.first_grid, B), dim3(NTT_THREADS), 0, st, a.work, io,
                     first, n_in, a.tab, (const Fr*)(a.tab.pass_tw + a.tab.pass_off[p]), L, lrem, dist, k29,
                     NttNoTwist{});
}

hipError_t ntt_run(const NttArgs& a, hipStream_t st) {
  const int L = a.tab.L;
  const uint64_t N = 1ull << L;
  const uint64_t out_len = a.out_len ? a.out_len : N;
  // epilogue multiplier per (y mod 3): scale * zeta-power / the scale folded into the
  // first pass's table, on the host
  Fr mul[3];
  bool one = true;
  for (int r = 0; r < 3; r++) {
    Fr m = (a.has_scale ? a.scale : Fr::one()) * a.tab.fold_inv;
    if (a.out_distribute && r == 1) m = m * a.out_z1;
    if (a.out_distribute && r == 2) m = m * a.out_z2;
    mul[r] = m;
    one = one && m == Fr::one();
  }
  NttPlan pl;
  if (!ntt_plan(L, a.n_in, a.out_len, a.count, a.in_twist, ntt_cus(), one, &pl)) return hipErrorInvalidValue;
  const int B = pl.batch;
  NttIo io = {};
  for (int b = 0; b < B; b++) {
    io.src[b] = B == 1 ? a.src : a.srcs[b];
    io.dst[b] = B == 1 ? a.dst : a.dsts[b];
  }
  const NttPlanLg& plan = pl.lg;
  const int P = plan.p;
  const int* lg = plan.lg;
  if (a.in_twist && (!a.tw_lo || !a.tw_hi || a.n_in > N)) return hipErrorInvalidValue;
  // gamma = zeta g, the twist's ratio (in_z1 = zeta)
  const Fr gamma = a.in_twist ? a.tw_g * a.in_z1 : Fr::one();
  if (pl.first == NTT_FIRST_ONE_BLOCK && a.in_twist) {
    const size_t sm = (N + N / 2 + 1) * sizeof(Fr);
    NttTwistFr tw = {a.tw_lo, a.tw_hi, a.tw_bits, a.tw_mul, a.tw_mask, pow_u64(gamma, 256)};
    hipLaunchKernelGGL(ntt_small_kernel<true>, dim3(pl.first_grid), dim3(256), sm, st, io, a.n_in, out_len, a.tab, L,
                       1, a.in_z1, a.in_z2, a.has_scale, a.scale, a.out_distribute, a.out_z1, a.out_z2, tw);
    return hipGetLastError();
  }
  if (pl.first == NTT_FIRST_ONE_BLOCK) {
    const size_t sm = (N + N / 2 + 1) * sizeof(Fr);
    hipLaunchKernelGGL(ntt_small_kernel<false>, dim3(pl.first_grid), dim3(256), sm, st, io, a.n_in, out_len, a.tab, L,
                       a.in_distribute, a.in_z1, a.in_z2, a.has_scale, a.scale, a.out_distribute, a.out_z1,
                       a.out_z2, NttNoTwist{});
    return hipGetLastError();
  }
  if (!a.tab.pass_tw) return hipErrorInvalidValue;
  NttConst29 k29;  // the F29 passes' constants
  k29.z1 = storage_to_f29<FrParams>(a.in_z1);
  k29.z2 = storage_to_f29<FrParams>(a.in_z2);
  for (int r = 0; r < 3; r++) k29.mul[r] = storage_to_f29<FrParams>(mul[r]);
  // N / N_0 and every middle S are multiples of 64 >= CPW: waves divide evenly.
  // pass 0: src -> work (out of place), passes 1..P-2 in place on work,
  // last pass: work -> dst in natural order.
  int lrem = L;
  for (int p = 0; p < P - 1; p++) {
    if (p == 0 && pl.first == NTT_FIRST_TWISTED) {
      NttTwist29 tw = {a.tw_lo, a.tw_hi, a.tw_bits, a.tw_mul, a.tw_mask,
                       storage_to_f29<FrParams>(pow_u64(gamma, 1ull << (L - 3)))};
      switch (lg[0]) {
        case 3: launch_pass_tw<3>(a, io, pl, L, k29, tw, st); break;
        case 4: launch_pass_tw<4>(a, io, pl, L, k29, tw, st); break;
        case 5: launch_pass_tw<5>(a, io, pl, L, k29, tw, st); break;
        case 6: launch_pass_tw<6>(a, io, pl, L, k29, tw, st); break;
        default: return hipErrorInvalidValue;
      }
      lrem -= lg[0];
      continue;
    }
    switch (lg[p]) {
      case 3: launch_pass<3>(a, io, pl, p, L, lrem, k29, st); break;
      case 4: launch_pass<4>(a, io, pl, p, L, lrem, k29, st); break;
      case 5: launch_pass<5>(a, io, pl, p, L, lrem, k29, st); break;
      case 6: launch_pass<6>(a, io, pl, p, L, lrem, k29, st); break;
      default: return hipErrorInvalidValue;
    }
    lrem -= lg[p];
  }
  {
    const dim3 g(pl.blocks, (unsigned)B), b(NTT_THREADS);
    if (pl.trunc && pl.one)
      hipLaunchKernelGGL((ntt_last29_kernel<true, true>), g, b, 0, st, (const Fr*)a.work, io, out_len, a.tab, L, plan,
                         k29);
    else if (pl.trunc)
      hipLaunchKernelGGL((ntt_last29_kernel<true, false>), g, b, 0, st, (const Fr*)a.work, io, out_len, a.tab, L,
                         plan, k29);
    else if (pl.one)
      hipLaunchKernelGGL((ntt_last29_kernel<false, true>), g, b, 0, st, (const Fr*)a.work, io, out_len, a.tab, L,
                         plan, k29);
    else
      hipLaunchKernelGGL((ntt_last29_kernel<false, false>), g, b, 0, st, (const Fr*)a.work, io, out_len, a.tab, L,
                         plan, k29);
  }
  return hipGetLastError();
}

}  // namespace h2g
