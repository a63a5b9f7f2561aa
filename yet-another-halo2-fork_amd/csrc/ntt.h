// ntt.h -- NTT plan/launch interface (see ntt.hip).
#pragma once
#include "bn254.h"

namespace h2g {

static constexpr int NTT_SMALL_MAX_LOG = 10;  // whole transform in one block up to 2^10
static constexpr int NTT_MAX_PASSES = 6;      // passes of 3..6 bits: N up to 2^28
static constexpr int NTT_MAX_BATCH = 8;       // transforms per batched launch (blockIdx.y)

// per-transform source / destination of a batched launch
struct NttIo {
  const Fr* src[NTT_MAX_BATCH];
  Fr* dst[NTT_MAX_BATCH];
};

struct NttPlanLg {
  int p = 0;
  int lg[NTT_MAX_PASSES] = {0, 0, 0, 0, 0, 0};
};

struct NttTables {
  int L = 0;  // log2 N
  int b = 0;  // split of the 2-level table
  Fr* lo = nullptr;
  Fr* hi = nullptr;
  // precomputed inter-pass twiddles of the non-last passes: pass p's table holds
  // w^((N/L_p) i_low k) at [k * S_p + i_low] (L_p entries; sum over passes ~ 1.1 N)
  Fr* pass_tw = nullptr;
  uint64_t pass_off[NTT_MAX_PASSES] = {0, 0, 0, 0, 0, 0};
  // the F29 passes' in-pass twiddles w_64^j, j < 32, as F29 elements packed in 8 x 32 bits
  // (a 2^m-point pass reads every 2^(6-m)-th); L >= 6
  Fr* root64 = nullptr;
  // Unused (two table pointers of a rejected pass variant lived here).  NttTables is a
  // by-value kernel argument: without these 16 bytes the argument offsets in 16 of the
  // NTT kernels move.  Drop them with the next change to those kernels.
  Fr* reserved[2] = {nullptr, nullptr};
  // the constant multiplied into the first pass's table (pass_tw; a transform's scale, so
  // its last pass needs no product) and its inverse (divided out of a call's epilogue)
  Fr fold = Fr::one();
  Fr fold_inv = Fr::one();
};

// One transform y = DFT_w(x) of size N = 2^tab.L with fused maps:
//   x_i = src[i] * (in_distribute ? zeta-power(i mod 3) : 1) for i < n_in, 0 beyond
//   dst[k] = y_k * (has_scale ? scale : 1) * (out_distribute ? zeta-power(k mod 3) : 1), k < out_len
// `work` is an N-element scratch buffer distinct from src and dst (src may alias dst).
// Batched: `count` > 1 independent transforms with the same maps, src / dst from
// `srcs` / `dsts`, `work` of count * N elements; one launch per pass serves them all
// (more waves in flight for the small transforms of many-column circuits).
struct NttArgs {
  const Fr* src = nullptr;
  uint64_t n_in = 0;
  Fr* work = nullptr;
  Fr* dst = nullptr;
  int count = 1;
  const Fr* srcs[NTT_MAX_BATCH] = {};
  Fr* dsts[NTT_MAX_BATCH] = {};
  uint64_t out_len = 0;
  NttTables tab;
  int in_distribute = 0;
  Fr in_z1, in_z2;
  int has_scale = 0;
  Fr scale;
  int out_distribute = 0;
  Fr out_z1, out_z2;
  // geometric input twist, fused into the first pass: x_i = src[i] * zeta^(i mod 3) * g^i
  // (in_z1 = zeta, in_z2 = zeta^2; in_distribute is implied).  g = tw_g = root^tw_mul for
  // the root whose powers the two-level table holds: root^i = tw_lo[i & (2^tw_bits - 1)] *
  // tw_hi[i >> tw_bits], i <= tw_mask (the root's order - 1).  The kernels form the factors
  // themselves -- one table power per thread, then a running product -- so no table of N
  // factors exists per g.
  int in_twist = 0;
  Fr tw_g;
  const Fr* tw_lo = nullptr;
  const Fr* tw_hi = nullptr;
  int tw_bits = 0;
  uint64_t tw_mul = 0, tw_mask = 0;
};

// Every choice ntt_run makes for one call, as a pure host function of the call's shape (test
// seam: h2g_debug_ntt_plan, tests/test_ntt_plan_cpu.py).  ntt_run launches from this and
// decides nothing itself, so a test that asks for a shape's plan knows which kernels ran.
enum NttFirst {
  NTT_FIRST_ONE_BLOCK = 0,  // ntt_small_kernel: the whole transform, P == 1 (twisted or not)
  NTT_FIRST_SPARSE = 1,     // ntt_first_sparse29_kernel: lg[0] == 3 and n_in <= N / 4
  NTT_FIRST_PLAIN = 2,      // ntt_pass29_kernel<M, false>
  NTT_FIRST_TWISTED = 3,    // ntt_pass29_kernel<M, true> (in_twist; never the sparse kernel)
};
struct NttPlan {
  NttPlanLg lg;          // P and the bits of every pass
  int batch = 1;         // transforms per launch (grid.y; grid.x of the one-block kernel)
  int first = NTT_FIRST_ONE_BLOCK;
  uint64_t items = 0;    // wave items of a pass per transform: N / 512 whatever the pass's bits
  unsigned blocks = 0;   // grid.x of the plain / twisted first pass and of the last pass
  unsigned first_grid = 0;  // grid.x of the first pass: `batch`, N / 8 / 256 (sparse) or `blocks`
  // grid.x of the persistent middle pass p, 0 < p < P - 1: min(blocks, 2 cus / batch), >= 1;
  // 0 elsewhere.  A wave walks item, item + 4 grid, ...: ragged when grid does not divide blocks.
  unsigned pgrid[NTT_MAX_PASSES] = {0, 0, 0, 0, 0, 0};
  bool trunc = false;    // last pass: out_len < N, predicated stores
  bool one = false;      // last pass: no epilogue product
};
// out_len 0 = N; count < 1 = 1; epilogue_one: the per-(y mod 3) epilogue constants are all
// one.  false: a shape ntt_run refuses (count > NTT_MAX_BATCH, L outside 0..28).
bool ntt_plan(int L, uint64_t n_in, uint64_t out_len, int count, int in_twist, int cus, bool epilogue_one,
              NttPlan* out);
int ntt_cus();  // the CU count ntt_run plans with: the current device's, 256 when it has none

void ntt_split(int L, int* P, int lg[NTT_MAX_PASSES]);
hipError_t ntt_build_tables(NttTables* t, const Fr& omega, int L, hipStream_t st, const Fr& fold = Fr::one());
void ntt_free_tables(NttTables* t);
hipError_t ntt_run(const NttArgs& a, hipStream_t st);
hipError_t ntt_init_attributes();

}  // namespace h2g
