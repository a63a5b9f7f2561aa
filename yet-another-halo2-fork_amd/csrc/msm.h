// msm.h -- Pippenger MSM over BN254 G1 (see msm.hip).
#pragma once
#include "bn254.h"

namespace h2g {

struct MsmConfig {
  int c = 0;         // window bits (0: choose from n)
  int item_len = 0;  // entries per accumulation chunk (0: choose)
};

// One device buffer of the workspace: grown on demand, never shrunk (MSMs of slightly
// different shapes -- n and n - 1 points, so another chunk length -- reuse it instead of
// reallocating, ~2 ms of host stall each).
struct MsmBuf {
  void* p = nullptr;
  size_t cap = 0;  // bytes
};

// The byte size of each workspace buffer for one MSM shape (msm_plan); the names are
// MsmWorkspace's.
struct MsmBytes {
  uint64_t ent, vals, items, bnd, buckets, red, windows, counters, multi, item_sums;
};

// Device workspace, reused across calls.  nbt = bucket sets x buckets per set, total = the
// entry bound n W nbatch, chunks = msm_chunk_cap (msm_part.h); G1xyzz29 is 144 B.
struct MsmWorkspace {
  int last_c = 0, last_W = 0;  // window bits and bucket sets of the most recent pipeline
  // u64 [total] coarse-binned entries (key << 32 | value).  Reused: dead once the partition
  // has run, it then holds the accumulation's whole buckets, G1xyzz29 [nbt] (raw F29
  // accumulators), until the fixup converts them into `buckets`.
  MsmBuf ent;
  MsmBuf vals;     // u32 [total] values (table index | sign << 31) in bucket order
  MsmBuf items;    // MsmBigItem [msm_big_items_cap(chunks)] big-bucket work items
  MsmBuf bnd;      // G1xyzz29 [2 chunks] the accumulation's boundary slots (raw)
  MsmBuf buckets;  // G1xyzz29 [nbt] the bucket sums (back-end class)
  // Reused: the reduction's intermediate points, G1xyzz29, one of two layouts.  Bit planes:
  // planes [(plane_lb + 2) x sets x nblk_p], then mid [(plane_lb + K + 2 <= 20) x sets] in
  // the rest (>= 32 per set).  rscale scheme: S, R [sets x m1] each, then the block sums P
  // [sets x nblk].
  MsmBuf red;
  MsmBuf windows;    // G1xyzz [max(W, sets)] the bucket sets' sums, read by the final / the host
  MsmBuf counters;   // u32: [0] big-bucket items, [1] multi-item buckets, [4] repairs, [5 ..] the repair list
  MsmBuf multi;      // uint4 [msm_big_multi_cap(chunks)] multi-item buckets (bucket, first item, items)
  MsmBuf item_sums;  // G1xyzz29 [msm_big_items_cap(chunks)] the items' partial sums
  // u32 partition counts / offsets and per-key offsets (msm_part.h MsmScratch), laid out for
  // kcap keys; zeroed when allocated, and every MSM leaves its counts zero
  MsmBuf scratch;
  size_t kcap = 0;
};

// Everything the pipeline decides from an MSM's shape, before it allocates or launches
// (msm_plan; host only -- test seam h2g_debug_msm_plan, tests/test_msm_plan_cpu.py).
// 32- and 64-bit fields only, no padding: include/h2g.h's h2g_msm_plan mirrors it.
struct MsmPlan {
  uint64_t total;    // entry bound n W nbatch (< 2^31: u32 positions in the sorted array)
  uint64_t nb_eff;   // buckets most windows can reach (the chunk rule's quarter-bucket floor)
  uint64_t nchunks;  // the most chunks the accumulation can make (msm_chunk_cap)
  MsmBytes bytes;
  uint64_t scratch_words;  // u32 words of the scratch laid out for kcap = nbt
  uint32_t c, W;           // window bits, windows
  uint32_t fixed, nbatch;
  uint32_t WB, NB, nbt;    // bucket sets, buckets per set 2^(c - 1), their product
  uint32_t L, adapt;       // the host's chunk length; 1: the device may shorten it (MsmChunkRule)
  uint32_t fb, ncoarse, kblocks;  // partition: fine bits, coarse bins, 1024-key scan blocks
  uint32_t staged;                // the fine pass's LDS-staged form
  uint32_t fixup_q;               // lanes per bucket of the fixup: 4 (quad) or 1
  uint32_t red_plane;             // reduction: 1 bit planes, 0 rscale scheme
  uint32_t plane_q, plane_lb, rgp, e0, m1p, nblk_p;  // planes: lanes per group, log2 groups per block,
                                                     // buckets per group and its log2, groups and blocks
                                                     // per set (0 under rscale)
  uint32_t m1, nblk;  // rscale: groups of RG buckets and blocks of 256 groups per set (0 under planes)
  uint32_t reserved;
};
// false: a shape the pipeline refuses (batch range, total >= 2^31, more than COARSE_MAX
// coarse bins, more than 256 bucket sets); *out is then untouched
bool msm_plan(size_t n, int c, int W, int fixed, int nbatch, uint32_t item_len, MsmPlan* out);

int msm_choose_c(size_t n);
int msm_windows_for(int c);

// Optional per-phase HIP events (profiling).  Phases: digits, sort, bucket_bounds,
// accumulate, bucket_fixup, reduce -> 7 events, recorded on the MSM's stream.
static constexpr int MSM_NPHASES = 6;
struct MsmPhaseEvents {
  hipEvent_t ev[MSM_NPHASES + 1];
  int msms = 1;  // MSMs the timed pipeline served (a batch counts each)
  uint32_t* entries = nullptr;  // pinned: receives the sorted-entry (nonzero digit) count
};

// Scalar vectors of a batch of MSMs (kernel argument by value).
static constexpr int MSM_MAX_BATCH = 64;
struct MsmScalarList {
  const Fr* p[MSM_MAX_BATCH];
};

// sum_i scalars[i] * bases[i]; scalars Montgomery Fr, bases affine Montgomery Fq
// (halo2curves layout).  Asynchronous on `st`.  If d_out != nullptr the affine
// result is written there by one device lane; otherwise the W window sums are
// left in ws->windows.p (G1xyzz[ws->last_W]) for msm_windows_host_finish.
hipError_t msm_run(const Fr* d_scalars, const G1Affine* d_bases, size_t n, MsmWorkspace* ws,
                   const MsmConfig& cfg, G1Affine* d_out, hipStream_t st, MsmPhaseEvents* prof = nullptr);
G1Affine msm_windows_host_finish(const G1xyzz* h_windows, int W, int c);
void msm_free(MsmWorkspace* ws);

// Fixed-base mode for resident bases (SRS, base descriptors): windows are
// pre-multiplied, table[w * n + i] = [2^(c w)] bases[i], so all W windows share one
// set of 2^(c-1) buckets (one reduction instead of W; larger c affordable).
// W * n * 64 B of HBM per table (e.g. 3.5 GB for n = 2^22, c = 20).
struct MsmFixedBase {
  G1Affine* table = nullptr;
  size_t n = 0;
  int c = 0, W = 0;
};
int msm_choose_c_fixed(size_t n);
hipError_t msm_fixed_base_build(const G1Affine* d_bases, size_t n, int c, MsmFixedBase* fb, hipStream_t st);
void msm_fixed_base_free(MsmFixedBase* fb);
// inclusive prefix sums of n affine points: out[i] = in[0] + ... + in[i] (setup; scratch
// allocated and freed inside)
hipError_t msm_prefix_points(const G1Affine* in, size_t n, G1Affine* out, hipStream_t st);
// sum_{i < n} scalars[i] * bases[off + i]; leaves ws->windows.p[0] (ws->last_W = 1)
hipError_t msm_run_fixed(const Fr* d_scalars, const MsmFixedBase& fb, size_t off, size_t n, MsmWorkspace* ws,
                         G1Affine* d_out, hipStream_t st, MsmPhaseEvents* prof = nullptr);
// nbatch MSMs sum_i list.p[b][i] * bases[off + i] (b < nbatch <= MSM_MAX_BATCH) as one
// pipeline -- one digits launch, one sort, one accumulation, one reduction with a bucket
// set per MSM -- so the latency-bound reduction is paid once.  Leaves MSM b's sum in
// ws->windows.p[b] (ws->last_W = nbatch).  nbatch * W * n must stay below 2^31.
hipError_t msm_run_fixed_batch(const MsmScalarList& list, int nbatch, const MsmFixedBase& fb, size_t off, size_t n,
                               MsmWorkspace* ws, hipStream_t st, MsmPhaseEvents* prof = nullptr);

}  // namespace h2g
