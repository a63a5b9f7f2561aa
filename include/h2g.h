/*
 * h2g.h -- C ABI of the MI355X-native halo2 prover hot path (libh2g.so).
 *
 * This is the drop-in boundary a halo2 (yetanotherco/yet-another-halo2-fork)
 * host binds over FFI.  Plain pointers and sizes only; no torch or HIP types.
 *
 * Data layout (identical to halo2curves 0.6 in memory, so Rust slices are passed
 * by pointer with no conversion):
 *   Fr  : 4 x uint64_t little-endian limbs, Montgomery form (R = 2^256), < r
 *   G1Affine : x[4], y[4] Fq limbs, Montgomery form; identity = (0, 0)
 * Host-pointer entry points copy in/out and return when the result is ready.
 * `_dev` entry points take device pointers (hipMalloc'd, or torch tensors'
 * data_ptr()) and a `stream` (hipStream_t; NULL = the library's stream for the
 * current device); they are asynchronous unless noted.
 *
 * Every function returns H2G_OK (0) or an error code; h2g_last_error() gives a
 * message.  Reference interfaces replaced are cited per entry point
 * (paths relative to the reference snapshot root).
 */
#ifndef H2G_H
#define H2G_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  H2G_OK = 0,
  H2G_ERR_ARG = 1,     /* invalid argument (the reference panics: assert_eq! in best_multiexp/commit) */
  H2G_ERR_DEVICE = 2,  /* HIP runtime error */
  H2G_ERR_NOMEM = 3,
  H2G_ERR_STATE = 4,   /* not initialised */
  H2G_ERR_HANDLE = 5,  /* unknown descriptor / domain handle */
  H2G_ERR_UNSATISFIED = 6 /* create_proof's self-check: the witness does not satisfy the circuit */
};

int h2g_abi_version(void);
const char* h2g_last_error(void);

/* ---- engine lifecycle ---------------------------------------------------
 * Replaces PlonkEngineConfig::new().set_curve::<G1Affine>().set_msm(engine).build()
 * (halo2_middleware/src/zal.rs:204-243): initialises the listed HIP devices
 * (NULL/0 = device 0). */
int h2g_init(const int* devices, int ndev);
int h2g_shutdown(void);
int h2g_device_count(int* out);
int h2g_set_device(int index); /* index into the h2g_init list */
/* free / total device memory of the current device, after a device-wide synchronize
 * (hipMemGetInfo): what a caller checks descriptor lifetimes against */
int h2g_device_mem_info(uint64_t* free_bytes, uint64_t* total_bytes);

/* ---- MsmAccel<G1Affine> (halo2_middleware/src/zal.rs:57-103) ----------------
 * msm(coeffs, base) -> C::Curve  (zal.rs:58; H2cEngine::msm = best_multiexp, zal.rs:136-138).
 * Result returned affine (out[8]) + identity flag; the shim converts with G1::from. */
int h2g_msm(const uint64_t* coeffs, const uint64_t* bases, size_t n, uint64_t out_affine[8],
            int* out_is_identity);
/* get_coeffs_descriptor / get_base_descriptor (zal.rs:83-84): upload once, keep on device */
int h2g_msm_coeffs_descriptor(const uint64_t* coeffs, size_t n, uint64_t* handle);
int h2g_msm_base_descriptor(const uint64_t* bases, size_t n, uint64_t* handle);
int h2g_msm_descriptor_free(uint64_t handle); /* Drop of a descriptor (zal.rs:47) */
/* Base descriptors keep fixed-base windows ([2^(o_w)] P_i at each window's bit offset o_w,
 * W x n x 64 B of HBM) so the MSM runs one shared bucket set; the _dev variants take device-resident bases /
 * scalars (window_bits 0 = choose). */
int h2g_msm_base_descriptor_dev(const void* d_bases, size_t n, int window_bits, uint64_t* handle);
int h2g_msm_with_cached_base_dev(const void* d_scalars, size_t n, uint64_t base, size_t base_offset,
                                 uint64_t out_affine[8], int* out_is_identity, void* stream);
/* msm_with_cached_scalars / _base / _inputs (zal.rs:86-102); base_offset selects the
 * prefix/sub-slice &bases[off..off+n] used by commit / commit_lagrange
 * (halo2_backend/src/poly/kzg/commitment.rs:316, 365) */
int h2g_msm_with_cached_scalars(uint64_t coeffs, const uint64_t* bases, size_t n, uint64_t out_affine[8],
                                int* out_is_identity);
int h2g_msm_with_cached_base(const uint64_t* coeffs, size_t n, uint64_t base, size_t base_offset,
                             uint64_t out_affine[8], int* out_is_identity);
int h2g_msm_with_cached_inputs(uint64_t coeffs, uint64_t base, size_t base_offset, uint64_t out_affine[8],
                               int* out_is_identity);
/* device-resident MSM: d_out receives 8 u64 (affine, identity = zeros) */
int h2g_msm_dev(const void* d_coeffs, const void* d_bases, size_t n, void* d_out_affine, void* stream);
/* same, with an explicit Pippenger window size c (0 = automatic) */
int h2g_msm_dev_cfg(const void* d_coeffs, const void* d_bases, size_t n, int window_bits, void* d_out_affine,
                    void* stream);
/* device-resident inputs, result returned to the host (synchronous) -- the path
 * MsmAccel::msm takes when the prover keeps polynomials in HBM */
int h2g_msm_dev_host(const void* d_coeffs, const void* d_bases, size_t n, int window_bits, uint64_t out_affine[8],
                     int* out_is_identity, void* stream);
int h2g_descriptor_device_ptr(uint64_t handle, void** d_ptr, size_t* n);
/* Segmented small MSM: nseg independent sums in one launch, one affine result each (a batch
 * verifier's shape: two ~10^2-term sums per proof over bases the proofs share).  CSR over one
 * base array: segment s is the terms j in [seg_off[s], seg_off[s + 1]),
 *   out[s] = sum_j scalars[j] * bases[index ? index[j] : j].
 * Exact for every input: empty segments (identity), zero scalars, identity bases, the same
 * base twice, a base and its negation.  One workgroup per segment: meant for many short
 * segments, correct for any length.
 * _dev: asynchronous on `stream`; the offsets must not decrease and every index must be below
 * nbases -- the caller's contract (an index >= nbases is skipped, never dereferenced; offsets
 * past the scalar array are not detected).  The host entry point checks both (H2G_ERR_ARG),
 * copies in and out and returns when the results are ready. */
int h2g_msm_segmented_dev(const void* d_bases, size_t nbases,      /* G1Affine, identity = zeros */
                          const void* d_scalars,                   /* seg_off[nseg] Fr (Montgomery) */
                          const uint32_t* d_index,                 /* base index per term; NULL = 0..nnz-1 */
                          const uint32_t* d_seg_off,               /* nseg + 1 offsets into scalars / index */
                          size_t nseg, void* d_out_affine,         /* nseg x 8 u64, identity = zeros */
                          void* stream);
int h2g_msm_segmented(const uint64_t* bases, size_t nbases, const uint64_t* scalars, const uint32_t* index,
                      const uint32_t* seg_off, size_t nseg, uint64_t* out_affine);

/* ---- SRS generation on device: g_i = [s^i] G, i < n
 * (ParamsKZG::setup, halo2_backend/src/poly/kzg/commitment.rs:64-90). s in Montgomery form. */
int h2g_srs_setup_dev(const uint64_t s[4], size_t n, void* d_out_affine, void* stream);

/* ---- NTT boundary (new seam; best_fft call sites halo2_backend/src/poly/domain.rs:238, 344
 * and halo2_backend/src/arithmetic.rs:38).  In place, natural order in and out:
 * a_k <- sum_i a_i omega^(ik), n = 2^log_n. */
int h2g_fft(uint64_t* a, uint32_t log_n, const uint64_t omega[4]);
int h2g_fft_dev(void* d_a, uint32_t log_n, const uint64_t omega[4], void* stream);

/* ---- EvaluationDomain (halo2_backend/src/poly/domain.rs) -------------------- */
/* EvaluationDomain::new(j, k) (domain.rs:38-144) */
int h2g_domain_create(uint32_t j, uint32_t k, uint64_t* handle);
int h2g_domain_free(uint64_t handle);
/* consts9 = omega, omega_inv, extended_omega, extended_omega_inv, g_coset, g_coset_inv,
 * ifft_divisor, extended_ifft_divisor, barycentric_weight (Fr, 4 limbs each) */
int h2g_domain_info(uint64_t handle, uint32_t* k, uint32_t* extended_k, uint64_t consts9[36]);
/* lagrange_to_coeff (domain.rs:216-226): in place, n = 2^k */
int h2g_lagrange_to_coeff(uint64_t dom, uint64_t* a);
int h2g_lagrange_to_coeff_dev(uint64_t dom, void* d_a, void* stream);
/* coeff_to_extended (domain.rs:230-244): in n, out 2^extended_k */
int h2g_coeff_to_extended(uint64_t dom, const uint64_t* a, uint64_t* out);
int h2g_coeff_to_extended_dev(uint64_t dom, const void* d_a, void* d_out, void* stream);
/* Sub-coset t of coeff_to_extended, for `count` polynomials at once: outs[i][m] =
 * coeff_to_extended(polys[i])[t + 2^(extended_k - k) m], m < n -- the evaluations on
 * zeta w_ext^t <omega>, by one n-point transform per polynomial (the twist w_ext^(t j) is
 * formed inside it; no extended array exists).  A quotient loop that walks the extended
 * domain sub-coset by sub-coset needs n-point slots only.  t < 2^(extended_k - k); polys /
 * outs are host arrays of `count` pointers to n elements; no outs[i] may overlap a polys[j]
 * (H2G_ERR_ARG).  Any count: NTT_MAX_BATCH (8) transforms share a launch. */
int h2g_coeff_to_subcoset(uint64_t dom, const uint64_t* const* polys, int count, uint64_t t, uint64_t* const* outs);
int h2g_coeff_to_subcoset_dev(uint64_t dom, const void* const* d_polys, int count, uint64_t t, void* const* d_outs,
                              void* stream);
/* The same results by the composition the fused transform replaces -- a twist launch per
 * column, then the batched NTT -- for measurements and cross-checks (tools/streamed_bench.py). */
int h2g_debug_coeff_to_subcoset_unfused_dev(uint64_t dom, const void* const* d_polys, int count, uint64_t t,
                                            void* const* d_outs, void* stream);
/* extended_to_coeff (domain.rs:271-293): in 2^extended_k, out n*(j-1) (truncated) */
int h2g_extended_to_coeff(uint64_t dom, const uint64_t* a, uint64_t* out);
int h2g_extended_to_coeff_dev(uint64_t dom, const void* d_a, void* d_out, void* stream);
/* divide_by_vanishing_poly (domain.rs:297-316): in place on 2^extended_k */
int h2g_divide_by_vanishing_poly(uint64_t dom, uint64_t* a);
int h2g_divide_by_vanishing_poly_dev(uint64_t dom, void* d_a, void* stream);
/* test seam: which kernels a transform of 2^log_n points takes -- the plan every NTT launches
 * from, as a function of the call's shape alone.  n_in: the inputs present (zero beyond);
 * out_len: the outputs kept, 0 = all; count: transforms per launch (< 1 = 1; more than 8:
 * H2G_ERR_ARG); in_twist: the sub-coset transform's fused input twist; cus: the compute units
 * planned for, 0 = the current device's as the library sees it (256 without a device);
 * epilogue_one: no constant is left for the last pass (lagrange_to_coeff, coeff_to_extended
 * and coeff_to_subcoset above 2^10 points; extended_to_coeff's zeta powers always leave one).
 * Host only: needs no h2g_init. */
enum {
  H2G_NTT_FIRST_ONE_BLOCK = 0, /* the whole transform in one block's LDS: log_n <= 10, passes == 1 */
  H2G_NTT_FIRST_SPARSE = 1,    /* 8-point first pass of two inputs: lg[0] == 3, n_in <= 2^log_n / 4 */
  H2G_NTT_FIRST_PLAIN = 2,
  H2G_NTT_FIRST_TWISTED = 3    /* in_twist above 2^10 points */
};
typedef struct h2g_ntt_plan {
  int32_t passes;      /* P */
  int32_t lg[6];       /* bits of pass p < P (3..6, the last 6), 0 beyond */
  int32_t first;       /* H2G_NTT_FIRST_* */
  int32_t last_trunc;  /* last pass stores under y < out_len (out_len < 2^log_n); 0 when passes == 1 */
  int32_t last_one;    /* last pass without its epilogue product; 0 when passes == 1 */
  int32_t cus;         /* the compute units planned for */
  uint32_t blocks;     /* blocks of 4 waves that cover a pass's 2^log_n / 512 wave items; 0 when passes == 1 */
  uint32_t first_grid; /* grid.x of the first pass */
  uint32_t pgrid[6];   /* grid.x of the persistent pass p, 0 < p < P - 1: min(blocks, 2 cus / count), at
                          least 1; 0 elsewhere.  Its waves stride over the items: when pgrid does not
                          divide blocks, some take one item more than others */
} h2g_ntt_plan;
int h2g_debug_ntt_plan(uint32_t log_n, uint64_t n_in, uint64_t out_len, int count, int in_twist, int cus,
                       int epilogue_one, h2g_ntt_plan* plan);
/* test seam: what an MSM of n points decides before it allocates or launches -- the plan
 * every MSM pipeline runs from, as a function of the call's shape alone.  c: window bits, 0 =
 * the library's choice for n (variable- or fixed-base); fixed: fixed-base tables (ceil(255 / c)
 * windows of balanced widths sharing one bucket set per MSM) with nbatch MSMs in one pipeline
 * (1..64; variable-base: 1); item_len: entries per accumulation chunk, 0 = the adaptive rule.
 * H2G_ERR_ARG (plan untouched) for a shape the pipeline refuses: the batch range, n W nbatch
 * >= 2^31 entries, more than 2048 coarse bins (sets x 2^(c-1) > 2^22 buckets), more than 256
 * bucket sets.  Host only: needs no h2g_init. */
typedef struct h2g_msm_plan {
  uint64_t total;      /* entry bound n W nbatch */
  uint64_t nb_eff;     /* buckets most windows can reach (chunk rule) */
  uint64_t nchunks;    /* the most accumulation chunks: grids and boundary slots are sized for it */
  uint64_t bytes[10];  /* workspace buffers: entries / whole buckets, values, big-bucket items, boundary
                          slots, buckets, reduction levels, window sums, counters, multi-item buckets,
                          items' partial sums */
  uint64_t scratch_words; /* 32-bit words of the partition's count / offset scratch */
  uint32_t c, W;          /* window bits, windows */
  uint32_t fixed, nbatch;
  uint32_t WB, NB, nbt;   /* bucket sets, buckets per set 2^(c-1), their product */
  uint32_t chunk_len;     /* the host's entries per chunk */
  uint32_t chunk_adapt;   /* 1: the device shortens it when few entries exist */
  uint32_t fb, ncoarse, kblocks; /* partition: fine bits, coarse bins, 1024-key scan blocks */
  uint32_t staged;        /* the partition's second round in its LDS-staged form */
  uint32_t fixup_q;       /* lanes per bucket of the fixup: 4 or 1 */
  uint32_t red_plane;     /* reduction: 1 bit planes, 0 per-group scalar multiplications (rscale) */
  uint32_t plane_q, plane_lb, rgp, e0, m1p, nblk_p; /* planes: lanes per group (4, 1), log2 groups per
                             block, buckets per group and its log2, groups and blocks per set; 0 under rscale */
  uint32_t m1, nblk;      /* rscale: groups of 8 buckets and blocks of 256 groups per set; 0 under planes */
  uint32_t reserved;
} h2g_msm_plan;
int h2g_debug_msm_plan(uint64_t n, int c, int fixed, int nbatch, uint32_t item_len, h2g_msm_plan* plan);
/* test seam: the per-launch capacities by which the prover's host loops split wide work, so that
 * tests can take their shapes from them (cap - 1, cap, cap + 1, 2 cap + 1).  Writes the first
 * min(max, H2G_LIMIT_COUNT) of them to out, in the order of the enum, and H2G_LIMIT_COUNT to
 * *count.  Host only: needs no h2g_init. */
enum {
  H2G_LIMIT_COPY_COLS = 0,    /* advice columns per copy / column-sum launch (device-resident advice, check_witness) */
  H2G_LIMIT_PREFIX_DIFF = 1,  /* permuted lookup columns per prefix-difference launch */
  H2G_LIMIT_COMPRESS_BATCH = 2, /* lookup / shuffle expressions per compression launch */
  H2G_LIMIT_LOOKUP_KEYS_BATCH = 3, /* columns per sort-key launch */
  H2G_LIMIT_PERM_COLS = 4,    /* permutation columns per numerator / denominator launch */
  H2G_LIMIT_LIN_TERMS = 5,    /* terms per linear-combination launch (the multi-open uses one or two fewer) */
  H2G_LIMIT_NTT_BATCH = 6,    /* transforms per launch */
  H2G_LIMIT_POLY_INV_BATCH = 7, /* arrays per batched inversion / prefix-product launch */
  H2G_LIMIT_MSM_BATCH = 8,    /* MSMs per batched pipeline */
  H2G_LIMIT_MSM_RING = 9,     /* result slots of one block of the asynchronous MSMs' ring (more are added on demand) */
  H2G_LIMIT_COUNT = 10
};
int h2g_debug_limits(int32_t* out, int max, int* count);
/* test seam: how many commitments of n points the prover batches into one MSM pipeline against
 * fixed-base windows of table_c bits (1: each goes alone).  Never a batch that
 * h2g_debug_msm_plan(n, table_c, 1, chunk) refuses.  Host only: needs no h2g_init. */
int h2g_debug_commit_batch_chunk(int table_c, uint64_t n, int* chunk);
/* test seam: the prover's commitment schedule on its own.  nb_total MSMs sum_i d_scalars[b][i] *
 * bases[base_offset + i] (i < n) against a base descriptor's fixed-base windows
 * (h2g_msm_base_descriptor_dev), launched back to back in ceil(nb_total / chunk) batched
 * pipelines of up to `chunk` (1..64) MSMs -- chunk = 1: one plain pipeline each, the schedule of
 * commitments too large to batch -- and collected only after the last launch, as a proof stage
 * does.  out_affine: nb_total x 8 limbs ((0, 0) for the identity); is_identity: nb_total flags,
 * or null.  H2G_ERR_ARG, with nothing launched, when a batch is a shape the MSM refuses. */
int h2g_debug_msm_batches_dev(uint64_t base, size_t base_offset, const void* const* d_scalars, int nb_total,
                              int chunk, size_t n, uint64_t* out_affine, int32_t* is_identity);

/* ---- Polynomial<F, B> arithmetic (halo2_backend/src/poly.rs:200-276) ---------
 * op: 0 add a+b, 1 sub a-b, 2 mul a*b, 3 scale a*c, 4 sub_const a-c, 5 add_const a+c,
 *     6 axpy a*c+b.  c is a host Fr (4 limbs), ignored by ops 0-2. */
int h2g_fr_op(int op, const uint64_t* a, const uint64_t* b, const uint64_t c[4], uint64_t* out, size_t n);
int h2g_fr_op_dev(int op, const void* d_a, const void* d_b, const uint64_t c[4], void* d_out, size_t n,
                  void* stream);
/* ff::BatchInvert (zeros stay zero); permutation/prover.rs:124, lookup/prover.rs:225 */
int h2g_fr_batch_invert(uint64_t* a, size_t n);
int h2g_fr_batch_invert_dev(void* d_a, size_t n, void* stream);
/* out_i = prod_{j<=i} a_j; grand products permutation/prover.rs:160-166 */
int h2g_fr_prefix_product(const uint64_t* a, uint64_t* out, size_t n);
int h2g_fr_prefix_product_dev(const void* d_a, void* d_out, size_t n, void* stream);
/* exclusive prefix sum of n u32 (n < 2^32; d_in == d_out allowed): the counts-to-offsets scan
 * of the lookup argument's sorts and compactions (lookup/prover.rs:410-494) */
int h2g_u32_exclusive_scan_dev(const void* d_in, void* d_out, size_t n, void* stream);

/* ---- a witness of Assigned<F> cells to field elements (csrc/assigned.hip) ------------
 * batch_invert_assigned (halo2_frontend/src/circuit.rs:363-404), the last step of
 * WitnessCalculator::calc: the frontend holds every advice cell as Zero, Trivial(x) or
 * Rational(numerator, denominator) (halo2_frontend/src/plonk/assigned.rs), inverts the
 * Rational cells' denominators in one batch and multiplies (Assigned::evaluate,
 * assigned.rs:352-364).  The wire form is what one walk over Vec<Vec<Assigned<F>>> emits:
 *   num   : ncells Fr, Assigned::numerator() of every cell (0 for Zero)
 *   index : nden flat cell indices into num, one per Rational cell, strictly increasing
 *   den   : nden Fr, that cell's denominator
 * out[index[j]] = num[index[j]] * den[j]^-1, and 0 where den[j] == 0 (ff::BatchInvert skips
 * zeros; x / 0 = 0 as in assigned.rs:280-295); a denominator of 1 is inverted like any other.
 * Every cell that is not listed: out = num.  out == num (in place) touches only the listed
 * cells, so its cost follows nden, not ncells.  den is not modified.  nden == 0 is a copy
 * (nothing in place), ncells == 0 is H2G_OK.  Field inverses are unique: the result is the
 * reference's for every input.
 * Host entry: validates before it touches the device -- a missing pointer, an index >=
 * ncells or a list that is not strictly increasing is H2G_ERR_ARG, the message names the
 * entry, out is left as it was -- then copies in and out and returns with the result.
 * _dev: device pointers, 16-byte aligned (H2G_ERR_ARG otherwise); asynchronous on `stream`
 * like h2g_fr_batch_invert_dev, with nden Fr of scratch from the device workspace
 * (H2G_ERR_NOMEM, nothing left allocated, if that cannot grow).  The index contract is the
 * caller's: an index >= ncells is skipped and never dereferenced, a repeated index leaves that
 * cell with an unspecified value.  Elements are reduced Montgomery limbs, as everywhere.
 * The inverses are never stored: the inversion's backward pass, which holds den[j]^-1 in
 * registers, loads index[j] and num[index[j]] and stores out[index[j]]. */
int h2g_assigned_to_fr(const uint64_t* num, size_t ncells, const uint64_t* index, const uint64_t* den, size_t nden,
                       uint64_t* out);
int h2g_assigned_to_fr_dev(const void* d_num, size_t ncells, const void* d_index, const void* d_den, size_t nden,
                           void* d_out, void* stream);
/* test seams (tests/test_gpu_assigned.py).  h2g_debug_assigned_per: the denominators per
 * first-level thread the size rule takes for nden of them (2, 4, 8 or 16; host only: needs no
 * h2g_init).  h2g_debug_assigned_to_fr_dev: h2g_assigned_to_fr_dev with that many at any nden;
 * per = 0 is the rule, a value that is none of those H2G_ERR_ARG. */
int h2g_debug_assigned_per(size_t nden, int* per);
int h2g_debug_assigned_to_fr_dev(const void* d_num, size_t ncells, const void* d_index, const void* d_den,
                                 size_t nden, void* d_out, int per, void* stream);

/* ---- device memory / stream helpers --------------------------------------- */
int h2g_dev_alloc(size_t bytes, void** d_ptr);
int h2g_dev_free(void* d_ptr);
int h2g_memcpy_htod(void* d_dst, const void* h_src, size_t bytes);
int h2g_memcpy_dtoh(void* h_dst, const void* d_src, size_t bytes);
int h2g_synchronize(void);
/* elapsed time (ms) of `fn`-free timing: record events on a stream */
int h2g_event_create(void** ev);
int h2g_event_destroy(void* ev);
int h2g_event_record(void* ev, void* stream);
int h2g_event_elapsed_ms(void* start, void* stop, float* ms);

/* ---- profiling: per-phase HIP-event times of MSM calls made while enabled.
 * Phases (in order): partition_coarse (digits -> coarse bins), partition_fine (bins -> bucket
 * order), bucket_bounds, accumulate, bucket_fixup, reduce.  collect() synchronises, returns the
 * per-phase sums (ms) over `calls` MSMs and resets.  With max_phases >= 8, ms[6] and ms[7] are
 * the busy time (union of the intervals) of the accumulate phases and of the whole MSMs:
 * MSMs on the two MSM streams overlap, so work / union is the aggregate rate. */
int h2g_profile_enable(int on);
int h2g_profile_msm_collect(float* ms, int max_phases, int* n_phases, int* calls);
/* the profiled MSMs' sorted entries (nonzero signed digits = mixed additions in the
 * accumulation) summed, before collect() resets them; *uncounted = MSMs past the
 * recorder's capacity (may be NULL) */
int h2g_profile_msm_entries(uint64_t* total, int* uncounted);
/* box calibration (bench line): Montgomery product throughput of this GPU now, in the two
 * limb forms the prover uses -- out[0] 8 x 32-bit FIPS, out[1] 9 x 29-bit (G products/s)
 * -- out[2] the shader clock during the run (GHz, s_memtime vs s_memrealtime), out[3] the
 * wall ms spent (~100); max >= 4.  Not part of the prover's interface. */
int h2g_profile_box_calibrate(double* out, int max);

/* ---- host-side point helpers (used to combine per-GPU MSM partials) -------- */
int h2g_g1_add_affine(const uint64_t a[8], const uint64_t b[8], uint64_t out[8]);


/* ---- create_proof (BN254 / KZG / SHPLONK, Blake2b transcript) -------------
 * The backend entry points of halo2_backend/src/plonk/{keygen.rs, prover.rs}:
 *   ParamsKZG::{setup, read}   poly/kzg/commitment.rs:64-131,167-267  -> h2g_params_*
 *   ParamsKZG::{from_parts, downsize}  kzg/commitment.rs:135-154,291-299 -> h2g_params_from_parts / _downsize
 *   keygen_vk + keygen_pk      plonk/keygen.rs:43-190                  -> h2g_keygen
 *   create_proof(params, pk, circuits=[1], instances, rng, transcript)
 *                              plonk/prover.rs:174-899 (ProverSingle)  -> h2g_create_proof
 * The circuit is the backend's CompiledCircuit (halo2_middleware/src/circuit.rs):
 * gates as flattened ExpressionMid nodes, permutation columns + copies, fixed values.
 * Node = 4 x int32 (op, a, b, c): op 0 CONST (a = constant index), 1 QUERY (a = column
 * type 0 advice / 1 fixed / 2 instance, b = column index, c = rotation), 2 NEG (a),
 * 3 SUM (a, b), 4 PROD (a, b), 5 CHALLENGE (a = challenge index; ExpressionMid::Challenge).
 * Copy = 6 x int32 (ltype, lindex, lrow, rtype, rindex, rrow).
 * Supported: advice phases and challenges (advice_column_phase / challenge_phase of
 * ConstraintSystemMid, circuit.rs), gates, permutation, lookups, shuffles.
 * rng: ChaCha20Rng::from_seed(rng_seed); vanishing_threads: the thread count that
 * splits the vanishing argument's random polynomial into ChaCha streams
 * (vanishing/prover.rs:57-81), part of the proof's determinism. */
typedef struct {
  uint32_t k, num_advice, num_fixed, num_instance;
  uint32_t num_gates;
  const int32_t* gate_roots;
  uint32_t num_nodes;
  const int32_t* nodes;
  uint32_t num_constants;
  const uint64_t* constants;      /* Fr */
  uint32_t num_perm_columns;
  const int32_t* perm_columns;    /* (type, index) pairs, permutation ArgumentMid.columns order */
  uint32_t num_copies;
  const int32_t* copies;
  const uint64_t* fixed_values;   /* num_fixed x n Fr (Lagrange) */
  const uint8_t* unblinded;       /* num_advice flags (unblinded_advice_columns) or NULL */
  const uint64_t* transcript_repr; /* vk.transcript_repr (Fr) */
  /* lookup arguments (lookup::Argument): per lookup m (input, table) expression pairs;
   * roots: per lookup m input roots then m table roots */
  uint32_t num_lookups;
  const uint32_t* lookup_sizes;
  const int32_t* lookup_roots;
  /* shuffle arguments (shuffle::Argument): per shuffle m input roots then m shuffle roots */
  uint32_t num_shuffles;
  const uint32_t* shuffle_sizes;
  const int32_t* shuffle_roots;
  /* phases (appended; NULL / 0 = one phase, no challenges): advice_phase[num_advice]
   * (advice_column_phase), challenge_phase[num_challenges] (challenge_phase) */
  const uint8_t* advice_phase;
  uint32_t num_challenges;
  const uint8_t* challenge_phase;
} h2g_circuit;

/* SRS resident on the current device: g[n] and g_lagrange[n] (G1Affine) from the host... */
int h2g_params_create(uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, uint64_t* handle);
/* ...or generated on the device from the toxic secret s (ParamsKZG::setup; tests/bench) */
int h2g_params_setup(uint32_t k, const uint64_t s[4], uint64_t* handle);
int h2g_params_export(uint64_t params, uint64_t* g, uint64_t* g_lagrange); /* n x 8 u64 each, may be NULL */
int h2g_params_free(uint64_t params);
/* the G2 points of ParamsKZG (kzg/commitment.rs:26-27): g2 and s_g2, 16 u64 each
 * (x.c0, x.c1, y.c0, y.c1 in Montgomery form); setup computes them, create needs set_g2
 * before the params can be written */
int h2g_params_g2(uint64_t params, uint64_t g2[16], uint64_t s_g2[16]);
int h2g_params_set_g2(uint64_t params, const uint64_t g2[16], const uint64_t s_g2[16]);

/* ---- from a ceremony's monomial powers to params of the circuit's size ----
 * g_to_lagrange (halo2_backend/src/arithmetic.rs:30-54): n = 2^k G1Affine in (identity = zeros
 * allowed anywhere), the Lagrange basis L_i = [n^-1] sum_j [omega^(-ij)] g_j out, natural order,
 * bit-identical to the reference's for every input (a G1 group FFT on the device,
 * csrc/g1_fft.hip).  k <= 27.  The points are not checked for being on the curve (as with
 * h2g_params_create); off-curve input gives unspecified points, never a fault.
 * _dev: device pointers, d_out may equal d_g.  Queued on `stream` (NULL: the library's), but
 * the call returns only after the work has completed: its scratch (16 * 2^k bytes of
 * twiddles) is taken for the call and released before it returns; H2G_ERR_NOMEM if it cannot
 * be had, with nothing left allocated. */
int h2g_g1_to_lagrange_dev(const void* d_g, uint32_t k, void* d_out, void* stream);
int h2g_g1_to_lagrange(const uint64_t* g, uint32_t k, uint64_t* out);   /* host copy in / out */
/* ParamsKZG::from_parts (kzg/commitment.rs:135-154).  g_lagrange == NULL: computed on the
 * device from g (above); given: stored as it is.  g2 / s_g2: both given (validated as
 * h2g_params_set_g2 does) or both NULL (params without G2); exactly one is H2G_ERR_ARG.  The G1
 * points are not checked for being on the curve.  The params have their fixed-base windows
 * when the call returns. */
int h2g_params_from_parts(uint32_t k, const uint64_t* g, const uint64_t* g_lagrange,
                          const uint64_t g2[16], const uint64_t s_g2[16], uint64_t* handle);
/* ParamsKZG::downsize (kzg/commitment.rs:291-299): a NEW params object of size 2^k <= the
 * source's (the reference shrinks in place; here the source stays valid and unchanged, keys
 * made from it keep working, and one resident ceremony SRS serves several circuit sizes):
 * g truncated (device-to-device), g_lagrange recomputed (also when k is the source's, as the
 * reference does), g2 / s_g2 carried over (params without G2 give params without G2), own
 * fixed-base windows; slab windows (h2g_params_set_slab) are not inherited.  k above the
 * source's: H2G_ERR_ARG; unknown handle: H2G_ERR_HANDLE; params on another device:
 * H2G_ERR_ARG. */
int h2g_params_downsize(uint64_t params, uint32_t k, uint64_t* handle);

/* ---- serialisation: SerdeFormat (halo2_backend/src/helpers.rs:8-21) -----------------
 * format 1 RawBytes (uncompressed points, Montgomery limbs; reads check that field
 * elements are below the modulus and points lie on the curve), 2 RawBytesUnchecked
 * (no checks), 0 Processed (helpers.rs:36-100: G1 points as 32-B GroupEncoding -- x
 * canonical LE, bit 7 of the last byte = y odd, identity all zero --, G2 points as 64 B
 * (x.c0 || x.c1, sign from y.c0), field elements canonical LE (to_repr); reads decompress
 * on the device and refuse x >= p, x without a curve point and field elements >= r).
 * Writers: out == NULL returns the byte length in *len.
 *   ParamsKZG::write_custom / read_custom  kzg/commitment.rs:166-267
 *   ProvingKey::write / read               plonk.rs:311-359 (+ VerifyingKey::write/read :73-129)
 * h2g_pk_read takes the constraint system from `circuit` (as the reference takes `cs`)
 * and every array of the key from the bytes; circuit->fixed_values / ->copies unused. */
int h2g_params_write(uint64_t params, int format, uint8_t* out, size_t cap, size_t* len);
int h2g_params_read(const uint8_t* buf, size_t len, int format, uint64_t* handle);

int h2g_keygen(uint64_t params, const h2g_circuit* circuit, uint64_t* pk);
int h2g_pk_free(uint64_t pk);
int h2g_pk_write(uint64_t pk, int format, uint8_t* out, size_t cap, size_t* len);
int h2g_pk_read(uint64_t params, const h2g_circuit* circuit, const uint8_t* buf, size_t len, int format,
                uint64_t* pk);
/* Key options.  `cosets` says how a key holds the columns that the quotient evaluation
 * (evaluate_h) reads on the extended domain:
 *   H2G_COSETS_RESIDENT  every such column as its extended coset, 2^extended_k elements:
 *                        the key's fixed / permutation / l_0, l_last, l_active cosets and,
 *                        per circuit of a proof, one per advice and instance column, one per
 *                        permutation set, three per lookup and one per shuffle.
 *   H2G_COSETS_STREAMED  one n-element slot per such column.  create_proof evaluates h(X)
 *                        one sub-coset of the extended domain at a time and refills the
 *                        slots from the coefficient forms for each (h2g_coeff_to_subcoset's
 *                        transform); only h(X)'s own three buffers stay extended.  Proofs,
 *                        key bytes (h2g_pk_write), verifying key and witness checks are the
 *                        same bytes as a resident key's; the price is the key's fixed /
 *                        permutation / l transforms redone in every proof.  Not combined
 *                        with an SPMD transport of more than one rank (H2G_ERR_STATE).
 * `size` is sizeof(h2g_key_options).  NULL options or mode 0 are h2g_keygen / h2g_pk_read
 * exactly; an unknown mode is H2G_ERR_ARG.  h2g_pk_read_opts in streamed mode accepts and
 * refuses the same files: the file's cosets pass the format's checks in scratch and are
 * dropped. */
enum { H2G_COSETS_RESIDENT = 0, H2G_COSETS_STREAMED = 1 };
typedef struct { uint32_t size; uint32_t cosets; } h2g_key_options;
int h2g_keygen_opts(uint64_t params, const h2g_circuit* circuit, const h2g_key_options* opts, uint64_t* pk);
int h2g_pk_read_opts(uint64_t params, const h2g_circuit* circuit, const uint8_t* buf, size_t len, int format,
                     const h2g_key_options* opts, uint64_t* pk);
/* out[0] the coset mode; out[1] the device bytes the key holds now (its arrays and the
 * per-proof workspace grown so far); out[2] those of them in arrays of 2^extended_k
 * elements; out[3] 0. */
int h2g_pk_memory(uint64_t pk, uint64_t out[4]);
/* degree, blinding_factors, extended_k, #perm sets, #advice/#fixed/#instance queries */
int h2g_pk_info(uint64_t pk, int32_t info[8]);
/* Diagnostics (read only): the value width in bits that the next proof's sort will assume
 * for every lookup, entry circuit * num_lookups + lookup, as the proofs made with this key
 * so far measured it: <= 48 the value itself is the sort key, wider a 48-bit window below
 * the top bit (with an order check), 0 the full 256-bit sort, 64 before the first proof.
 * The list covers as many circuits as the largest proof so far proved at once (one after
 * keygen).  Writes min(*count, max) entries; out may be NULL when max is 0. */
int h2g_pk_lookup_sort_hints(uint64_t pk, int32_t* out, int max, int* count);
/* the verifying key's commitments: VerifyingKey::fixed_commitments() (plonk.rs:228-231) and
 * the permutation VerifyingKey's commitments (plonk/permutation.rs:18-47), G1Affine (8 u64 each):
 * fixed[num_fixed], perm[num_perm_columns]; either may be NULL */
int h2g_pk_vk_commitments(uint64_t pk, uint64_t* fixed, uint64_t* perm);
/* the multi-open argument h2g_create_proof ends with -- the reference's Prover type
 * parameter of create_proof (halo2_proofs/src/plonk/prover.rs:19-36): 0 ProverSHPLONK
 * (default; poly/kzg/multiopen/shplonk/prover.rs:121-305), 1 ProverGWC
 * (poly/kzg/multiopen/gwc/prover.rs:40-90) */
int h2g_pk_set_multiopen(uint64_t pk, int scheme);
/* the transcript the proof is written with -- create_proof's TranscriptWrite type
 * parameter: 0 Blake2bWrite (default; halo2_backend/src/transcript.rs:291-419),
 * 1 Keccak256Write (EVM-verifiable; transcript.rs:299-463) */
int h2g_pk_set_transcript(uint64_t pk, int kind);

/* advice: num_advice x n Fr; instance: num_instance x n Fr (zero padded), of which
 * instance_lens[i] values enter the transcript.  Writes the proof bytes.
 * advice_on_device != 0: `advice` is a device pointer (inputs resident in HBM), 16-byte
 * aligned (H2G_ERR_ARG otherwise; the columns are read in 16-byte chunks). */
int h2g_create_proof(uint64_t params, uint64_t pk, const uint64_t* advice, int advice_on_device,
                     const uint64_t* instance, const uint32_t* instance_lens, const uint8_t rng_seed[32],
                     uint32_t vanishing_threads, uint8_t* proof, size_t proof_cap, size_t* proof_len);
/* Prover::commit_phase driven by the caller's witness generator (plonk/prover.rs:309-494):
 * before committing phase p (0..max advice phase) the prover calls
 *   fill(ctx, p, challenges, advice)
 * with the challenges squeezed so far (num_challenges x 4 u64 Montgomery limbs; those of
 * phases >= p are zero) and the host advice buffer (num_advice x n Fr), in which the
 * callback writes the columns of phase p (staging owned by the key, pinned when the host
 * allows: num_advice x n x 32 B for the key's lifetime; the prover reads only phase p's
 * columns from it, other columns may hold anything).  fill must write rows
 * [0, n - blinding_factors - 1) of every phase-p column; the prover zeroes the unusable rows
 * of unblinded columns before calling it (blinded ones receive randomness).  Nonzero from
 * fill fails the proof with H2G_ERR_ARG.  Callbacks (fill, and the shard transport's
 * launch / collect) run on the calling thread with the library lock held: they must not
 * wait on h2g calls made from other threads.  h2g_create_proof is the same prover with every phase read from
 * `advice` (a witness that was computed with the challenges already known). */
typedef struct {
  void* ctx;
  int (*fill)(void* ctx, uint32_t phase, const uint64_t* challenges, uint64_t* advice);
} h2g_witness_source;
int h2g_create_proof_phased(uint64_t params, uint64_t pk, const h2g_witness_source* witness,
                            const uint64_t* instance, const uint32_t* instance_lens, const uint8_t rng_seed[32],
                            uint32_t vanishing_threads, uint8_t* proof, size_t proof_cap, size_t* proof_len);
/* ---- create_proof with the reference's full argument list ------------------------
 * create_proof(params, pk, circuits: &[C], instances: &[&[&[F]]], rng: R: RngCore,
 * transcript) (halo2_proofs/src/plonk/prover.rs:19-36; Prover::new_with_engine /
 * commit_phase / create_proof, halo2_backend/src/plonk/prover.rs:174-899): several
 * circuits of one key in one proof, in the reference's interleaving -- instances per
 * circuit, each phase's advice commitments circuit by circuit, then per circuit its
 * lookups, permutation sets, lookup products and shuffles, one vanishing argument and one
 * h(X) over all circuits (evaluation.rs:365-620), evaluations and queries circuit by
 * circuit before the fixed and common ones.
 * rng: the caller's `R: RngCore`, drawn in the reference's order.  Two kinds
 * of draw exist: F::random(&mut rng) (blinding rows and blinds) and rng.fill_bytes(&mut
 * [u8; 32]) (the vanishing argument's ChaCha20 seeds, vanishing/prover.rs:69-73).
 *   random_fr : F::random(&mut rng) as 4 Montgomery limbs (the Rust shim calls
 *               Fr::random itself, so the proof does not depend on how halo2curves
 *               consumes the RNG); NULL = fill_bytes(64) read as from_uniform_bytes
 *   fill_bytes: RngCore::fill_bytes(out[0..len]); required, even with random_fr (the
 *               vanishing seeds are fill_bytes draws) -- NULL fails the call up front
 * Nonzero from either fails the proof with H2G_ERR_ARG. */
typedef struct {
  void* ctx;
  int (*fill_bytes)(void* ctx, uint8_t* out, size_t len);
  int (*random_fr)(void* ctx, uint64_t out[4]);
} h2g_rng;
/* Prover::commit_phase's witness per circuit: like h2g_witness_source.fill, for circuit c */
typedef struct {
  void* ctx;
  int (*fill)(void* ctx, uint32_t circuit, uint32_t phase, const uint64_t* challenges, uint64_t* advice);
} h2g_witness_source_multi;
typedef struct {
  uint32_t num_circuits;                /* >= 1 */
  const uint64_t* const* advice;        /* [num_circuits] num_advice x n Fr, or NULL with `witness` */
  int advice_on_device;                 /* advice[c] are device pointers */
  const h2g_witness_source_multi* witness;
  const uint64_t* const* instance;      /* [num_circuits] num_instance x n Fr (zero padded) */
  const uint32_t* const* instance_lens; /* [num_circuits] num_instance values each */
  const h2g_rng* rng;                   /* NULL: ChaCha20Rng::from_seed(rng_seed) */
  const uint8_t* rng_seed;
  uint32_t vanishing_threads;
} h2g_prove_inputs;
int h2g_create_proof_multi(uint64_t params, uint64_t pk, const h2g_prove_inputs* in, uint8_t* proof,
                           size_t proof_cap, size_t* proof_len);
/* h2g_create_proof_multi with the witness as the frontend holds it (Assigned<F> cells, the
 * wire form of h2g_assigned_to_fr): batch_invert_assigned (circuit.rs:363-404) runs on the
 * device, not in the caller's WitnessCalculator::calc.  in->advice and in->witness must both
 * be NULL (H2G_ERR_ARG otherwise); everything else in h2g_prove_inputs keeps its meaning.
 * fill is h2g_witness_source_multi.fill that writes phase p's NUMERATORS into `advice` (the
 * key's host staging) and points *dens at this (circuit, phase)'s Rational cells: flat
 * indices into `advice` (column * n + row), strictly increasing, and their denominators --
 * memory the callback owns, valid until the next fill call or the return of the proof.
 * count == 0 (index / den may be NULL) is a witness without divisions.  Entries that name
 * cells outside phase p's columns are ignored.  An index >= num_advice * n, or a list that is
 * not strictly increasing, fails the proof with H2G_ERR_ARG (the message names the circuit and
 * the phase).  The proof is h2g_create_proof_multi's for the evaluated advice, byte for byte.
 * The phase's columns and the list go up to a scratch the key owns (num_advice x n Fr, counted
 * by h2g_pk_memory, released by h2g_pk_free), are converted there in place on the prover's
 * stream, and enter the prover as device advice.  Under a shard or SPMD transport every rank's
 * callback supplies the same witness, as with h2g_witness_source. */
typedef struct { const uint64_t* index; const uint64_t* den; size_t count; } h2g_assigned_dens;
typedef struct {
  void* ctx;
  int (*fill)(void* ctx, uint32_t circuit, uint32_t phase, const uint64_t* challenges, uint64_t* advice,
              h2g_assigned_dens* dens);
} h2g_assigned_source;
int h2g_create_proof_assigned(uint64_t params, uint64_t pk, const h2g_prove_inputs* in,
                              const h2g_assigned_source* source, uint8_t* proof, size_t proof_cap, size_t* proof_len);
/* a native ChaCha20Rng::from_seed(seed) (rand_chacha 0.3) as an h2g_rng: *out's callbacks
 * draw from it (the RngCore a Rust host passes to create_proof, without the host); the
 * proof equals the rng_seed path's bytes.  h2g_rng_free releases it. */
int h2g_rng_chacha20(const uint8_t seed[32], h2g_rng* out, uint64_t* handle);
int h2g_rng_free(uint64_t handle);
/* the challenges of the last proof (num_challenges x 4 u64), *count = num_challenges */
int h2g_last_challenges(uint64_t* out, int max, int* count);
/* ---- which constraints does a witness leave unsatisfied? ----------------------------
 * MockProver::verify (halo2_frontend/src/dev.rs:742-1166) for a complete witness of ONE
 * circuit, on the device, before any proof is made.  h2g_create_proof* accepts any advice;
 * this call says which gate, lookup, shuffle or copy is wrong and at which row.
 * Let u = n - (blinding_factors + 1).  The library works on its own copy of the advice
 * (uploaded as h2g_create_proof uploads it) and fills rows [u, n) the way the prover will:
 * zero for unblinded columns, Fr::random of a ChaCha20 stream seeded from `seed` for the
 * others.  This is the one deliberate difference from MockProver, so that "no failures"
 * means "the proof will verify": a gate that is live in a blinding row, or reads a blinded
 * cell from a usable row, fails with overwhelming probability (kind 2, or kind 1 at the
 * reading row).
 *   gates    every gate polynomial at all n rows, rotations mod n, challenges from
 *            `challenges` (MockProver's self.challenges)              dev.rs:849-925
 *   lookups  the input tuple of every row < u must occur among the table tuples of rows < u
 *                                                                     dev.rs:957-1052
 *   shuffles the input and shuffle tuples of rows < u must be equal as multisets; one
 *            record per failing shuffle, row = H2G_CHECK_NO_ROW       dev.rs:1054-1112
 *   copies   the two cells of every listed copy must be equal          dev.rs:1114-1142
 * Lookup and shuffle tuples are compared through their theta-compression with theta drawn
 * from `seed`: PROBABILISTIC, a wrong m-expression argument over n rows passes with
 * probability about m n / r (r the 254-bit field order).  Gates and copies are exact.
 * Returns H2G_OK whether or not there are failures: *total is their exact number, out
 * receives min(*total, cap) records sorted by (kind, index, row) -- when *total > cap, any cap
 * of the failures.  out == NULL or cap == 0 only counts.  H2G_ERR_ARG: challenges missing
 * on a key with challenges, a copy naming a column or row out of range, misaligned device
 * advice, a missing advice or instance array; H2G_ERR_HANDLE: unknown key.  Synchronous;
 * the key stays usable and later proofs have the bytes they would have had.  Shard and SPMD
 * transports take no part. */
enum {
  H2G_CHECK_GATE = 1,          /* gate `index` is nonzero at usable row `row` */
  H2G_CHECK_GATE_BLINDING = 2, /* gate `index` is nonzero at row >= n - (blinding_factors + 1) */
  H2G_CHECK_LOOKUP = 3,        /* lookup `index`: input of usable row `row` not in the table */
  H2G_CHECK_SHUFFLE = 4,       /* shuffle `index`: the multisets differ; row = H2G_CHECK_NO_ROW */
  H2G_CHECK_COPY = 5           /* copies[index]: the two cells differ; row = its left row */
};
#define H2G_CHECK_NO_ROW 0xFFFFFFFFu
typedef struct {
  uint32_t kind, index, row, reserved;
} h2g_check_failure;
typedef struct {
  const uint64_t* advice;     /* num_advice x n Fr, as h2g_create_proof */
  int advice_on_device;       /* advice is a device pointer, 16-byte aligned */
  const uint64_t* instance;   /* num_instance x n Fr, zero padded */
  const uint64_t* challenges; /* num_challenges x 4 (Montgomery); required iff the key has challenges */
  const uint8_t* seed;        /* 32 bytes; NULL = a fixed default */
  const int32_t* copies;      /* h2g_circuit.copies layout; NULL / 0 skips the copy check */
  uint32_t num_copies;
} h2g_check_inputs;
int h2g_check_witness(uint64_t pk, const h2g_check_inputs* in, h2g_check_failure* out, size_t cap, uint64_t* total);

/* ---- the prover's self-checks: refuse a proof that will not verify, and say why -----------
 * h2g_create_proof* accepts any advice; by default (H2G_SELFCHECK_OFF) a witness that breaks a
 * gate, a copy or a shuffle gives H2G_OK and bytes the verifier rejects.  Per key, like
 * h2g_pk_set_multiopen (an unknown mode: H2G_ERR_ARG):
 *   H2G_SELFCHECK_VERDICT    after its evaluations the prover forms the verifier's expected_h
 *       from the very scalars, challenges and instances of the proof (the code h2g_verify_proof
 *       runs) and compares it with h(x), the one condition of verify_proof that depends on the
 *       witness.  Equal: the proof is returned, byte for byte mode 0's.  Different: the call
 *       returns H2G_ERR_UNSATISFIED, writes no proof (*proof_len = 0) and leaves the key
 *       usable; h2g_last_self_check then says where, located on the run's own data:
 *         kinds 1 / 2  gates, as h2g_check_witness defines them, on the advice with the blinding
 *                      rows this proof drew and its own challenges
 *         kind 6       circuit's permutation product does not close: z_last[u] != 1, index =
 *                      the last column set, row = u.  Some copy constraint is broken; the copy
 *                      list is not part of the key, so h2g_check_witness with the list names it
 *         kind 4       shuffle `index`: its product does not close (row = H2G_CHECK_NO_ROW)
 *         kind 10      the identity fails and none of the above says where
 *       A wrong witness passes with probability about d / r (d the circuit's degree times n, r
 *       the 254-bit field order): x is drawn after the commitments.
 *   H2G_SELFCHECK_ARGUMENTS  the above, and the reference's `sanity-checks` assertions while
 *       each argument is built (device kernels behind the kernel that made the argument; no RNG
 *       draw, nothing written to the transcript: a valid witness gives mode 0's bytes):
 *         kind 9  the advice as handed in is nonzero at row >= u of unblinded column `index`
 *                 (prover.rs:418-421; a blinded column's rows there are overwritten and are
 *                 not asked)                                         -> H2G_ERR_UNSATISFIED
 *         kind 8  lookup `index`: permuted pair, A'[row] is neither S'[row] nor A'[row - 1]
 *                 (lookup/prover.rs:475-488)                         -> H2G_ERR_STATE
 *         kind 6  column set `index`'s permutation product (ours; the reference asserts nothing
 *                 here): at row < u the recurrence against sigma and delta^c omega^row fails, or
 *                 at row 0 the set does not start at the previous set's z[u] (set 0: at one)
 *                                                                    -> H2G_ERR_STATE
 *         kind 7  product `index` (a lookup's, or num_lookups + a shuffle's): z[0] != 1 or the
 *                 recurrence from row to row + 1 fails (lookup/prover.rs:269-305,
 *                 shuffle/prover.rs:176-191)                         -> H2G_ERR_STATE
 *                 row = u: a lookup's z[u] != 1                      -> H2G_ERR_UNSATISFIED
 *       H2G_ERR_STATE: no witness can cause it; the message names the library.
 * A lookup input missing from its table stays H2G_ERR_ARG in every mode.  With a shard or SPMD
 * transport installed and mode != 0, create_proof* returns H2G_ERR_STATE before any work.
 * h2g_last_self_check: the records of the last h2g_create_proof* in this process (library state
 * under the library's lock, as h2g_last_challenges is: callers that prove from several threads
 * read it before the next proof starts; none after a proof that was
 * returned or failed for another reason), sorted by (circuit, kind, index, row); `reserved`
 * carries the circuit's index in the proof (0 from h2g_check_witness).  *total is exact; the
 * library keeps at most 4096 records per circuit. */
enum { H2G_SELFCHECK_OFF = 0, H2G_SELFCHECK_VERDICT = 1, H2G_SELFCHECK_ARGUMENTS = 2 };
enum {
  H2G_CHECK_PERMUTATION = 6,  /* set `index`'s grand product: closing value (row = u), recurrence (row < u) */
  H2G_CHECK_PRODUCT = 7,      /* lookup / shuffle product `index` at `row` */
  H2G_CHECK_PERMUTED_PAIR = 8,/* lookup `index`: the permuted pair at `row` */
  H2G_CHECK_UNUSABLE_ROW = 9, /* unblinded advice column `index` is nonzero at unusable row `row` */
  H2G_CHECK_IDENTITY = 10     /* the vanishing identity fails at x; nothing located */
};
int h2g_pk_set_self_check(uint64_t pk, int mode);
int h2g_last_self_check(h2g_check_failure* out, size_t cap, uint64_t* total);
/* test seams (tests/test_selfcheck_kernels_gpu.py): the product and permuted-pair kernels on device
 * arrays of any n >= 2 (z: n elements, the others u; 1 <= u < n), max_blocks > 0 caps the grid.
 * d_num_b == d_den_b == NULL: the one-factor (shuffle) form, z[i+1] (gamma + den_a[i]) = z[i]
 * (gamma + num_a[i]).  Records {kind, 0, row, 0} sorted by row, min(cap, failures) of them. */
int h2g_debug_selfcheck_product_dev(const void* d_z, const void* d_num_a, const void* d_num_b, const void* d_den_a,
                                    const void* d_den_b, const uint64_t beta[4], const uint64_t gamma[4], uint64_t n,
                                    uint64_t u, int max_blocks, h2g_check_failure* out, size_t cap, uint64_t* total);
int h2g_debug_selfcheck_permuted_dev(const void* d_a, const void* d_s, uint64_t u, int max_blocks,
                                     h2g_check_failure* out, size_t cap, uint64_t* total);
/* ... and the permutation-product kernel on one column set of m columns (1 <= m <= 64; more than 8
 * go in several launches, as in the prover): d_values / d_sigmas are host arrays of m device
 * pointers (u elements each), d_z has u + 1, delta_pows is m x 4 (delta^c of each column),
 * first the value z[0] must have (NULL: one).  Records {6, 0, row, 0}. */
int h2g_debug_selfcheck_permutation_dev(const void* d_z, const uint64_t* first, const void* const* d_values,
                                        const void* const* d_sigmas, const uint64_t* delta_pows, int m,
                                        const uint64_t beta[4], const uint64_t gamma[4], const uint64_t omega[4],
                                        uint64_t u, h2g_check_failure* out, size_t cap, uint64_t* total);

/* ---- verify_proof (halo2_backend/src/plonk/verifier.rs:58-512) with the KZG multi-open
 * verifiers (poly/kzg/multiopen/{shplonk,gwc}/verifier.rs) and DualMSM::check
 * (poly/kzg/msm.rs:188-206), for hosts without the Rust crate and for batches.
 * VerifyingKey (plonk.rs:42-231): the constraint system plus the fixed and permutation
 * commitments, host memory only.  The constraint system comes from `circuit` as for
 * h2g_pk_read (circuit->fixed_values / ->copies unused).  h2g_vk_write's bytes are the leading
 * bytes of h2g_pk_write's in the same format; out == NULL returns the length. */
int h2g_vk_from_pk(uint64_t pk, uint64_t* vk);            /* computes the fixed/permutation commitments if the key has none yet */
int h2g_vk_read(const h2g_circuit* circuit, const uint8_t* buf, size_t len, int format, uint64_t* vk);  /* VerifyingKey::read, plonk.rs:73-129 */
int h2g_vk_write(uint64_t vk, int format, uint8_t* out, size_t cap, size_t* len);
int h2g_vk_free(uint64_t vk);
/* ParamsVerifierKZG: the three points a verifier needs (G1 generator g[0], g2, s_g2), no SRS on
 * the device; the params need their G2 points (h2g_params_setup / _read / _set_g2) */
typedef struct { uint64_t g1[8], g2[16], s_g2[16]; } h2g_verifier_params;
int h2g_params_verifier(uint64_t params, h2g_verifier_params* out);
typedef struct {
  const uint8_t* proof; size_t proof_len;
  uint32_t num_circuits;                 /* >= 1 */
  const uint64_t* const* instance;       /* [num_circuits]: the columns' values concatenated, instance_lens[c][i] Fr each (no padding to n) */
  const uint32_t* const* instance_lens;  /* [num_circuits][num_instance] */
} h2g_verify_item;
/* MALFORMED: what verify_proof answers with an Err before the pairing -- a proof of the wrong
 * length (the key, the circuit count and the multi-open scheme fix it), a point encoding with
 * x >= p or off the curve, the point at infinity, an evaluation >= r, an instance value >= r or
 * more instance values than usable rows.  REJECTED: well formed, the pairing equation fails. */
enum { H2G_VERIFY_OK = 1, H2G_VERIFY_REJECTED = 0, H2G_VERIFY_MALFORMED = -1 };
/* SingleStrategy (kzg/strategy.rs:146-186): one proof, one pairing check.  multiopen and
 * transcript take the codes of h2g_pk_set_multiopen / h2g_pk_set_transcript.  The points are
 * decompressed and the DualMSM's two sums evaluated on the device (the path of
 * h2g_verify_batch with one item and no random factor).  Returns H2G_OK with the answer in
 * *verdict; an error code only for bad arguments, unknown handles or device errors. */
int h2g_verify_proof(uint64_t vk, const h2g_verifier_params* vp, int multiopen, int transcript,
                     const h2g_verify_item* item, int32_t* verdict);
/* A batch: one verdict per proof, at about one pairing check for a batch without bad proofs.
 * All point encodings of all proofs are decompressed in one launch, every proof's transcript
 * and scalar assembly runs on the host, one segmented MSM gives each well-formed proof's
 * (L_i, R_i), and e(sum r_i L_i, s_g2) = e(sum r_i R_i, g2) is decided for random nonzero r_i.
 * This is AccumulatorStrategy's random linear combination (kzg/strategy.rs:126-137) with one
 * difference: the reference answers for the whole batch, this call for each proof -- a failing
 * set of more than one proof is halved and both halves are tested, a failing set of one is
 * REJECTED, so f bad proofs among B cost at most 1 + 2 f ceil(log2 B) pairing checks, and a
 * malformed proof costs none and does not touch the others.  An accepted set is sound up to
 * probability ~ 1 / r over the choice of the r_i.
 * rng: the source of the r_i (random_fr, or 64 bytes of fill_bytes per draw).  NULL draws them
 * from the operating system's generator, never from a fixed seed: THE r_i MUST BE
 * UNPREDICTABLE to whoever made the proofs -- with known r_i two invalid proofs can be built
 * whose errors cancel in the combination, and both would be accepted.  A seeded rng is for
 * tests.
 * verdicts[count]; stats (may be NULL): [0] pairing checks, [1] MSM terms of the per-proof
 * sums, [2] points decompressed, [3] host milliseconds (transcripts, scalar assembly and
 * pairings; rounded).  Shard and SPMD transports take no part. */
int h2g_verify_batch(uint64_t vk, const h2g_verifier_params* vp, int multiopen, int transcript,
                     const h2g_verify_item* items, size_t count, const h2g_rng* rng,
                     int32_t* verdicts, uint64_t stats[4]);
/* wall milliseconds of the last h2g_verify_proof / h2g_verify_batch: [0] host (transcripts,
 * scalar assembly, the r_i), [1] decompression (upload, kernel, copy back), [2] the segmented
 * MSMs (uploads, kernels, results), [3] pairing checks */
int h2g_verify_stages(double ms[4]);

/* ---- the polynomial-commitment layer on its own (halo2_backend/src/poly/{commitment,query}.rs,
 * poly/kzg/**, transcript.rs, arithmetic.rs): for a host that opens polynomials of its own over
 * the resident SRS -- an aggregation layer, a protocol of its own, a shim implementing the
 * reference's Prover / Verifier traits.  create_proof and verify_proof run the same SHPLONK and
 * GWC code (csrc/multiopen.cpp).
 *
 * Transcript objects: Blake2bWrite / Blake2bRead / Keccak256Write / Keccak256Read
 * (transcript.rs:291-463; Challenge255).  Host only, usable before h2g_init; `kind` takes the
 * codes of h2g_pk_set_transcript.  H2G_ERR_ARG is what the reference answers with an io::Error:
 * the identity as a point, a read past the end, an encoding with x >= p or off the curve, a
 * scalar >= r -- and a call in the wrong mode.  A failed call leaves the transcript as it was.
 * Points are affine Montgomery limbs (the ABI's G1Affine); the byte stream carries them compressed.
 * read_point decompresses on the host. */
int h2g_transcript_new_write(int kind, uint64_t* t);
int h2g_transcript_new_read(int kind, const uint8_t* proof, size_t len, uint64_t* t);  /* copies the bytes */
int h2g_transcript_common_point(uint64_t t, const uint64_t p[8]);    /* Transcript::common_point, either mode */
int h2g_transcript_common_scalar(uint64_t t, const uint64_t s[4]);
int h2g_transcript_write_point(uint64_t t, const uint64_t p[8]);     /* TranscriptWrite, write mode only */
int h2g_transcript_write_scalar(uint64_t t, const uint64_t s[4]);
int h2g_transcript_read_point(uint64_t t, uint64_t p[8]);            /* TranscriptRead, read mode only */
int h2g_transcript_read_scalar(uint64_t t, uint64_t s[4]);
int h2g_transcript_squeeze(uint64_t t, uint64_t c[4]);               /* squeeze_challenge_scalar */
int h2g_transcript_bytes(uint64_t t, uint8_t* out, size_t cap, size_t* len);  /* finalize() of a write-mode transcript (it stays usable); out == NULL: the length */
int h2g_transcript_remaining(uint64_t t, size_t* bytes);             /* read mode: unread bytes */
int h2g_transcript_free(uint64_t t);

/* ParamsKZG::commit / commit_lagrange (poly/kzg/commitment.rs:305-317,354-366): the params'
 * fixed-base MSM over the prefix [0, len) of g / g_lagrange.  len above the params' n is
 * H2G_ERR_ARG (the reference's assert!), len == 0 the identity.  _dev: device scalars (16-byte
 * aligned) read on `stream`; the result comes to the host (synchronous, as h2g_msm_dev_host).
 * Like h2g_params_msm_dev these are plain local MSMs: an installed shard or SPMD transport
 * takes no part. */
int h2g_params_commit(uint64_t params, const uint64_t* coeffs, size_t len, uint64_t out[8], int* is_identity);
int h2g_params_commit_lagrange(uint64_t params, const uint64_t* evals, size_t len, uint64_t out[8], int* is_identity);
int h2g_params_commit_dev(uint64_t params, const void* d_coeffs, size_t len, uint64_t out[8], int* is_identity,
                          void* stream);
int h2g_params_commit_lagrange_dev(uint64_t params, const void* d_evals, size_t len, uint64_t out[8],
                                   int* is_identity, void* stream);
/* eval_polynomial (arithmetic.rs:57-82): out = sum_i poly[i] x^i (len == 0: zero).  Synchronous. */
int h2g_fr_eval(const uint64_t* poly, size_t len, const uint64_t x[4], uint64_t out[4]);
int h2g_fr_eval_dev(const void* d_poly, size_t len, const uint64_t x[4], uint64_t out[4], void* stream);
/* kate_division (arithmetic.rs:101-120): q = (a - a(b)) / (X - b), len - 1 coefficients; len == 1
 * writes nothing, len == 0 is H2G_ERR_ARG (the reference's subtraction overflows).  _dev:
 * asynchronous on `stream`, d_q must not overlap d_a, both 16-byte aligned. */
int h2g_kate_division(const uint64_t* a, size_t len, const uint64_t b[4], uint64_t* q);
int h2g_kate_division_dev(const void* d_a, size_t len, const uint64_t b[4], void* d_q, void* stream);
/* test seam: h2g_kate_division_dev with the kernel variant chosen by the caller.  tile_s = the
 * coefficients per thread, 8, 16, 32 or 64 (a tile is 256 tile_s quotients), 0 = by the size
 * rule as h2g_kate_division_dev (another value: H2G_ERR_ARG).  accumulate != 0: d_q holds
 * len - 1 reduced elements on entry and receives d_q + the quotient (SHPLONK's h(X) += ..). */
int h2g_debug_kate_division_dev(const void* d_a, size_t len, const uint64_t b[4], void* d_q, int accumulate,
                                int tile_s, void* stream);
/* the size rule itself: the tile_s h2g_kate_division_dev takes for `len` coefficients (len == 0:
 * H2G_ERR_ARG).  Host only: needs no h2g_init. */
int h2g_debug_kate_tile_s(size_t len, int* tile_s);

/* The multi-open argument.  A polynomial is in coefficient form, 1 <= len <= the params' n, in
 * host memory or (on_device) device memory, 16-byte aligned.  A query names its polynomial by
 * index -- the reference's pointer equality of ProverQuery -- and KZG ignores ProverQuery.blind,
 * so there is no such field.  The order of the queries is part of the argument (SHPLONK's
 * commitment and rotation-set order, GWC's point groups in first-appearance order) and is kept.
 * A repeated (polynomial, point) pair does what construct_intermediate_sets does: SHPLONK
 * (shplonk.rs:48-140) keeps one entry per pair (its sets are maps); GWC (gwc.rs:25-50) lists the
 * polynomial in the point's group once per occurrence, and so does the verifier.  (If a
 * verifier's caller gives one pair two different evaluations, SHPLONK uses the later one, as
 * h2g_verify_proof does; the reference's get_eval finds the first.) */
typedef struct { const uint64_t* coeffs; size_t len; int on_device; } h2g_poly_ref;
typedef struct { uint32_t poly; uint32_t reserved; uint64_t point[4]; } h2g_open_query;
/* Prover::create_proof (poly/commitment.rs:141-168): scheme 0 ProverSHPLONK
 * (shplonk/prover.rs:121-305), 1 ProverGWC (gwc/prover.rs:40-90).  Evaluates the queries on the
 * device, then squeezes from and writes into `transcript` (write mode) exactly what the
 * reference does: SHPLONK y, v, [h], u, [h']; GWC v, one [W] per point group.
 * A commitment that is the identity cannot enter the transcript (one constant polynomial opened
 * at one point: h(X) = 0): H2G_ERR_ARG as the reference's Err, and the transcript is left as
 * it was before the call.  H2G_ERR_ARG also for nqueries == 0, an index out of range, len == 0 or
 * len > n, a point >= r, a missing pointer, a misaligned device polynomial, a read-mode
 * transcript.  While a shard or SPMD transport is installed the call returns H2G_ERR_STATE (the
 * commitments' MSMs would be cut into the transport's slabs).  Scratch (4 n Fr and the GWC
 * witnesses) is kept with the params. */
int h2g_multiopen_prove(uint64_t params, int scheme, uint64_t transcript, const h2g_poly_ref* polys, size_t npolys,
                        const h2g_open_query* queries, size_t nqueries);
typedef struct { uint32_t commitment; uint32_t reserved; uint64_t point[4]; uint64_t eval[4]; } h2g_verify_query;
/* Verifier::verify_proof (poly/commitment.rs:171-193; shplonk/verifier.rs:45-140,
 * gwc/verifier.rs:42-123) + DualMSM::check (kzg/msm.rs:188-206): `commitments` are
 * ncommitments x 8 u64 affine points (VerifierQuery::new_commitment; MSM-valued commitments are
 * not offered), the argument's points are read from `transcript` (read mode).
 * *verdict: H2G_VERIFY_OK / _REJECTED / _MALFORMED (a point of the argument that does not
 * decode or is the identity, or the bytes end).  lr (may be NULL; written for OK and REJECTED):
 * the DualMSM's (left, right), affine, for a host that defers or aggregates the pairing: the
 * proof holds iff e(left, s_g2) = e(right, g2).  H2G_ERR_ARG for bad arguments as above, a
 * commitment off the curve, a point or evaluation >= r. */
int h2g_multiopen_verify(const h2g_verifier_params* vp, int scheme, uint64_t transcript,
                         const uint64_t* commitments, size_t ncommitments,
                         const h2g_verify_query* queries, size_t nqueries, int32_t* verdict, uint64_t lr[16]);

/* ---- the pairing check on the device (csrc/pairing_dev.hip): every input's verdict in one
 * launch, for a failing batch and for a host that deferred the pairings of many
 * h2g_multiopen_verify calls.  Both G2 arguments are the params' fixed points, so the host
 * builds their Miller-loop lines once per (g2, s_g2) (kept with the device state, released by
 * h2g_shutdown) and the device does no G2 arithmetic.  The final exponentiation goes through
 * powers of u and raises to m (p^12 - 1) / r with m = 2u (6u^2 + 3u + 1), u = 0x44e992b44a6909f1;
 * gcd(m, r) = 1, so "== 1" decides what the exact exponent decides.
 * ok[i] = 1 iff e(left_i, s_g2) == e(right_i, g2); lr = count x 16 u64 (left[8], right[8],
 * affine Montgomery, identity = zeros): the layout h2g_multiopen_verify writes.  A pair with
 * the identity as its G1 point contributes 1, as on the host.
 * The host entry validates vp (a G2 point outside the r-torsion is H2G_ERR_ARG) and every
 * coordinate (below p, on the curve or the identity; H2G_ERR_ARG names the index and leaves ok
 * untouched), copies in and out and returns when ok is ready; count == 0 is H2G_OK, count
 * above 2^24 H2G_ERR_ARG.  One launch lasts about as long as one check's dependent chain
 * (~6.6 ms on an MI355X) up to a few thousand checks. */
int h2g_pairing_check_batch(const h2g_verifier_params* vp, const uint64_t* lr, size_t count, int32_t* ok);
/* d_lr / d_ok (count x int32) in device memory, 16-byte aligned; asynchronous on `stream`
 * (NULL: the library's).  The points are not validated: an input off the curve gets an
 * unspecified verdict, never a fault.  d_lr is only read. */
int h2g_pairing_check_batch_dev(const h2g_verifier_params* vp, const void* d_lr, size_t count,
                                void* d_ok /* count x int32 */, void* stream);
/* how h2g_verify_batch resolves a failing batch: 0 bisection (default, as before),
 * 1 one device launch of per-proof checks over the resident (L_i, R_i): the combined check runs
 * as in mode 0, and if it fails every well-formed proof gets the verdict h2g_verify_proof
 * would give (these checks carry no random factor); stats[0] is then 1 + the number of
 * well-formed proofs, whatever the number of bad ones.  Process-wide.  Another mode is
 * H2G_ERR_ARG. */
int h2g_verify_set_isolation(int mode);
/* test seam: the values behind the verdicts, 48 u64 each (6 Fq2 coefficients of 1, w, .., w^5,
 * Montgomery form): miller = f_{s_g2}(left) f_{g2}(-right), gt = its final value (the exact
 * final exponentiation's, raised to m); either output may be NULL */
int h2g_debug_pairing_values(const h2g_verifier_params* vp, const uint64_t* lr, size_t count,
                             uint64_t* miller, uint64_t* gt);

/* wall milliseconds of the stages of the last h2g_create_proof (names: h2g_prover_stage_name).
 * Stages end when their work is queued, unless h2g_prover_stage_sync(1) is set: then each
 * stage boundary synchronises the prover stream and the times are GPU completion times
 * (diagnostics only -- it serialises the pipeline) */
int h2g_prover_stage_sync(int on);
int h2g_prover_stages(double* ms, int max, int* count);
const char* h2g_prover_stage_name(int i);

/* ---- one proof across several GPUs: MSM point slabs ------------
 * Every commitment MSM of create_proof (the MsmAccel::msm call sites of SURVEY 8a-1)
 * is split into `world` contiguous point slabs [P r / world, P (r + 1) / world) (P = 2^k
 * of the params, clipped to the MSM length n); rank 0 (the
 * prover) computes slab 0 and the transport hands slabs 1.. to the peer ranks, each of
 * which holds the same SRS (h2g_params_setup / _create) and answers with the affine
 * partial sum of its slab (h2g_params_msm_dev).  Rank 0 adds the partials (the group sum
 * is exact, so the proof bytes do not depend on `world`).  The transport is the host's
 * (one process per GPU over RCCL in yet-another-halo2-fork_amd/h2g_dist.py).
 *   launch : called once per MSM, in transcript order, after the scalars (n Fr,
 *            device pointer, valid until the matching collect) are complete;
 *            base_set 0 = params.g (commit), 1 = params.g_lagrange (commit_lagrange),
 *            2 = the prefix sums P_i = L_0 + ... + L_i of g_lagrange (a lookup's permuted
 *            columns, committed as sum_i (a_i - a_{i+1}) P_i: the same point, from
 *            scalars that vanish inside the columns' runs of equal values)
 *   collect: the world - 1 partials of MSM `seq` (8 u64 affine each, is_identity flags)
 * Both return 0 on success; nonzero fails the proof with H2G_ERR_STATE. */
typedef struct {
  void* ctx;
  int32_t world;
  int (*launch)(void* ctx, uint64_t seq, int32_t base_set, uint64_t n, const void* d_scalars);
  int (*collect)(void* ctx, uint64_t seq, uint64_t* partials, int32_t* is_identity);
} h2g_shard_transport;
/* install (world >= 2) or remove (NULL or world <= 1) the transport of h2g_create_proof */
int h2g_set_shard_transport(const h2g_shard_transport* t);
/* this rank's slab [lo, hi) of the params' points: builds fixed-base windows sized for
 * the slab (used by h2g_params_msm_dev and, on rank 0, by create_proof's own slab);
 * lo == hi removes them */
int h2g_params_set_slab(uint64_t params, uint64_t lo, uint64_t hi);
/* peer side: MSM of n device scalars against params' base set [offset, offset + n) */
int h2g_params_msm_dev(uint64_t params, int32_t base_set, uint64_t offset, uint64_t n, const void* d_scalars,
                       uint64_t out_affine[8], int32_t* out_is_identity);
/* device bytes the params hold in fixed-base windows: out[0] g and g_lagrange (full), out[1]
 * their slab windows, out[2] the prefix-summed Lagrange basis's full windows (built for a
 * key with lookups, or on a set-2 MSM outside the slab), out[3] its slab windows (built on
 * the first set-2 MSM inside the slab) -- a serving peer's footprint, observable */
int h2g_params_table_bytes(uint64_t params, uint64_t out[4]);
/* synchronous device-to-device copy (staging slabs for the transport) */
int h2g_memcpy_dtod(void* d_dst, const void* d_src, size_t bytes);

/* ---- the same sharding with the library's own RCCL transport (xGMI), no host callbacks:
 * a Rust (or any) host binds these five calls and shards create_proof's MSMs natively.
 * One process per GPU, each after h2g_init on its own device and with the same params:
 *   rank 0:  h2g_comm_unique_id(id) -> the host sends the 256 bytes to every rank
 *   all:     h2g_comm_init(id, world, rank)          (ncclCommInitRank x 2: slabs, partials)
 *   rank 0:  h2g_comm_install(params)  -> create_proof shards every commitment MSM
 *            ... h2g_create_proof* ...  -> h2g_comm_stop() ends the peers' sessions
 *   ranks 1..: h2g_comm_serve(params, &served)     (returns when rank 0 stops)
 *   all:     h2g_comm_destroy()
 * Slab r = points [P r / world, P (r + 1) / world) of the params' P, as for
 * h2g_shard_transport; rank 0 stages the peers' scalars with one device copy, sends them
 * over one communicator and receives the 64-B partials over the other, so later MSMs'
 * slabs stream while the peers compute.  The proof bytes do not depend on `world`. */
int h2g_comm_unique_id(uint8_t id[256]);
int h2g_comm_init(const uint8_t id[256], int world, int rank);
/* deadline (seconds; <= 0: none; default 300) of every wait on the library's RCCL
 * communicators: their non-blocking setup in h2g_comm_init, each call's enqueue and each
 * collective's completion.  Past it -- or on an RCCL error -- the communicators are aborted
 * (ncclCommAbort) and the call fails with H2G_ERR_DEVICE, so a run that would hang inside
 * RCCL returns and the caller can fall back to another transport (bench.py).  The peers'
 * wait for rank 0's next slab request (h2g_comm_serve) has its own deadline, below. */
int h2g_comm_set_timeout(double seconds);
/* shard mode: a serving peer's longest wait (seconds; <= 0: none, the default) for rank 0's
 * next request header in h2g_comm_serve.  Rank 0 that aborts its communicators (a timed-out
 * wait) or dies need not surface as an RCCL error on the peer; past this deadline the peer
 * aborts its own and h2g_comm_serve fails with H2G_ERR_DEVICE instead of waiting forever.
 * Rank 0 renews the peers' deadline with h2g_comm_keepalive while it idles between proofs
 * (a header the serve loop only counts as a sign of life). */
int h2g_comm_set_serve_timeout(double seconds);
int h2g_comm_keepalive(void);
int h2g_comm_install(uint64_t params);
int h2g_comm_serve(uint64_t params, uint64_t* served);
int h2g_comm_stop(void);
int h2g_comm_destroy(void);
/* the communicator as RCCL reports it (ncclCommCount / ncclCommUserRank); 0 / -1 without one */
int h2g_comm_info(int32_t* rccl_count, int32_t* rccl_rank);

/* ---- one proof across several GPUs, SPMD: every rank runs the same create_proof (same
 * key, witness, instances and RNG stream -- a seed, or draws the host replicates -- hence
 * the same transcript).  Rank r computes point slab r ([P r / world, P (r + 1) / world),
 * h2g_params_set_slab) of every commitment MSM from its own copy of the scalars, and the
 * 64-B partials are all-gathered and summed in rank order, so every rank writes the same
 * proof bytes as one GPU would and no scalars cross the links.
 *   allgather: in = this rank's H2G_SPMD_WORDS words: its partial (8 u64 affine limbs,
 *              then 1 if the identity) and 4 words of consistency digest (a Blake2b of
 *              the transcript state, of every RNG draw so far and of the advice columns'
 *              values at a fixed point, each rank evaluating its whole copy of every
 *              column once per advice phase); out = world x H2G_SPMD_WORDS u64 in rank
 *              order; 0 on success.  Every rank compares the digests and fails the proof
 *              (H2G_ERR_STATE) if any rank's differ: ranks fed different witnesses,
 *              instances or RNG draws would otherwise sum slabs of different polynomials
 *              into one invalid proof without an error (the commitments and evaluations
 *              are sums of the ranks' slabs, so they alone cannot reveal it). */
#define H2G_SPMD_WORDS 13
/*
 * The host transport (callbacks) or the library's RCCL all-gather (h2g_comm_spmd_install,
 * after h2g_comm_init on every rank).  Installing one sharding mode removes the other. */
typedef struct {
  void* ctx;
  int32_t world;
  int32_t rank;
  int (*allgather)(void* ctx, uint64_t seq, const uint64_t in[9], uint64_t* out);
  /* optional -- NULL replicates the extended-domain work on every rank.  Otherwise the
   * 2^e sub-cosets of the extended domain (e = extended_k - k; row t + 2^e m is point
   * zeta w_ext^t w^m) are divided over the ranks: rank r computes the sub-cosets
   * t = r, r + world, ... of every column and h(X) on those rows, and each sub-coset's
   * h evaluations (n Fr, device memory) are broadcast from their owner t mod world:
   * bcast(ctx, d_buf, bytes, root) in place, complete on return */
  int (*bcast)(void* ctx, void* d_buf, size_t bytes, int root);
  /* optional -- NULL replicates the multi-open tail.  Otherwise the evaluations and the
   * SHPLONK multi-open (poly/kzg/multiopen/shplonk/prover.rs:121-305) run on coefficient
   * slabs: rank r evaluates, combines and divides only coefficients [P r / world,
   * P (r + 1) / world) of each polynomial -- the points its MSM slabs cover -- and the
   * few scalars that join the slabs (partial evaluations, the kate divisions' carries
   * between slabs) are all-gathered: allgather_host(ctx, in, bytes, out) with `bytes`
   * host bytes from this rank, out = world x bytes in rank order, complete on return */
  int (*allgather_host)(void* ctx, const void* in, size_t bytes, void* out);
  /* optional, with bcast and allgather_host -- h(X) reaches the ranks as coefficient
   * slabs instead of broadcast evaluations: the owner of sub-coset t interpolates its h
   * evaluations (an n-point inverse NTT instead of everyone's 2^e n-point one) and every
   * rank receives slab r of each sub-coset's folded coefficients, from which it forms
   * its slab of the h pieces (vanishing/prover.rs:102-155).  exchange(ctx, d_send,
   * send_bytes, d_recv, recv_bytes): device buffers, all-to-all with per-peer byte counts
   * (world entries each; peer p's data contiguous, in peer order; the rank's own entry
   * is a local copy), complete on return */
  int (*exchange)(void* ctx, const void* d_send, const size_t* send_bytes, void* d_recv, const size_t* recv_bytes);
} h2g_spmd_transport;
/* install (world >= 2) or remove (NULL or world <= 1); either removes the overlapped
 * exchange below */
int h2g_set_spmd_transport(const h2g_spmd_transport* t);
/* optional, with exchange: the column-ownership exchanges (h2g_spmd_set_column_owners)
 * overlap the stages after them instead of draining the stream.  post(ctx, d_send,
 * send_bytes, d_recv, recv_bytes, stream, done) queues the same all-to-all as exchange()
 * behind the work queued on `stream` (a hipStream_t) so far and returns without waiting for
 * the transfer; `done` (a hipEvent_t the library owns) is recorded once the received bytes
 * are in place.  wait(ctx, done) returns once `done` has been recorded and the transfer has
 * finished, 0 on success (a transport with a deadline fails it there).  The prover posts a
 * stage's exchange right after its sub-cosets are packed and waits for all of them after
 * the vanishing commitments, before h(X) reads them; every rank posts in the same order.
 * ctx is the transport's.  NULL post: every exchange completes on return. */
typedef int (*h2g_spmd_exchange_post)(void* ctx, const void* d_send, const size_t* send_bytes, void* d_recv,
                                      const size_t* recv_bytes, void* stream, void* done);
typedef int (*h2g_spmd_exchange_wait)(void* ctx, void* done);
int h2g_set_spmd_exchange_async(h2g_spmd_exchange_post post, h2g_spmd_exchange_wait wait);
/* helpers for host transports of the overlapped exchange (with h2g_event_record):
 * hipEventSynchronize(done); and, for the one-GPU SPMD emulation (tools/spmd_emulate.py),
 * `done` recorded `us` microseconds of device time after the work queued on `stream` so
 * far (a one-thread wait kernel on a side stream stands for a modelled transfer) */
int h2g_event_wait(void* done);
int h2g_debug_link_delay(void* stream, void* done, double us);
/* SPMD slab partition (optional): rank r's slab -- of every commitment MSM and of the
 * multi-open tail's coefficients -- is [P S_r / S, P S_{r+1} / S) with S_r = weights[0] +
 * ... + weights[r - 1] and S their total, instead of [P r / world, P (r + 1) / world).
 * Every rank must pass the same weights, and its h2g_params_set_slab the same slab.  The
 * ranks that own extended-domain sub-cosets carry that extra work; smaller slabs balance
 * them against the others.  NULL (or world <= 1) restores the uniform partition. */
int h2g_spmd_set_weights(const uint32_t* weights, int world);
/* SPMD column ownership of wide stages (on by default; used with bcast, allgather_host and
 * exchange installed): an advice phase, the lookups' permuted columns or their products
 * with as many columns as ranks or more (a multiple of the ranks, or 4x them) go to the
 * ranks whole, column i to rank i mod world -- the owner commits it (its rank's partial is
 * the whole commitment, the others' the identity), forms its coefficients and its
 * sub-cosets, and one exchange per stage hands every sub-coset owner its sub-cosets and
 * every rank its coefficient slab; a lookup's sort, match and product run on its owner
 * only.  Stages with fewer columns keep the point slabs.  Applies from 4 ranks up: at 2
 * the exchange puts a quarter of the extended-domain data on the one link between the
 * ranks (more time than the transforms it saves).  0 turns it off. */
int h2g_spmd_set_column_owners(int on);
/* time inside the SPMD transport since the last reset, per collective kind k (0 the MSM
 * partials' all-gathers, 1 the host all-gathers, 2 the exchanges, 3 the broadcasts):
 * out[3k] milliseconds (host wall clock around the call), out[3k + 1] calls, out[3k + 2]
 * bytes sent + received; reset != 0 zeroes the counters after reading */
int h2g_spmd_stats(double* out, int max, int reset);
/* split_subcosets: 1 divides the extended domain's sub-cosets over the ranks (bcast over
 * the communicator), 0 replicates that work; the multi-open tail always runs on
 * coefficient slabs (allgather_host over the communicator) */
int h2g_comm_spmd_install(int split_subcosets);
/* SPMD over the library's communicators: 1 posts the column-ownership exchanges on the
 * second communicator's stream so they overlap the stages after them (the prover waits for
 * them before h(X)); 0 (the default) keeps them blocking on the first.  Read at
 * h2g_comm_spmd_install.  Both produce the same proof bytes. */
int h2g_comm_set_exchange_overlap(int on);
int h2g_comm_spmd_uninstall(void);

#ifdef __cplusplus
}
#endif

#endif /* H2G_H */
