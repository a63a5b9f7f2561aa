// prover_state.h -- what the prover's translation units share (internal: included only by
// params.cpp, commit.cpp, keygen.cpp, spmd.cpp, pk_serde.cpp, check_witness.cpp, verifier.cpp,
// g1_fft.hip, through multiopen.h by multiopen.cpp and kzg.cpp, through vanishing.h by the
// verifier and the self-check, and through proof_run.h by prover.cpp, prover_lookup.cpp and
// prover_selfcheck.cpp):
// the params / proving-key / workspace objects, the library's globals and the prototypes of
// the functions that cross files.  Each global is defined in the file that owns it.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <functional>
#include <set>
#include <thread>

#include <unistd.h>

#include "check.h"
#include "comm.h"
#include "comm_wait.h"
#include "poly.h"
#include "radix.h"
#include "g2.h"
#include "prover_kernels.h"
#include "runtime.h"
#include "srs.h"
#include "transcript.h"


namespace h2g {
namespace prv {
using namespace h2g::rt;

enum { COL_ADVICE = 0, COL_FIXED = 1, COL_INSTANCE = 2 };
enum { OP_CONST = 0, OP_QUERY = 1, OP_NEG = 2, OP_SUM = 3, OP_PROD = 4, OP_CHALLENGE = 5 };

struct Pool {  // owns device allocations of one params / pk object
  std::vector<void*> ptrs;
  uint64_t bytes = 0;  // requested, of the live allocations (h2g_pk_memory)
  hipError_t get(void** p, size_t nbytes) {
    hipError_t e = hipMalloc(p, nbytes ? nbytes : 16);
    if (e == hipSuccess) {
      ptrs.push_back(*p);
      bytes += nbytes ? nbytes : 16;
    }
    return e;
  }
  ~Pool() {
    for (void* p : ptrs) (void)hipFree(p);
  }
};
#define PALLOC(pool, ptr, count) HIPCHK((pool).get((void**)&(ptr), (size_t)(count) * sizeof(*(ptr))))

struct Params {
  int device = 0;
  uint32_t k = 0;
  size_t n = 0;
  G1Affine* g = nullptr;
  G1Affine* gl = nullptr;
  MsmFixedBase fg, fgl;  // fixed-base MSM windows of g and g_lagrange (commit / commit_lagrange)
  // this rank's point slab [slab_lo, slab_hi) when one proof spans several GPUs: windows
  // sized for the slab length (h2g_params_set_slab)
  size_t slab_lo = 0, slab_hi = 0;
  MsmFixedBase sg, sgl;
  // windows of the prefix-summed Lagrange basis (params_prefix): built with the first key
  // that has lookups (keygen, outside any timed proof), for the whole basis (fgp) or -- once
  // a slab is set -- for the slab only (sgp), as sg / sgl are
  MsmFixedBase fgp, sgp;
  // the G2 half of ParamsKZG (g2, s_g2 = [s] g2; verifier side, serialised with the params)
  bool has_g2 = false;
  G2Affine g2, s_g2;
  Pool pool;
  // h2g_multiopen_prove's device scratch (kzg.cpp), made by the first standalone opening
  std::shared_ptr<void> kzg_ws;
  ~Params() {
    msm_fixed_base_free(&fg);
    msm_fixed_base_free(&fgl);
    msm_fixed_base_free(&sg);
    msm_fixed_base_free(&sgl);
    msm_fixed_base_free(&fgp);
    msm_fixed_base_free(&sgp);
  }
  // windows and table offset serving the base range [off, off + n) of set 0 (g) / 1
  // (g_lagrange) / 2 (the Lagrange prefix sums: the slab's windows once built, else full)
  const MsmFixedBase& tables(int set, size_t off, size_t n, size_t* table_off) const {
    if (sg.table && off >= slab_lo && off + n <= slab_hi && (set != 2 || sgp.table)) {
      *table_off = off - slab_lo;
      return set == 0 ? sg : (set == 1 ? sgl : sgp);
    }
    if (set == 2) {
      *table_off = off;
      return fgp;
    }
    *table_off = off;
    return set == 0 ? fg : fgl;
  }
};

int params_prefix(Params& p, hipStream_t st, size_t off = 0, size_t n = 0);  // params.cpp
int params_finish(Params& p, hipStream_t st);

struct Query {
  int type, index, rot;
  bool operator==(const Query& o) const { return type == o.type && index == o.index && rot == o.rot; }
};

// The constraint system as the host sees it: the shape that keygen derives from an h2g_circuit
// (degree, queries, blinding factors; circuit.rs:143-170,292-320, keygen.rs:191-260) and a
// copy of its expression graph.  The prover runs the compiled device program; the verifier
// (verifier.cpp) evaluates these nodes at one point.
struct CsHost {
  uint32_t k = 0;
  int A = 0, F = 0, I = 0, P = 0, NL = 0, NS = 0;
  int degree = 0, bf = 0, chunk_len = 0, nsets = 0, max_phase = 0;
  std::vector<Query> adv_q, fix_q, ins_q;
  std::vector<std::pair<int, int>> perm_cols;
  std::vector<uint8_t> adv_phase, ch_phase;
  Fr transcript_repr;
  std::vector<int32_t> nodes;  // 4 per node (op, a, b, c), children before parents
  std::vector<Fr> constants;
  std::vector<int32_t> gate_roots;
  std::vector<std::vector<int32_t>> lk_in, lk_tab, sh_in, sh_sh;  // per argument, expression roots
};
// keygen.cpp: validates the graph and fills `cs`; fails with H2G_ERR_ARG and keygen's messages
int cs_host_build(const h2g_circuit* c, CsHost* cs);

// Per-circuit workspace of create_proof (one per circuit of a proof over several
// circuits, grown on demand and reused across proofs): the advice / instance columns,
// permutation, lookup and shuffle polynomials, and the device pointer tables that
// evaluate_h and the expression compressions read for this circuit.
struct CircuitWs {
  Pool pool;
  std::vector<Fr*> adv, adv_poly, adv_coset, inst_val, inst_poly, inst_coset, z, z_lag, z_coset;
  std::vector<Fr*> lk_a, lk_s, lk_ap, lk_sp, lk_ap_poly, lk_sp_poly, lk_z, lk_z_poly, lk_zc, lk_apc, lk_spc;
  std::vector<Fr*> sh_z, sh_z_poly, sh_zc;
  const Fr** d_load_col = nullptr;      // extended-coset columns (evaluate_h)
  const Fr** d_load_col_lag = nullptr;  // Lagrange columns (lookup / shuffle compression)
  const Fr** d_z = nullptr;
  const Fr** d_perm_v = nullptr;
  EvalLookup* d_lookups = nullptr;
  EvalShuffle* d_shuffles = nullptr;
  uint64_t* wit_pin = nullptr;  // advice staging of the witness source (num_advice x n Fr), pinned if possible
  bool wit_pin_pinned = false;
  // SPMD sub-coset split: per owned sub-coset i, the evaluate_h pointer tables with every
  // extended-coset column replaced by its sub-coset i (built for ProvingKey::sub_key)
  struct SubTables {
    const Fr** load_col = nullptr;
    const Fr** z = nullptr;
    const Fr** perm_v = nullptr;
    EvalLookup* lookups = nullptr;
    EvalShuffle* shuffles = nullptr;
  };
  std::vector<SubTables> sub;
  int64_t sub_key = -1;
  SubTables whole() const { return SubTables{d_load_col, d_z, d_perm_v, d_lookups, d_shuffles}; }  // the d_* tables
  ~CircuitWs() {
    if (!wit_pin) return;
    if (wit_pin_pinned) (void)hipHostFree(wit_pin);
    else std::free(wit_pin);
  }
};

struct ProvingKey {
  int device = 0;
  uint64_t params = 0;
  // the circuit's shape (k, the column and argument counts, queries, phases, degree, blinding
  // factors: read as pk.cs.X) and its expression graph, which h2g_vk_from_pk hands on
  CsHost cs;
  size_t n = 0, ext = 0;
  uint64_t rot_scale = 0;
  std::vector<uint8_t> unblinded;
  int num_consts = 0;  // challenge values live in consts[num_consts ..]
  // verifying-key commitments (fixed, permutation) of a key read from bytes; a key made
  // by keygen computes them when it is written (h2g_pk_write)
  std::vector<G1Affine> vk_fixed, vk_perm;
  // multi-open scheme of create_proof (the Prover type parameter, prover.rs:19-36):
  // 0 ProverSHPLONK, 1 ProverGWC; GWC witness polynomials, one per opening point
  int multiopen = 0;
  int transcript = 0;  // TRANSCRIPT_BLAKE2B / TRANSCRIPT_KECCAK256 (transcript.h)
  int self_check = 0;  // h2g_pk_set_self_check (H2G_SELFCHECK_*)
  std::vector<Fr*> gwc_q;
  static constexpr int LKC = 8;
  // the lookups' gathers and matches on LKS streams (lookup j's on stream j mod LKS), each
  // stream with its own scratch set (of the key's blinding-row count: allocated once, by the
  // first proof that uses them); set 0 is the key's own (ck_a2 ... rep_rows, lkb_scr)
  static constexpr int LKS = 4;
  Stream lk_st[LKS];
  Event lk_ev[LKS + 1];
  CanonKey *lks_a2[LKS] = {}, *lks_t2[LKS] = {}, *lks_left[LKS] = {};
  uint8_t* lks_rep[LKS] = {};
  uint32_t* lks_rows[LKS] = {};
  void* lks_scr[LKS] = {};
  // per-(circuit, lookup) device counters (LKC each) and table-row flags of the match, so
  // that one memset each clears every lookup's and one copy brings all counters back
  PinArr<uint32_t> lk_cnt;  // pinned per-(circuit, lookup) match counters (LKC each)
  DevArr<uint32_t> lk_counters;
  DevArr<uint8_t> lk_flags;
  DevArr<Fr> lk_diff;  // the lookup commitments' prefix-basis scalars (2 per lookup and circuit)
  // permute_expression_pair's sort, chosen per lookup from the value width lk_hb[l] (bit
  // length of the largest canonical value) seen by the previous proof: <= 64 bits: radix
  // sort of the values themselves; wider: radix sort of a 48-bit window of the top bits
  // with the row index, gather, and a sortedness check; 0: merge sort of the 256-bit
  // values.  lk_or_* (device / pinned, LKF per lookup): the limbs' OR and the check flag.
  static constexpr int LKF = 5;
  std::vector<int> lk_hb;
  DevArr<unsigned long long> lk_or_d;
  PinArr<unsigned long long> lk_or_h;
  // SPMD witness checksums of an advice phase (copy_columns), device / pinned, and the event
  // that their copy to the host has landed (spmd_witness_fold)
  DevArr<unsigned long long> wsum_d;
  PinArr<unsigned long long> wsum_h;
  Event wsum_ev;
  Event asg_ev;  // h2g_create_proof_assigned: the denominator list's upload has been read
  // pinned staging of a proof's small host-to-device uploads (blinding rows, seeds, staged
  // scalars; pk_upload): from pageable memory a hipMemcpyAsync costs 8-60 us of host time
  // (a staged copy), which left the GPU idle between the keccak-style circuit's 32 advice
  // columns; from pinned memory the copy is queued at once.  Re-armed per proof
  PinArr<uint8_t> up_h;
  size_t up_off = 0;
  Domain dom;
  Pool pool;
  // H2G_COSETS_RESIDENT: every column evaluate_h reads is held as its extended coset (the
  // *_coset arrays of the key and of each CircuitWs, l0 / l_last / l_active: 2^ek elements
  // each).  H2G_COSETS_STREAMED: each of those arrays is one n-element slot; evaluate_h runs
  // sub-coset by sub-coset (ProofRun::eval_h) and the slots are refilled from the coefficient
  // forms for every sub-coset (coeff_to_subcoset_batch).  Set before keygen_impl.
  int cosets = 0;
  // proving key (device)
  std::vector<Fr*> fixed_lag, fixed_poly, fixed_coset, sigma_lag, sigma_poly, sigma_coset;
  Fr *l0 = nullptr, *l_last = nullptr, *l_active = nullptr;
  // streamed only: coefficient forms of l_0, l_last and l_blind (the sum of the blinding
  // rows' Lagrange polynomials); on any set of points l_active = 1 - l_last - l_blind
  Fr *l0_poly = nullptr, *l_last_poly = nullptr, *l_blind_poly = nullptr;
  PowTable om, eo;
  int4* prog = nullptr;
  int prog_len = 0, n_slots = 0;
  int2 seg_gates = {0, 0};
  // one program segment per gate root (h2g_check_witness: seg_gates folds the gates into one
  // Horner chain, so a single gate's value is not available from it), host and device
  std::vector<int2> seg_gate;
  int2* d_seg_gate = nullptr;
  std::vector<int2> seg_lk_in, seg_lk_tab, seg_sh_in, seg_sh_sh;  // expression-list programs
  // lookup l's table expressions equal lookup lk_trep[l]'s (the first such; l itself when
  // none): the proof sorts that table once
  std::vector<int> lk_trep;
  Fr* consts = nullptr;
  int n_loads = 0;
  std::vector<Query> loads;  // the programs' load table (column, rotation)
  int* d_load_rot = nullptr;
  const Fr** d_sigma = nullptr;
  Fr *tmp_a = nullptr, *tmp_b = nullptr, *one = nullptr;
  CanonKey *ck_a2 = nullptr, *ck_t2 = nullptr, *ck_left = nullptr;
  uint8_t *rep_flag = nullptr, *left_flag = nullptr;
  uint32_t *rep_rows = nullptr, *counters = nullptr;
  // per-proof workspace (device), reused across proofs: per circuit, and shared
  std::vector<std::unique_ptr<CircuitWs>> cws;
  Fr *mod = nullptr, *pre = nullptr, *scr = nullptr, *random_poly = nullptr, *h_ext = nullptr, *h_coeff = nullptr;
  Fr *h_poly = nullptr, *nx = nullptr, *q1 = nullptr, *hx = nullptr, *lx = nullptr;
  Fr *small = nullptr, *last_z = nullptr;
  // the evaluation batches' requests, results and scratch (openings_and_evals, slab_carries)
  DevArr<EvalReq> d_reqs;
  DevArr<Fr> evals, eval_scr;
  // SPMD sub-coset split (h2g_spmd_transport.bcast): this rank's sub-cosets t = rank,
  // rank + world, ... < 2^e of the extended domain; the key's cosets cut to them (slot i
  // of each buffer = sub-coset sub_ts[i]), per-slot sigma tables, and the 2^e x n slots
  // the h evaluations are broadcast through
  int64_t sub_key = -1;  // (world * 65536 + rank) * 2 + pieces the cache holds
  std::vector<uint64_t> sub_ts;
  // more ranks than sub-cosets (world a multiple of 2^e, with the slab exchange): rank r
  // evaluates rows [sub_lo, sub_hi) of sub-coset r mod 2^e -- piece r / 2^e of world / 2^e
  // -- and holds its columns there with a halo of rotations [rot_lo, rot_hi]
  bool sub_pieces = false;
  uint64_t sub_lo = 0, sub_hi = 0;
  int rot_lo = -1, rot_hi = 1;
  DevArr<Fr> cs_scr;   // column ownership: the owned columns' 2^e sub-cosets
  DevArr<Fr> perm_lz;  // slab-wise grand products: z at each set's slab start
  std::vector<Fr*> sub_fixed, sub_sigma;
  Fr *sub_l0 = nullptr, *sub_ll = nullptr, *sub_la = nullptr;
  std::vector<const Fr**> d_sigma_sub;
  Fr* h_gather = nullptr;
  size_t scr_len = 0;  // of scr (allocated at keygen)
  // permute_expression_pair's batched sort: every lookup column's canonical values, keys
  // and row indices (ping-pong pairs), radix / compaction scratch
  DevArr<CanonKey> lkb_canon;
  DevArr<uint64_t> lkb_key[2];
  DevArr<uint32_t> lkb_idx[2];
  DevBuf lkb_scr;
  // SPMD coefficient slabs: per SHPLONK point a (slab + halo) combination buffer
  DevArr<Fr> slab_buf;
  // SPMD h(X) by slabs (h2g_spmd_transport.exchange): send / receive staging
  DevArr<Fr> x_send, x_recv;
  // SPMD column ownership: the pack / unpack copy lists (host lists live until the next
  // stage, after a stream synchronisation, so their asynchronous uploads have completed)
  DevArr<CopySeg> d_segs;
  std::vector<CopySeg> h_segs[2];
  // overlapped column-ownership exchanges (h2g_set_spmd_exchange_async), in posting order:
  // each its own send / receive staging (grow-only, reused by the same position in the
  // next proof), completion event and unpack list, live from its post until xp_flush
  struct XPending {
    DevArr<Fr> send, recv;
    Event done;
    std::vector<CopySeg> unpack;
    bool live = false;
  };
  std::vector<XPending> xp, xp_lost;  // xp_lost: abandoned by xp_drain, kept until the key goes
  size_t xp_used = 0;
  // a stage's blinding rows, uploaded in one copy (upload_rows_batch)
  DevArr<Fr> blind_d;
  // h2g_create_proof_assigned's scratch: the phase's numerators (num_advice x n, evaluated
  // in place and read as device advice) and its Rational cells' indices and denominators
  DevArr<Fr> asg_num, asg_den;
  DevArr<uint64_t> asg_idx;
  DevArr<uint32_t> d_seeds;  // the vanishing argument's chunk seeds (8 words each) and offsets
  DevArr<uint64_t> d_offsets;
  // the keystream position of the vanishing argument's seed draws in the last proof with
  // the seeded RNG (the draws before them depend on the circuit's shape only), and its
  // thread count: the next proof generates and commits the random polynomial early
  int64_t van_pos = -1;
  uint32_t van_T = 0;
  // the self-checks' record slots and counters, one set per circuit of a proof (grow-only,
  // allocated by the first checked proof)
  DevArr<uint4> sc_rec;
  DevArr<unsigned long long> sc_total;
  // h2g_check_witness's own buffers (grow-only, allocated by the first check): the record
  // buffer and counters, the blinding rows' generator inputs and values, the full sort's
  // keys / indices / scratch and its two sorted outputs, the copy list and column table
  struct CheckWs {
    DevArr<uint4> rec;
    unsigned long long* total = nullptr;  // [0] the failure count, [1..9) lookup_keys / lookup_gather masks
    uint32_t* sh_flags = nullptr;         // one per shuffle
    uint32_t* seeds = nullptr;
    uint64_t* offs = nullptr;
    Fr* blind = nullptr;
    CanonKey *canon = nullptr, *sorted_a = nullptr, *sorted_b = nullptr;
    uint64_t* key[2] = {nullptr, nullptr};
    uint32_t* idx[2] = {nullptr, nullptr};
    void* scr = nullptr;
    bool sort_ready = false;
    const Fr** cols = nullptr;
    DevArr<int32_t> copies;  // 6 words per copy constraint
    CopySeg* segs = nullptr;
    bool ready = false;
  } ck;
  // Destruction.  h2g_pk_free synchronises the device stream and drains the overlapped
  // exchanges first; the destructor waits for the lookup streams (a proof that failed
  // between their fork and join leaves them running) before any member goes.  The members
  // then go in reverse order of declaration: the buffers (ck ... lk_cnt) and `pool`
  // before the events and streams that were declared above them (lk_ev, lk_st), so no
  // stream is destroyed with work queued on a buffer, and no buffer freed under a stream
  // that was not waited for.  A key that keygen or a read gives up on goes the same way.
  ~ProvingKey() {
    for (Stream& s : lk_st)
      if (s) (void)hipStreamSynchronize(s);
  }
};

// VerifyingKey (plonk.rs:42-231) as the verifier needs it: the constraint system and the
// fixed / permutation commitments, all on the host -- no params, no device arrays
struct VerifyingKey {
  CsHost cs;
  std::vector<G1Affine> fixed, perm;
};
extern std::map<uint64_t, std::unique_ptr<VerifyingKey>> g_vks;   // verifier.cpp

extern std::map<uint64_t, std::unique_ptr<Params>> g_params;      // params.cpp
extern std::map<uint64_t, std::unique_ptr<ProvingKey>> g_pks;     // keygen.cpp

// the object behind a handle, or null
template <class M>
auto find_handle(M& m, uint64_t h) -> decltype(m.begin()->second.get()) {
  auto it = m.find(h);
  return it == m.end() ? nullptr : it->second.get();
}
inline Params* find_params(uint64_t h) { return find_handle(g_params, h); }
inline ProvingKey* find_pk(uint64_t h) { return find_handle(g_pks, h); }
inline VerifyingKey* find_vk(uint64_t h) { return find_handle(g_vks, h); }

inline Fr fr_neg_one() { return Fr::zero() - Fr::one(); }

// SRS_LAGRANGE_PREFIX: prefix sums of the Lagrange basis, P_i = L_0 + ... + L_i (params_prefix)
enum { SRS_G = 0, SRS_LAGRANGE = 1, SRS_LAGRANGE_PREFIX = 2 };
extern h2g_shard_transport g_shard;  // spmd.cpp, like every global below
extern uint64_t g_shard_seq;
extern h2g_spmd_transport g_spmd;
extern uint64_t g_spmd_seq;
// time, calls and bytes (sent + received) inside the transport, per collective kind
// (h2g_spmd_stats): 0 MSM all-gathers, 1 host all-gathers, 2 exchanges, 3 broadcasts
struct SpmdStats {
  double ms[4] = {};
  uint64_t calls[4] = {}, bytes[4] = {};
};
extern SpmdStats g_spmd_stats;
template <class F>
int spmd_timed(int kind, uint64_t bytes, F&& f) {
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = f();
  g_spmd_stats.ms[kind] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g_spmd_stats.calls[kind]++;
  g_spmd_stats.bytes[kind] += bytes;
  return rc;
}
// the running proof's transcript, RNG draws and witness, whose digest travels with every
// SPMD partial (H2G_SPMD_WORDS): ranks that diverged fail the proof instead of summing
// slabs of different polynomials.  The witness enters as a 64-bit checksum of every advice
// column, over the whole column on each rank, taken by the kernel that copies the column
// in (copy_columns; spmd_witness_fold): with the slabs summed, the commitments and
// evaluations alone would be the same on ranks fed different witnesses.  The checksums
// reach the host behind the stream and are folded in when the next collective needs the
// digest (spmd_witness_settle), so the check costs no synchronisation of its own.
struct SpmdCheck {
  const Transcript* tr = nullptr;
  const ProverRng* rng = nullptr;
  uint8_t wit[64] = {};
  const unsigned long long* pend = nullptr;  // pinned checksums still to fold (pend_n), ready at pend_ev
  int pend_n = 0;
  hipEvent_t pend_ev = nullptr;
};
extern SpmdCheck g_spmd_check;
struct SpmdCheckScope {
  SpmdCheckScope(const Transcript* tr, const ProverRng* rng) {
    g_spmd_check = SpmdCheck{};
    g_spmd_check.tr = tr;
    g_spmd_check.rng = rng;
  }
  ~SpmdCheckScope() { g_spmd_check = SpmdCheck{}; }
};

// SPMD column ownership of wide stages (h2g_spmd_set_column_owners; on by default)
extern bool g_spmd_colshard;
// ... from this world size up.  Ownership trades transform work for an all-to-all of the
// owned columns' sub-coset pieces: each rank sends (W - 1) / W of its 1 / W share of the
// extended-domain data, over W - 1 point-to-point xGMI links at once, i.e. ~D / W^2 per
// link for D bytes of cosets.  At W = 2 that is D / 4 on ONE link (keccak-style k = 18: D
// ~ 3 GB -> ~0.75 GB, ~12 ms at ~64 GB/s, against ~10 ms of transforms saved); at W = 4
// D / 16 and at W = 8 D / 64 (~50 MB per link, < 1 ms)
constexpr int kColshardMinWorld = 4;

extern std::vector<uint64_t> g_spmd_wprefix;

// Proving-key arrays taken from a serialised ProvingKey (h2g_pk_read, plonk.rs:311-359)
// instead of being computed: host pointers into the file buffer, raw Montgomery Fr
// (SerdeFormat::RawBytes layout = the device layout), or canonical Fr (Processed: each
// array is converted with from_repr on the device right after its upload, elements >= r
// counted into *bad).
struct PkImage {
  std::vector<const uint8_t*> fixed_lag, fixed_poly, fixed_coset, sigma_lag, sigma_poly, sigma_coset;
  const uint8_t *l0 = nullptr, *l_last = nullptr, *l_active = nullptr;
  bool canonical = false;
  uint32_t* bad = nullptr;  // device counter, Processed only
  // device counter of unreduced elements in the arrays a streamed key checks and drops (its
  // cosets, SerdeFormat::RawBytes); null: no such check
  uint32_t* bad_raw = nullptr;
  hipError_t upload(Fr* dst, const uint8_t* src, size_t cnt, hipStream_t st) const {
    hipError_t e = hipMemcpyAsync(dst, src, cnt * sizeof(Fr), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && canonical) e = fr_from_repr(dst, cnt, bad, st);
    return e;
  }
};

// ------------------------------------------------------------------ SPMD coefficient slabs
// With h2g_spmd_transport.allgather_host the evaluations and the SHPLONK multi-open run on
// coefficient slabs: rank r owns coefficients [lo, hi) of every length-n polynomial (the
// points of its MSM slabs, shard_lo) and computes one more (hi, the halo) where a kate
// division reads a[i + 1].  Partial evaluations and the divisions' carries between slabs
// are the only values that cross ranks (a few Fr per proof).
struct Slab {
  size_t lo = 0, hi = 0;  // owned coefficients
  size_t hi1 = 0;         // hi + 1 (the halo coefficient), clipped to n
};

// Synchronises a stream when it goes out of scope: declared after host staging buffers
// that asynchronous copies read, so that an early return cannot free them under a copy.
struct StreamSyncGuard {
  hipStream_t s;
  ~StreamSyncGuard() { (void)hipStreamSynchronize(s); }
};


// commit.cpp
size_t shard_lo(size_t P, size_t n, int world, int r);
int commit_launch(Device* d, const Params& prm, const Fr* scalars, size_t n, int set, hipStream_t st, MsmTicket* t);
int commit_collect(Device* d, MsmTicket* t, G1Affine* out);
int commit_collect_all(Device* d, MsmTicket* const* t, int nb, G1Affine* out);
int commit_batch_chunk(const Params& prm, size_t n, int set);
int commit_launch_batch(Device* d, const Params& prm, const Fr* const* scalars, int nb, size_t n, int set,
                        hipStream_t st, MsmTicket* t);
int commit_launch_owned(Device* d, const Params& prm, const Fr* const* scalars, const int* owner, int nb, size_t n,
                        int set, hipStream_t st, MsmTicket* t);
int commit(Device* d, const Params& prm, const Fr* scalars, size_t n, int set, G1Affine* out, hipStream_t st);

// keygen.cpp
int build_pow_table(Pool& pool, const Fr& w, int L, PowTable* t, hipStream_t st);
int circuit_ws_add(ProvingKey& pk);
int key_options_mode(const h2g_key_options* opts, const char* who, int* mode);
int keygen_impl(Device* d, Params& prm, const h2g_circuit* c, ProvingKey& pk, const PkImage* img);

// spmd.cpp
void spmd_digest(uint64_t out[4]);
bool spmd_subcosets();
Slab spmd_slab(size_t n, int r);
int spmd_allgather_fr(const std::vector<Fr>& mine, std::vector<Fr>* all);
int lincomb_range(Fr* out, size_t lo, size_t hi, LinTerms t, bool accumulate, hipStream_t st);
int sub_prepare(ProvingKey& pk, hipStream_t st, bool pieces);
int sub_ws_tables(const ProvingKey& pk, CircuitWs& w);
int ext_cosets(Device* d, const ProvingKey& pk, const Fr* const* src, Fr* const* dst, int count, hipStream_t st);
int h_by_slabs(Device* d, ProvingKey& pk, const Slab& sl, hipStream_t st);
int coef_exchange(ProvingKey& pk, const std::vector<Fr*>& cols, hipStream_t st);
int colshard_distribute(Device* d, ProvingKey& pk, const std::vector<const Fr*>& lag, const std::vector<Fr*>& poly,
                        const std::vector<Fr*>& coset, const std::vector<int>& owner, hipStream_t st);
int xp_flush(ProvingKey& pk, hipStream_t st);
void xp_drain(ProvingKey& pk);
int h_gather_pieces(ProvingKey& pk, hipStream_t st);
int gather_to_owners(ProvingKey& pk, const std::vector<Fr*>& cols, const std::vector<int>& owner, size_t P,
                     hipStream_t st);
int spmd_witness_prepare(ProvingKey& pk, int m, hipStream_t st);
int spmd_witness_fold(ProvingKey& pk, int m, hipStream_t st);

// pk_serde.cpp
bool g2_valid(const G2Affine& a);

// prover.cpp
hipError_t pk_upload(ProvingKey& pk, void* dst, const void* src, size_t bytes, hipStream_t st);
// a copy list in one launch: `segs` goes up into pk.d_segs (host list valid until st is synchronised)
int copy_list_run(ProvingKey& pk, const std::vector<CopySeg>& segs, hipStream_t st);

}  // namespace prv
}  // namespace h2g

#define NEED_DEV_P()                                                          \
  std::lock_guard<std::recursive_mutex> _lk(g_mu);                            \
  Device* d = cur();                                                          \
  if (!d) return fail(H2G_ERR_STATE, "h2g_init has not been called");         \
  HIPCHK(hipSetDevice(d->id));
