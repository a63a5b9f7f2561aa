// prover.cpp -- keygen (keygen.cpp) and create_proof on the device (BN254 / KZG / SHPLONK).
//
// Host orchestration of halo2_backend's prover, all polynomial data resident in HBM:
//   keygen_vk / keygen_pk          plonk/keygen.rs:43-190, circuit.rs:95-180,292-320
//   permutation Assembly/build_pk  plonk/permutation/keygen.rs:16-213
//   Prover::new_with_engine        plonk/prover.rs:174-305 (instances)
//   commit_phase                   plonk/prover.rs:309-494 (every advice phase, challenges after each)
//   create_proof                   plonk/prover.rs:512-899
//   permutation_commit/evaluate    plonk/permutation/prover.rs:50-333
//   vanishing commit/construct     plonk/vanishing/prover.rs:40-205
//   evaluate_h                     plonk/evaluation.rs:317-483
//   SHPLONK / GWC                  poly/kzg/multiopen/** -- multiopen.cpp, run over ProofRun::multiopen_ctx()
// Host work is the transcript, the prover RNG's few hundred draws, query bookkeeping
// and O(#queries^2) interpolation; every length-n or extended-length operation is a
// kernel (MSM, NTT, prover_kernels.hip, poly.hip).  MSM results come back to the host
// (they enter the transcript), which is the only per-step synchronisation.
#include "assigned.h"
#include "multiopen.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace {
std::vector<std::pair<const char*, double>> g_stages;
bool g_stage_sync = false;  // h2g_prover_stage_sync: stage times = GPU completion times
std::vector<Fr> g_last_challenges;  // the challenges of the last proof (h2g_last_challenges)

// ------------------------------------------------------------------ host field helpers
Fr rotate_omega(const Domain& d, const Fr& x, int rot) {
  return x * pow_u64(rot >= 0 ? d.omega : d.omega_inv, (uint64_t)(rot >= 0 ? rot : -rot));
}

// Debug aid: a build with -DH2G_DUMP_DIR='"<dir>"' writes named intermediates (raw Fr
// arrays) of create_proof to <dir>/p<pid>/<name>.bin, one directory per process (rank); no
// run-time switch in the shipped library
void dump(const char* name, const Fr* dptr, size_t count, hipStream_t st, bool host = false) {
#ifndef H2G_DUMP_DIR
  (void)name, (void)dptr, (void)count, (void)st, (void)host;
  return;
#else
  const std::string dir = std::string(H2G_DUMP_DIR) + "/p" + std::to_string((long)getpid());
  std::vector<Fr> h(count);
  if (host) std::memcpy(h.data(), dptr, count * sizeof(Fr));
  else {
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(h.data(), dptr, count * sizeof(Fr), hipMemcpyDeviceToHost);
  }
  const std::string path = dir + "/" + name + ".bin";
  if (FILE* f = std::fopen(path.c_str(), "wb")) {
    std::fwrite(h.data(), sizeof(Fr), count, f);
    std::fclose(f);
  }
#endif
}

// ------------------------------------------------------------------ create_proof
struct StageClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  hipStream_t st;
  bool sync_each;
  explicit StageClock(hipStream_t s, bool sync) : st(s), sync_each(sync) { g_stages.clear(); }
  void mark(const char* name) {
    if (sync_each) (void)hipStreamSynchronize(st);
    const auto t = std::chrono::steady_clock::now();
    g_stages.emplace_back(name, std::chrono::duration<double, std::milli>(t - t0).count());
    t0 = t;
  }
};

// the proof's upload staging (ProvingKey::up_h): armed behind a sync of the prover's
// stream, so no copy of the previous proof still reads it
int pk_upload_arm(ProvingKey& pk, hipStream_t st) {
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(pk.up_h.ensure(4u << 20));
  pk.up_off = 0;
  return H2G_OK;
}
// dst <- src (host, any) on st through the staging; past its end, the pageable copy
}  // namespace

namespace h2g {
namespace prv {
hipError_t pk_upload(ProvingKey& pk, void* dst, const void* src, size_t bytes, hipStream_t st) {
  const size_t a = (pk.up_off + 63) & ~(size_t)63;
  if (a + bytes <= pk.up_h.len) {
    std::memcpy(pk.up_h.p + a, src, bytes);
    pk.up_off = a + bytes;
    return hipMemcpyAsync(dst, pk.up_h.p + a, bytes, hipMemcpyHostToDevice, st);
  }
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
}
int copy_list_run(ProvingKey& pk, const std::vector<CopySeg>& segs, hipStream_t st) {
  if (segs.empty()) return H2G_OK;
  HIPCHK(pk.d_segs.ensure(segs.size()));
  uint64_t mx = 0;
  for (const CopySeg& g : segs) mx = std::max<uint64_t>(mx, g.len);
  HIPCHK(pk_upload(pk, pk.d_segs.p, segs.data(), segs.size() * sizeof(CopySeg), st));
  HIPCHK(copy_segments(pk.d_segs.p, (int)segs.size(), mx, st));
  return H2G_OK;
}
}  // namespace prv
}  // namespace h2g

namespace {

// several blocks of blinding rows in one upload and one copy launch: `host` (count Fr) lands
// in pk.blind_d.p (sized by the caller, before it built `segs`), which `segs` read from.  Every small host-to-device copy is a ~6-us blit
// on the stream; a keccak-style proof made ~80 of them, one per column and lookup side
int upload_rows_batch(ProvingKey& pk, const Fr* host, size_t count, const std::vector<CopySeg>& segs,
                      hipStream_t st) {
  if (segs.empty()) return H2G_OK;
  HIPCHK(pk_upload(pk, pk.blind_d.p, host, count * sizeof(Fr), st));
  return copy_list_run(pk, segs, st);
}


// create_proof's inputs (halo2_proofs/src/plonk/prover.rs:19-36): per circuit the witness
// and the instances, the RNG, and the vanishing argument's thread count
struct ProveIn {
  int nc = 1;                                     // circuits
  const uint64_t* const* advice = nullptr;        // [nc] num_advice x n Fr (host, or device)
  bool adv_dev = false;
  const h2g_witness_source* src1 = nullptr;       // one circuit's per-phase witness source
  const h2g_witness_source_multi* src = nullptr;  // per-circuit per-phase witness source
  const h2g_assigned_source* asg = nullptr;       // the same, as Assigned cells (h2g_create_proof_assigned)
  const uint64_t* const* instance = nullptr;      // [nc] num_instance x n Fr (zero padded)
  const uint32_t* const* inst_lens = nullptr;     // [nc] num_instance lengths
  ProverRng* rng = nullptr;
  uint32_t vthreads = 1;
};

// One proof in flight: what create_proof's stages hand to each other, declared in the order
// the stages first need it.  Destruction (the reverse) is part of the behaviour: a
// StreamSyncGuard stands after the host staging that asynchronous copies read, so the stream
// is drained before that staging is freed, and spmd_check, tr, xjoin and ring_guard end the
// proof in that order whatever its outcome -- do not reorder the members.  The stages are
// the methods declared last, each run once by prove_impl, in that order.
struct ProofRun {
  Device* const d;
  Params& prm;
  ProvingKey& pk;
  const ProveIn& in;
  std::vector<uint8_t>* const proof;
  const hipStream_t st = d->stream;
  const size_t n = pk.n, ext = pk.ext;
  const int bf = pk.cs.bf;
  const Domain& D = pk.dom;
  const int ncirc = in.nc;
  std::vector<CircuitWs*> W = std::vector<CircuitWs*>(ncirc);
  const int E_sub;    // 2^e sub-cosets; with `pieces`, every rank takes a row piece of one (both from
  const bool pieces;  // prove_impl, which needs them for sub_prepare before anything here exists)
  MsmRingGuard ring_guard{d};
  StageClock clk{st, g_stage_sync};
  // SPMD coefficient slabs for the multi-open tail (SHPLONK only; GWC stays replicated)
  const bool slabs = g_spmd.world > 1 && g_spmd.allgather_host != nullptr && pk.multiopen == 0;
  const Slab sl = slabs ? spmd_slab(n, g_spmd.rank) : Slab{0, n, n};
  // SPMD with more ranks than sub-cosets: a rank that owns none needs the circuit's
  // coefficient columns only on its slab (evaluations, SHPLONK) -- the owners, which need
  // them whole for their cosets, send it (coef_exchange) and it skips their iNTTs
  const bool h_slabs = spmd_subcosets() && slabs && g_spmd.exchange != nullptr;
  const bool coef_recv = h_slabs && pk.sub_ts.empty();
  const bool coef_send = h_slabs && !pieces && !pk.sub_ts.empty() && g_spmd.world > (1 << (pk.dom.ek - pk.dom.k));
  // column ownership of wide stages (colshard_distribute): under the full split, a stage of
  // M columns goes to the ranks whole when M is a multiple of the ranks or at least 4x them
  // (balanced); fewer columns keep point slabs
  const int Wsp = g_spmd.world;
  bool wide(int M) const {
    return h_slabs && g_spmd_colshard && Wsp >= kColshardMinWorld && M >= Wsp && (M % Wsp == 0 || M >= 4 * Wsp);
  }
  // a stage's coefficient forms and extended-domain columns: with row pieces every stage's
  // transforms have one owner per column (round-robin across the stages, tr_next), a wide
  // stage's are its columns' owners (own); otherwise every sub-coset owner transforms
  // every column (the others receive coefficient slabs at the end, coef_exchange)
  // (with row pieces the rotation starts after the sub-cosets' leaders, ranks 0 .. E - 1,
  // which interpolate their sub-coset's h: C3 at 8 ranks puts its 6 column transforms on
  // ranks 2 .. 7 instead of stacking two roles on ranks 0 and 1)
  int tr_next = pieces ? E_sub : 0;
  // the transform stream: xs_begin orders it after the prover stream's
  // work so far (the inputs), xs_end marks its last transform, and the prover stream waits
  // for that mark before evaluate_h -- and at the end of the proof whatever its outcome
  // (XformJoin), so that the next proof's uploads never overtake a transform still reading
  const bool xsplit;  // (prove_impl, which creates the stream)
  const hipStream_t xst = xsplit ? d->xstream : st;
  struct XformJoin {
    Device* d;
    hipStream_t st;
    bool pending = false;
    hipError_t join() {
      if (!pending) return hipSuccess;
      pending = false;
      return hipStreamWaitEvent(st, d->xev_done, 0);
    }
    ~XformJoin() { (void)join(); }
  };
  XformJoin xjoin{d, st};
  int xs_begin() {
    if (xst == st) return H2G_OK;
    HIPCHK(hipEventRecord(d->xev_in, st));
    HIPCHK(hipStreamWaitEvent(xst, d->xev_in, 0));
    return H2G_OK;
  }
  int xs_end() {
    if (xst == st) return H2G_OK;
    HIPCHK(hipEventRecord(d->xev_done, xst));
    xjoin.pending = true;
    return H2G_OK;
  }
  int xform(const std::vector<const Fr*>& lag, const std::vector<Fr*>& pol, const std::vector<Fr*>& cst,
            const std::vector<int>* own) {
    const int M = (int)lag.size();
    if (M == 0) return H2G_OK;
    if (own || pieces) {
      std::vector<int> o(M);
      for (int i = 0; i < M; i++) o[i] = own ? (*own)[i] : (tr_next + i) % Wsp;
      if (!own) tr_next += M;
      return colshard_distribute(d, pk, lag, pol, cst, o, st);
    }
    RCCHK(xs_begin());
    if (!coef_recv) RCCHK(lagrange_to_coeff_batch(d, D, lag.data(), pol.data(), M, xst));
    RCCHK(ext_cosets(d, pk, (const Fr* const*)pol.data(), cst.data(), M, xst));
    return xs_end();
  }
  // with row pieces the advice columns' transforms wait for the permutation stage: at the
  // advice commitments' all-gather every rank would otherwise wait for the ranks that
  // transform an advice column (their slab partials come late), and in the permutation
  // stage the ranks without a grand product's transform are idle -- run there, the advice
  // transforms overlap the products' (the owners are fixed here, in the same rotation)
  struct DeferredXform {
    std::vector<const Fr*> lag;
    std::vector<Fr*> pol, cst;
    std::vector<int> own;
  };
  std::vector<DeferredXform> deferred;
  // (the column transforms of the whole proof, an upper bound, against the ranks that are
  // not sub-coset leaders: C3 at 8 ranks has 3 advice + 3 grand products for 6 ranks; at 4
  // ranks two transforms would share a rank in the permutation stage, measured slower:
  // profiles/r05/emulation/defer_adv/)
  const int n_xf = ncirc * (pk.cs.A + pk.cs.nsets + 3 * pk.cs.NL + pk.cs.NS);
  const bool defer_adv = pieces && n_xf <= Wsp - E_sub;
  void xform_later(const std::vector<const Fr*>& lag, const std::vector<Fr*>& pol, const std::vector<Fr*>& cst) {
    DeferredXform x{lag, pol, cst, std::vector<int>(lag.size())};
    for (size_t i = 0; i < lag.size(); i++) x.own[i] = (int)((tr_next + (int)i) % Wsp);
    tr_next += (int)lag.size();
    deferred.push_back(std::move(x));
  }
  int run_deferred() {
    for (DeferredXform& x : deferred) RCCHK(colshard_distribute(d, pk, x.lag, x.pol, x.cst, x.own, st));
    deferred.clear();
    return H2G_OK;
  }
  ProverRng& rng = *in.rng;
  Transcript tr{proof, pk.transcript};
  SpmdCheckScope spmd_check{&tr, &rng};
  int write_point(const G1Affine& p) {
    if (!tr.write_point(p)) return fail(H2G_ERR_ARG, "cannot write points at infinity to the transcript");
    return H2G_OK;
  }
  // a stage's commitments: collected together (one SPMD all-gather), written in order
  int collect_write(const std::vector<MsmTicket*>& tks) {
    std::vector<G1Affine> cms(tks.size());
    RCCHK(commit_collect_all(d, tks.data(), (int)tks.size(), cms.data()));
    for (const G1Affine& cm : cms) RCCHK(write_point(cm));
    return H2G_OK;
  }
  // h2g_create_proof_assigned: circuit ci's phase-ph numerators (w.wit_pin) and its Rational
  // cells go up to the key's scratch and are evaluated there in place on the prover's stream
  // (assigned.hip); the phase then reads the scratch as device advice
  int assigned_convert(int ci, int ph, const std::vector<int>& cols, CircuitWs& w, const h2g_assigned_dens& dn) {
    const size_t cells = (size_t)pk.cs.A * n;
    const std::string at = "circuit " + std::to_string(ci) + " phase " + std::to_string(ph);
    if (dn.count && (!dn.index || !dn.den))
      return fail(H2G_ERR_ARG, "create_proof_assigned: null denominator list at " + at);
    bool inside = true;  // every entry in one of this phase's columns (the usual case: no copy)
    for (size_t j = 0; j < dn.count; j++) {
      const uint64_t c = dn.index[j];
      if (c >= cells)
        return fail(H2G_ERR_ARG, "create_proof_assigned: index[" + std::to_string(j) + "] = " + std::to_string(c) +
                                     " is not below num_advice * n at " + at);
      if (j && c <= dn.index[j - 1])
        return fail(H2G_ERR_ARG, "create_proof_assigned: index[" + std::to_string(j) +
                                     "] does not exceed the entry before it (the list must be strictly increasing) at " + at);
      inside = inside && pk.cs.adv_phase[c >> pk.cs.k] == ph;  // n = 2^k
    }
    const uint64_t* idx = dn.index;
    const uint64_t* den = dn.den;
    size_t m = dn.count;
    if (!inside) {
      asg_idx_h.clear();
      asg_den_h.clear();
      for (size_t j = 0; j < dn.count; j++)
        if (pk.cs.adv_phase[dn.index[j] >> pk.cs.k] == ph) {
          asg_idx_h.push_back(dn.index[j]);
          asg_den_h.push_back(fr_from_limbs(dn.den + 4 * j));
        }
      idx = asg_idx_h.data();
      den = reinterpret_cast<const uint64_t*>(asg_den_h.data());
      m = asg_idx_h.size();
    }
    HIPCHK(pk.asg_num.ensure(cells));  // sizes first, then pointers (DevArr)
    HIPCHK(pk.asg_idx.ensure(m));
    HIPCHK(pk.asg_den.ensure(m));
    if (m) HIPCHK(d->work.ensure(m * sizeof(Fr) + 32));
    for (int c : cols)
      HIPCHK(hipMemcpyAsync(pk.asg_num.p + n * c, w.wit_pin + 4 * n * c, n * sizeof(Fr), hipMemcpyHostToDevice, st));
    if (m == 0) return H2G_OK;
    HIPCHK(hipMemcpyAsync(pk.asg_idx.p, idx, m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pk.asg_den.p, den, m * sizeof(Fr), hipMemcpyHostToDevice, st));
    HIPCHK(pk.asg_ev.ensure());
    HIPCHK(hipEventRecord(pk.asg_ev, st));
    asg_pending = true;
    HIPCHK(assigned_to_fr(pk.asg_num.p, cells, pk.asg_idx.p, pk.asg_den.p, m, pk.asg_num.p, d->work.as<Fr>(), 0, st));
    return H2G_OK;
  }
  int rng_ok() { return rng.failed() ? fail(H2G_ERR_ARG, "create_proof: the caller's RNG failed") : H2G_OK; }

  const size_t unusable = n - (size_t)(bf + 1);
  // host staging that device copies read asynchronously: lives until the proof returns
  // (every copy has completed by then: the final commitment is collected after it)
  std::vector<Fr> adv_blind = std::vector<Fr>((size_t)ncirc * pk.cs.A * (bf + 1));
  const bool from_src = in.src || in.src1 || in.asg;
  // h2g_create_proof_assigned: a list with cells outside its phase's columns, compacted to
  // those inside (staging that asynchronous copies read, like adv_blind), and whether the
  // last list's upload (the callback's memory until its next call) is still to be waited for
  std::vector<uint64_t> asg_idx_h;
  std::vector<Fr> asg_den_h;
  bool asg_pending = false;
  const int NCH = (int)pk.cs.ch_phase.size();
  std::vector<Fr> challenges = std::vector<Fr>(NCH);
  StreamSyncGuard adv_guard{st};
  // the vanishing argument's seeds and chunk offsets (staging read by async copies: lives
  // until the proof returns), its commitment's ticket, and whether it was launched early
  // (queued behind phase 0's advice MSMs; placed after the advice commitments instead it
  // measured slower, profiles/r03/s3/ab_early_vanishing)
  const std::vector<uint64_t> van_off = van_chunks();
  std::vector<uint32_t> van_seeds;
  StreamSyncGuard van_guard{st};  // destroyed before the staging above: the copies finish first
  MsmTicket van_tk;
  bool van_early = false;
  // it holds an MSM ring slot from phase 0 until y: only when every later stage's
  // outstanding commitments still fit beside it (advice phases, the permuted lookup
  // columns, the permutation / lookup / shuffle products)
  const bool early_van = rng.seeded() && pk.van_pos >= 0 &&
                         pk.van_T == (uint32_t)van_off.size() && g_spmd.world <= 1 && g_shard.world <= 1 &&
                         msm_ring_peak() + 1 <= MSM_RING;
  int launch_van_early() {
    // the vanishing argument's random polynomial does not depend on the witness: with the
    // seeded RNG its seeds are the keystream bytes at the position the last proof drew
    // them from, so it is generated and its commitment MSM launched early -- queued behind
    // phase 0's advice MSMs, it runs under the advice transforms and the lookup and
    // permutation products instead of between the product commitments and y; the
    // vanishing stage checks that the real draws equal these bytes (else it redoes both)
    van_seeds.assign(van_off.size() * 8, 0);
    rng.peek((uint64_t)pk.van_pos, reinterpret_cast<uint8_t*>(van_seeds.data()), van_seeds.size() * 4);
    HIPCHK(pk_upload(pk, pk.d_seeds.p, van_seeds.data(), van_seeds.size() * 4, st));
    HIPCHK(pk_upload(pk, pk.d_offsets.p, van_off.data(), van_off.size() * 8, st));
    HIPCHK(chacha_random_poly(pk.random_poly, n, pk.d_seeds.p, pk.d_offsets.p, (int)van_off.size(), st, sl.lo, sl.hi1));
    RCCHK(commit_launch(d, prm, pk.random_poly, n, SRS_G, st, &van_tk));
    van_early = true;
    return H2G_OK;
  }
  // advice columns distributed by their owners
  std::vector<char> adv_shard = std::vector<char>((size_t)ncirc * pk.cs.A, 0);
  // advice handed over in host memory: the first column's upload has nothing to overlap
  // (its MSM needs the whole column), so the random polynomial's commitment goes first and
  // runs under that upload; device-resident advice keeps it behind the advice commitments
  // and the advice transforms (first in both cases, or right behind the advice commitments
  // and ahead of the transforms: measured, rejected)
  const bool van_first = early_van && !in.adv_dev;

  // the challenges: each is assigned exactly once, by the stage that squeezes it (the only
  // writes to `ch`), and read by the later stages through these const names
  struct {
    Fr theta, beta, gamma, y, x;
  } ch;
  const Fr &theta = ch.theta, &beta = ch.beta, &gamma = ch.gamma, &y = ch.y, &x = ch.x;

  int compress(const CircuitWs& w, int2 seg, Fr* out) {
    CompressArgs ca;
    ca.prog = pk.prog;
    ca.seg = seg;
    ca.n_slots = pk.n_slots;
    ca.consts = pk.consts;
    ca.load_col = w.d_load_col_lag;
    ca.load_rot = pk.d_load_rot;
    ca.n = n;
    ca.theta = theta;
    ca.out = out;
    HIPCHK(compress_lagrange(ca, st));
    return H2G_OK;
  }
  const int NLT = ncirc * pk.cs.NL;  // (circuit, lookup) pairs, circuit-major: j = ci * NL + l
  bool lk_shard = false;  // the lookups went to their owners (A', S' and z distributed)
  std::vector<int> lk_owner_all = std::vector<int>(NLT, g_spmd.rank);
  const int NST = ncirc * pk.cs.nsets;  // (circuit, set), circuit-major
  std::vector<MsmTicket> perm_tk = std::vector<MsmTicket>(NST);
  // host staging of every set's / product's blinding rows: no host synchronisation per
  // set, the transforms of all sets go as batches after the loop
  std::vector<Fr> perm_blind = std::vector<Fr>((size_t)NST * bf),
                  prod_blind = std::vector<Fr>((size_t)ncirc * (pk.cs.NL + pk.cs.NS) * bf);
  StreamSyncGuard blind_guard{st};
  std::vector<Fr*> all_z_lag, all_z, all_z_coset;
  const Fr* col_vals(const CircuitWs& w, int c) const {
    const auto& pc = pk.cs.perm_cols[c];
    return pc.first == COL_ADVICE ? w.adv[pc.second]
                                  : (pc.first == COL_FIXED ? pk.fixed_lag[pc.second] : w.inst_val[pc.second]);
  }
  const int NSH = ncirc * pk.cs.NS;
  std::vector<MsmTicket> lkz_tk = std::vector<MsmTicket>(NLT), shz_tk = std::vector<MsmTicket>(NSH);
  // the evaluate_h arguments that depend neither on the domain (whole cosets or one
  // sub-coset) and the output nor on the sub-coset's slot: the caller fills those
  EvalHArgs eval_h_args(int ci) const {
    EvalHArgs a;
    a.prog = pk.prog;
    a.gates = pk.seg_gates;
    a.n_slots = pk.n_slots;
    a.theta = theta;
    a.nlookups = pk.cs.NL;
    a.nshuffles = pk.cs.NS;
    a.consts = pk.consts;
    a.query_rot = pk.d_load_rot;
    a.nsets = pk.cs.nsets;
    a.chunk_len = pk.cs.chunk_len;
    a.P = pk.cs.P;
    a.beta = beta;
    a.gamma = gamma;
    a.y = y;
    a.delta = fr_delta();
    a.last_rot = -(bf + 1);
    a.divide = ci + 1 == ncirc;
    return a;
  }

  // poly ids: per circuit ci (base ci * per_c): advice c, z s, lookup l (z, A', S'),
  // shuffle s; then fixed, sigma, h, random
  const int per_c = pk.cs.A + pk.cs.nsets + 3 * pk.cs.NL + pk.cs.NS;
  int id_adv(int ci) const { return ci * per_c; }
  int id_z(int ci) const { return ci * per_c + pk.cs.A; }
  int id_lk(int ci) const { return ci * per_c + pk.cs.A + pk.cs.nsets; }  // lookup l: z, A', S' at + 3 l
  int id_sh(int ci) const { return ci * per_c + pk.cs.A + pk.cs.nsets + 3 * pk.cs.NL; }
  std::vector<PolyRef> polys;
  std::vector<OpenQ> queries;
  // unique (poly, point) evaluations, one batched launch
  std::vector<OpenQ> ev_keys;
  std::vector<std::vector<int>> ev_of;  // per polynomial its ev_keys entries (a few points)
  int ev_index(int poly, const Fr& pt) {
    if ((size_t)poly >= ev_of.size()) ev_of.resize((size_t)poly + 1);
    for (int i : ev_of[poly])
      if (ev_keys[i].pt == pt) return i;
    ev_keys.push_back({poly, pt});
    ev_of[poly].push_back((int)ev_keys.size() - 1);
    return (int)ev_keys.size() - 1;
  }
  std::vector<Fr> evals;
  Fr ev(int poly, const Fr& pt) { return evals[ev_index(poly, pt)]; }

  // pure helpers of the initialisers above (no data members below this line)
  std::vector<uint64_t> van_chunks() const {
    std::vector<uint64_t> van_off;
    const uint64_t T = in.vthreads ? in.vthreads : 1;
    const uint64_t chunk = n / T, rem = n % T;
    for (uint64_t i = 0; i < rem && van_off.size() < T; i++) van_off.push_back(i * (chunk + 1));
    if (chunk)
      for (uint64_t o = rem * (chunk + 1); van_off.size() < T; o += chunk) van_off.push_back(o);
    return van_off;
  }
  int msm_ring_peak() const {
    int peak_msms = 0;
    for (int ph = 0; ph <= pk.cs.max_phase; ph++) {
      int a = 0;
      for (int c = 0; c < pk.cs.A; c++) a += pk.cs.adv_phase[c] == ph;
      peak_msms = std::max(peak_msms, a * ncirc);
    }
    peak_msms = std::max(peak_msms, 2 * ncirc * pk.cs.NL);
    peak_msms = std::max(peak_msms, ncirc * (pk.cs.nsets + pk.cs.NL + pk.cs.NS));
    return peak_msms;
  }

  ProofRun(Device* d, Params& prm, ProvingKey& pk, const ProveIn& in, std::vector<uint8_t>* proof, int E_sub,
           bool pieces, bool xsplit)
      : d(d), prm(prm), pk(pk), in(in), proof(proof), E_sub(E_sub), pieces(pieces), xsplit(xsplit) {
    for (int c = 0; c < ncirc; c++) W[c] = pk.cws[c].get();
    std::memset(challenges.data(), 0, challenges.size() * sizeof(Fr));
  }
  int instances();
  int advice_phases();
  int lookup_permuted();
  int permutation_products();
  int lookup_shuffle_products();
  int vanishing_commit();
  int eval_h();
  int eval_h_streamed();
  int h_commit();
  int openings_and_evals();
  MultiopenCtx multiopen_ctx();
  int gwc();
  int shplonk();
};

// ---- vk.hash_into + every circuit's instances (prover.rs:187-271; KZG: QUERY_INSTANCE = false)
int ProofRun::instances() {
  tr.common_scalar(pk.cs.transcript_repr);
  for (int ci = 0; ci < ncirc; ci++)
    for (int i = 0; i < pk.cs.I; i++) {
      const uint32_t len = in.inst_lens[ci][i];
      if ((size_t)len > n - (size_t)(bf + 1)) return fail(H2G_ERR_ARG, "create_proof: InstanceTooLarge");
      const uint64_t* col = in.instance[ci] + 4 * n * i;
      for (uint32_t r = 0; r < len; r++) tr.common_scalar(fr_from_limbs(col + 4 * r));
      HIPCHK(hipMemcpyAsync(W[ci]->inst_val[i], col, n * sizeof(Fr), hipMemcpyHostToDevice, st));
      if (!coef_recv) RCCHK(lagrange_to_coeff(d, D, W[ci]->inst_val[i], W[ci]->inst_poly[i], st));
    }
  return H2G_OK;
}

// ---- commit_phase per advice phase (prover.rs:309-494), circuit by circuit: the
// phase's blinding rows, its blinds, its commitments; then the phase's challenges
int ProofRun::advice_phases() {
  if (from_src)  // a witness source writes straight into pinned staging, one per circuit,
    for (CircuitWs* w : W) {  // allocated once (a pinned allocation costs more than the copies it speeds up)
      if (w->wit_pin) continue;
      const size_t bytes = (size_t)std::max(pk.cs.A, 1) * n * sizeof(Fr);
      if (hipHostMalloc((void**)&w->wit_pin, bytes, hipHostMallocDefault) == hipSuccess) {
        w->wit_pin_pinned = true;
      } else {  // pageable fallback: slower uploads, same bytes
        (void)hipGetLastError();
        w->wit_pin = static_cast<uint64_t*>(std::malloc(bytes));
        w->wit_pin_pinned = false;
        if (!w->wit_pin) return fail(H2G_ERR_NOMEM, "create_proof: witness staging allocation failed");
      }
    }
  HIPCHK(pk.d_seeds.ensure(van_off.size() * 8));
  HIPCHK(pk.d_offsets.ensure(van_off.size()));
  for (int ph = 0; ph <= pk.cs.max_phase; ph++) {
    if (ph == 0 && van_first) RCCHK(launch_van_early());
    std::vector<int> cols;
    for (int c = 0; c < pk.cs.A; c++)
      if (pk.cs.adv_phase[c] == ph) cols.push_back(c);
    if (from_src && ph > 0) HIPCHK(hipStreamSynchronize(st));  // the previous phase's uploads read the staging
    std::vector<MsmTicket> tk(cols.size() * ncirc);
    // a wide phase: column i (circuit-major) is rank i mod world's -- every rank uploads the
    // whole witness (the lookups and products read it), only the owner commits and
    // transforms the column
    const bool adv_wide = wide((int)(cols.size() * ncirc));
    const bool digest = g_spmd.world > 1 && !cols.empty();  // this phase's witness into the consistency digest
    if (digest) RCCHK(spmd_witness_prepare(pk, (int)(ncirc * cols.size()), st));
    for (int ci = 0; ci < ncirc; ci++) {
      CircuitWs& w = *W[ci];
      const uint64_t* from = in.advice ? in.advice[ci] : nullptr;
      bool from_dev = in.adv_dev;
      // copy_columns reads device advice in 16-byte chunks: refuse what it cannot
      if (from_dev && from && (reinterpret_cast<uintptr_t>(from) & 15) != 0)
        return fail(H2G_ERR_ARG, "create_proof: device advice must be 16-byte aligned");
      if (from_src) {
        // the staging outlives proofs: the unusable rows of unblinded columns start at zero
        // as the reference requires (prover.rs:417-421), whatever an earlier proof left there
        for (int c : cols)
          if (pk.unblinded[c]) std::memset(w.wit_pin + 4 * (n * c + unusable), 0, (n - unusable) * sizeof(Fr));
        const uint64_t* chp = reinterpret_cast<const uint64_t*>(challenges.data());
        h2g_assigned_dens dn = {nullptr, nullptr, 0};
        if (asg_pending) {  // the last list is the callback's again once its upload has been read
          HIPCHK(hipEventSynchronize(pk.asg_ev));
          asg_pending = false;
        }
        const int frc = in.asg   ? in.asg->fill(in.asg->ctx, (uint32_t)ci, (uint32_t)ph, chp, w.wit_pin, &dn)
                        : in.src ? in.src->fill(in.src->ctx, (uint32_t)ci, (uint32_t)ph, chp, w.wit_pin)
                                 : in.src1->fill(in.src1->ctx, (uint32_t)ph, chp, w.wit_pin);
        if (frc)
          return fail(H2G_ERR_ARG, "create_proof: witness source failed at " +
                                       (ncirc > 1 ? "circuit " + std::to_string(ci) + " " : std::string()) + "phase " +
                                       std::to_string(ph));
        from = w.wit_pin;
        from_dev = false;
        if (in.asg) {
          RCCHK(assigned_convert(ci, ph, cols, w, dn));
          from = reinterpret_cast<const uint64_t*>(pk.asg_num.p);
          from_dev = true;
        }
      }
      // column by column: upload, blinding rows, and (when the MSMs go one by one) the
      // commitment at once, so that a column's MSM overlaps the next column's upload
      // from host memory; the RNG draws keep the reference's order (every column's rows,
      // then every column's blind)
      const bool early = !adv_wide && commit_batch_chunk(prm, n, SRS_LAGRANGE) < 2;
      // device-resident columns come in through copy_columns (a streaming kernel, up to
      // COPY_COLS_MAX columns a launch; per-column DMA copies left the GPU idle for ~0.8 ms
      // of 32 columns at 2^18), host ones through the DMA upload; under SPMD either way
      // also takes each column's checksum before its blinding rows land (spmd_witness_fold)
      ColCopy cc{};
      int ncc = 0;
      auto flush = [&]() -> int {
        if (ncc) HIPCHK(copy_columns(cc, ncc, n, digest, st));
        ncc = 0;
        return H2G_OK;
      };
      auto blind = [&](int c) -> int {
        if (pk.unblinded[c]) return H2G_OK;
        Fr* rows = adv_blind.data() + ((size_t)ci * pk.cs.A + c) * (bf + 1);
        for (int i = 0; i <= bf; i++) rows[i] = rng.random_fr();
        HIPCHK(pk_upload(pk, w.adv[c] + unusable, rows, (size_t)(bf + 1) * sizeof(Fr), st));
        return H2G_OK;
      };
      for (size_t k = 0; k < cols.size(); k++) {
        const int c = cols[k];
        const Fr* src = reinterpret_cast<const Fr*>(from + 4 * n * c);
        unsigned long long* sum = digest ? pk.wsum_d.p + (size_t)ci * cols.size() + k : nullptr;
        if (from_dev) {
          cc.src[ncc] = src;
          cc.dst[ncc] = w.adv[c];
          cc.sum[ncc++] = sum;
        } else {
          HIPCHK(hipMemcpyAsync(w.adv[c], src, n * sizeof(Fr), hipMemcpyHostToDevice, st));
          if (digest) {
            cc.src[ncc] = w.adv[c];
            cc.dst[ncc] = nullptr;
            cc.sum[ncc++] = sum;
          }
        }
        if (early || ncc == COPY_COLS_MAX || !from_dev) RCCHK(flush());
        if (early) {
          RCCHK(blind(c));
          RCCHK(commit_launch(d, prm, w.adv[c], n, SRS_LAGRANGE, st, &tk[(size_t)ci * cols.size() + k]));
        }
      }
      RCCHK(flush());
      if (!early) {  // every column's rows drawn in order, then one upload for the phase
        HIPCHK(pk.blind_d.ensure((size_t)pk.cs.A * (bf + 1)));
        std::vector<CopySeg> segs;
        for (int c : cols) {
          if (pk.unblinded[c]) continue;
          Fr* rows = adv_blind.data() + ((size_t)ci * pk.cs.A + c) * (bf + 1);
          for (int i = 0; i <= bf; i++) rows[i] = rng.random_fr();
          segs.push_back(CopySeg{pk.blind_d.p + (size_t)c * (bf + 1), w.adv[c] + unusable, (uint64_t)(bf + 1)});
        }
        RCCHK(upload_rows_batch(pk, adv_blind.data() + (size_t)ci * pk.cs.A * (bf + 1), (size_t)pk.cs.A * (bf + 1), segs,
                                st));
      }
      for (int c : cols)
        if (!pk.unblinded[c]) (void)rng.random_fr();  // commitment blinds (unused by KZG)
      if (!cols.empty() && !early && !adv_wide) {
        std::vector<const Fr*> polys(cols.size());
        for (size_t i = 0; i < cols.size(); i++) polys[i] = w.adv[cols[i]];
        RCCHK(commit_launch_batch(d, prm, polys.data(), (int)cols.size(), n, SRS_LAGRANGE, st,
                                  tk.data() + (size_t)ci * cols.size()));
      }
    }
    if (digest) RCCHK(spmd_witness_fold(pk, (int)(ncirc * cols.size()), st));
    std::vector<int> adv_owner;
    std::vector<const Fr*> adv_lag;
    std::vector<Fr*> adv_poly, adv_cst;
    if (adv_wide) {
      for (int ci = 0; ci < ncirc; ci++)
        for (int c : cols) {
          adv_owner.push_back((int)(adv_owner.size() % (size_t)Wsp));
          adv_lag.push_back(W[ci]->adv[c]);
          adv_poly.push_back(W[ci]->adv_poly[c]);
          adv_cst.push_back(W[ci]->adv_coset[c]);
        }
      RCCHK(commit_launch_owned(d, prm, adv_lag.data(), adv_owner.data(), (int)adv_lag.size(), n, SRS_LAGRANGE, st,
                                tk.data()));
    }
    // the phase's advice to coefficient form and its extended-domain cosets do not depend
    // on any challenge: queued behind the uploads, they run while the commitment MSMs
    // (their own streams) are in flight (lagrange_to_coeff, prover.rs:673-689; the
    // cosets of evaluation.rs:344-361)
    if (pieces && !adv_wide && !cols.empty()) {  // one owner per column, every circuit's
      std::vector<const Fr*> l2;
      std::vector<Fr*> p2, c2;
      for (int ci = 0; ci < ncirc; ci++)
        for (int c : cols) {
          l2.push_back(W[ci]->adv[c]);
          p2.push_back(W[ci]->adv_poly[c]);
          c2.push_back(W[ci]->adv_coset[c]);
        }
      if (defer_adv) xform_later(l2, p2, c2);
      else RCCHK(xform(l2, p2, c2, nullptr));
    }
    for (int ci = 0; ci < ncirc && !cols.empty() && !adv_wide && !pieces; ci++) {
      CircuitWs& w = *W[ci];
      std::vector<const Fr*> src;
      std::vector<Fr*> dst, cst;
      for (int c : cols) {
        src.push_back(w.adv[c]);
        dst.push_back(w.adv_poly[c]);
        cst.push_back(w.adv_coset[c]);
      }
      if (coef_recv) continue;  // coefficients from the owners (coef_exchange), no cosets
      RCCHK(xs_begin());
      RCCHK(lagrange_to_coeff_batch(d, D, src.data(), dst.data(), (int)cols.size(), xst));
      RCCHK(ext_cosets(d, pk, (const Fr* const*)dst.data(), cst.data(), (int)cols.size(), xst));
      RCCHK(xs_end());
    }
    if (adv_wide) {
      RCCHK(xform(adv_lag, adv_poly, adv_cst, &adv_owner));
      for (int ci = 0; ci < ncirc; ci++)
        for (int c : cols) adv_shard[(size_t)ci * pk.cs.A + c] = 1;
    }
    if (ph == 0 && early_van && !van_first) RCCHK(launch_van_early());
    if (ph == 0) clk.mark("upload+instances");
    {  // circuit by circuit, column by column
      std::vector<MsmTicket*> tl;
      for (auto& t : tk) tl.push_back(&t);
      RCCHK(collect_write(tl));
    }
    RCCHK(rng_ok());
    for (int i = 0; i < NCH; i++)
      if (pk.cs.ch_phase[i] == ph) challenges[i] = tr.squeeze();
  }
  if (NCH)
    HIPCHK(pk_upload(pk, pk.consts + pk.num_consts, challenges.data(), NCH * sizeof(Fr), st));
  g_last_challenges = challenges;
  clk.mark("advice commit");
  return H2G_OK;
}

// ---- lookup_commit_permuted, per circuit, per lookup (lookup/prover.rs:64-173, 410-494)
int ProofRun::lookup_permuted() {
  ch.theta = tr.squeeze();
  {
    std::vector<MsmTicket> tk(2 * NLT);
    const size_t u = unusable;
    // per-lookup host staging (random rows, match counters): no host synchronisation
    // between lookups, so their device pipelines queue back to back; the counters are
    // checked once all lookups are queued
    std::vector<Fr> rows((size_t)NLT * 2 * (bf + 1));
    constexpr int LKC = ProvingKey::LKC;
    constexpr int LKF = ProvingKey::LKF;
    HIPCHK(pk.lk_cnt.ensure((size_t)NLT * LKC));
    HIPCHK(pk.lk_or_d.ensure((size_t)NLT * LKF));
    HIPCHK(pk.lk_or_h.ensure((size_t)NLT * LKF));
    if ((int)pk.lk_hb.size() < NLT) pk.lk_hb.resize(NLT, 64);
    if (NLT) HIPCHK(hipMemsetAsync(pk.lk_or_d.p, 0, (size_t)NLT * LKF * sizeof(unsigned long long), st));
    // permute_expression_pair (lookup/prover.rs:410-494): sort by Ord (canonical value),
    // match, fill leftovers; then the bf + 1 random rows (input first, then table).
    // Every lookup's two columns go through ONE radix sort (radix.hip): column g = 2 j + side
    // keys on a 48-bit window of its canonical values -- bits [hb - 48, hb) below the value
    // width hb the previous proof measured for that lookup (lk_hb) -- with g above the
    // window, so each column's rows come out contiguous and sorted.  The gather of the
    // canonical values checks the order (a window that tied different values); a lookup
    // whose check or width failed, or whose width is unknown (hb 0), is sorted in full
    // (four stable 64-bit limb sorts, least significant first).
    // a wide lookup stage: lookup j is rank j mod world's (its compression, sort, match and
    // fill, commitments and transforms); every rank still makes every RNG draw.  lq[j]:
    // the lookup's region in the batch buffers (-1: another rank's)
    const bool lk_wide = wide(NLT);
    std::vector<int>& lk_owner = lk_owner_all;
    std::vector<int> lq(NLT, -1);
    int nown = 0;
    for (int j = 0; j < NLT; j++) {
      if (lk_wide) lk_owner[j] = j % Wsp;
      if (lk_owner[j] == g_spmd.rank) lq[j] = nown++;
    }
    // Lookups with identical table expressions (the same table, e.g. keccak's nibble-xor
    // columns for every lookup) share one sorted table: lookup j gathers it from lookup
    // tsrc[j]'s group.  Batch groups: the inputs [0, nown), then one per distinct table
    // (single-owner stages, and only while every lookup sorts by its
    // window -- a full sort writes its table group).  Otherwise two groups per lookup.
    std::vector<int> tsrc(NLT), gi0(NLT, -1), gi1(NLT, -1);
    bool share = !lk_wide && pk.lk_trep.size() == (size_t)pk.cs.NL && (int)pk.lk_hb.size() >= NLT;
    for (int j = 0; j < NLT && share; j++)
      if (lq[j] >= 0 && pk.lk_hb[j] == 0) share = false;
    int ntab = 0;
    for (int j = 0; j < NLT; j++) {
      tsrc[j] = j;
      if (lq[j] < 0) continue;
      if (share) {
        const int r = (j / pk.cs.NL) * pk.cs.NL + pk.lk_trep[j % pk.cs.NL];
        if (lq[r] >= 0) tsrc[j] = r;
        gi0[j] = lq[j];
        if (tsrc[j] == j) gi1[j] = nown + ntab++;
        else gi1[j] = gi1[tsrc[j]];  // (r < j: assigned already)
      } else {
        gi0[j] = 2 * lq[j];
        gi1[j] = 2 * lq[j] + 1;
      }
    }
    const int G = share ? nown + ntab : 2 * nown;
    int gbits = 0;
    while ((1 << gbits) < G) gbits++;
    if (NLT) {  // the batch buffers, sized before anything below takes an address in them
      const size_t m = (size_t)G * u;
      HIPCHK(pk.lkb_canon.ensure(m));
      for (int q = 0; q < 2; q++) {
        HIPCHK(pk.lkb_key[q].ensure(m));
        HIPCHK(pk.lkb_idx[q].ensure(m));
      }
      HIPCHK(pk.lkb_scr.ensure(std::max(std::max(radix_sort_scratch_bytes(m), radix_sort_scratch_bytes(n)),
                                        compact_scratch_bytes(n))));
    }
    // the match and fill of lookup j from its sorted columns (pk.ck_a2 input, pk.ck_t2 table)
    // every lookup's counters and flags cleared at once (a redo clears its own again)
    HIPCHK(pk.lk_counters.ensure((size_t)NLT * LKC));
    HIPCHK(pk.lk_flags.ensure((size_t)NLT * u));
    if (NLT) {
      HIPCHK(hipMemsetAsync(pk.lk_counters.p, 0, (size_t)NLT * LKC * sizeof(uint32_t), st));
      HIPCHK(hipMemsetAsync(pk.lk_flags.p, 1, (size_t)NLT * u, st));
    }
    // scratch set q (0: the key's own) for the gathers and matches
    struct LkSet {
      CanonKey *a2, *t2, *left;
      uint8_t* rep;
      uint32_t* rows;
      void* scr;
    };
    auto lk_set = [&](int q) -> LkSet {
      if (q == 0) return LkSet{pk.ck_a2, pk.ck_t2, pk.ck_left, pk.rep_flag, pk.rep_rows, pk.lkb_scr.p};
      return LkSet{pk.lks_a2[q], pk.lks_t2[q], pk.lks_left[q], pk.lks_rep[q], pk.lks_rows[q], pk.lks_scr[q]};
    };
    auto match_fill = [&](int j, bool again, const LkSet& z, hipStream_t sj) -> int {
      const int ci = j / pk.cs.NL, l = j % pk.cs.NL;
      CircuitWs& w = *W[ci];
      uint32_t* cnt = pk.lk_counters.p + (size_t)LKC * j;
      uint8_t* flags = pk.lk_flags.p + (size_t)j * u;
      if (again) {
        HIPCHK(hipMemsetAsync(flags, 1, u, sj));
        HIPCHK(hipMemsetAsync(cnt, 0, LKC * sizeof(uint32_t), sj));
      }
      HIPCHK(lookup_mark(z.a2, z.t2, u, z.rep, flags, cnt + 2, sj));
      HIPCHK(compact_canon(z.t2, flags, u, z.left, cnt, z.scr, sj));
      HIPCHK(compact_index(z.rep, u, z.rows, cnt + 1, z.scr, sj));
      HIPCHK(lookup_assign(z.a2, z.rep, u, w.lk_ap[l], w.lk_sp[l], sj));
      HIPCHK(lookup_scatter(z.left, z.rows, cnt + 1, u, w.lk_sp[l], sj));
      if (again)
        HIPCHK(hipMemcpyAsync(pk.lk_cnt.p + (size_t)LKC * j, cnt, LKC * sizeof(uint32_t), hipMemcpyDeviceToHost, sj));
      return H2G_OK;  // the blinding rows of every lookup land together below (upload_rows_batch)
    };
    // the full sort of lookup j's columns into pk.ck_a2 / ck_t2 (radix sorts on the limbs,
    // in lookup j's own regions of the batch's key / index buffers)
    auto full_sort = [&](int j) -> int {
      const int ci = j / pk.cs.NL, l = j % pk.cs.NL;
      CircuitWs& w = *W[ci];
      const Fr* srcs[2] = {w.lk_a[l], w.lk_s[l]};
      CanonKey* sorted[2] = {pk.ck_a2, pk.ck_t2};
      for (int side = 0; side < 2; side++) {
        CanonKey* canon = pk.lkb_canon.p + (size_t)(side ? gi1[j] : gi0[j]) * u;
        HIPCHK(lookup_keys(srcs[side], u, 0, canon, nullptr, nullptr, pk.lk_or_d.p + (size_t)LKF * j, st));
        const size_t o = (size_t)gi0[j] * u;  // (the sort's scratch: the lookup's input group)
        uint64_t *k0 = pk.lkb_key[0].p + o, *k1 = pk.lkb_key[1].p + o;
        uint32_t *i0 = pk.lkb_idx[0].p + o, *i1 = pk.lkb_idx[1].p + o;
        HIPCHK(iota_u32(i0, u, st));
        for (int limb = 0; limb < 4; limb++) {  // least significant first; 8 passes end where they began
          HIPCHK(canon_limb_keys(canon, i0, u, limb, k0, st));
          bool alt = false;
          HIPCHK(radix_sort_pairs(k0, i0, k1, i1, u, 0, 64, pk.lkb_scr.p, st, &alt));
          if (alt) return fail(H2G_ERR_STATE, "lookup full sort: unexpected pass parity");
        }
        HIPCHK(lookup_gather(canon, i0, u, sorted[side], pk.lk_or_d.p + (size_t)LKF * j + 4, st));
      }
      return H2G_OK;
    };
    std::vector<int> used(NLT);
    {  // every lookup's compressed input and table, batched launches
      CompressBatch cb;
      cb.prog = pk.prog;
      cb.n_slots = pk.n_slots;
      cb.consts = pk.consts;
      cb.load_rot = pk.d_load_rot;
      cb.n = n;
      cb.theta = theta;
      auto add = [&](int2 seg, const CircuitWs& w, Fr* out) -> int {
        if (cb.count == COMPRESS_BATCH_MAX) {
          HIPCHK(compress_lagrange_batch(cb, st));
          cb.count = 0;
        }
        cb.seg[cb.count] = seg;
        cb.load_col[cb.count] = w.d_load_col_lag;
        cb.out[cb.count++] = out;
        return H2G_OK;
      };
      for (int ci = 0; ci < ncirc; ci++)
        for (int l = 0; l < pk.cs.NL; l++)
          if (lq[ci * pk.cs.NL + l] >= 0) {
            RCCHK(add(pk.seg_lk_in[l], *W[ci], W[ci]->lk_a[l]));
            RCCHK(add(pk.seg_lk_tab[l], *W[ci], W[ci]->lk_s[l]));
          }
      HIPCHK(compress_lagrange_batch(cb, st));
    }
    LookupKeysBatch kb;  // every column's keys, batched launches
    kb.n = u;
    kb.canon = pk.lkb_canon.p;
    kb.key = pk.lkb_key[0].p;
    kb.idx = pk.lkb_idx[0].p;
    kb.kbits = 48;
    kb.kmask = (1ull << 48) - 1;
    for (int ci = 0; ci < ncirc; ci++)
      for (int l = 0; l < pk.cs.NL; l++) {
        const int j = ci * pk.cs.NL + l;
        for (int which = 0; which < 2; which++) {
          Fr* r = rows.data() + ((size_t)2 * j + which) * (bf + 1);
          for (int i = 0; i <= bf; i++) r[i] = rng.random_fr();
        }
        (void)rng.random_fr();  // permuted input blind
        (void)rng.random_fr();  // permuted table blind
        if (lq[j] < 0) continue;
        used[j] = pk.lk_hb[j];
        const int shift = used[j] > 48 ? used[j] - 48 : 0;
        const Fr* srcs[2] = {W[ci]->lk_a[l], W[ci]->lk_s[l]};
        for (int side = 0; side < 2; side++) {  // every column keys (a full-sort lookup's are ignored)
          if (side == 1 && tsrc[j] != j) continue;  // a shared table: keyed once, by tsrc[j]
          if (kb.count == LOOKUP_KEYS_BATCH_MAX) {
            HIPCHK(lookup_keys_batch(kb, st));
            kb.count = 0;
          }
          kb.in[kb.count] = srcs[side];
          kb.s[kb.count] = shift;
          kb.g[kb.count] = side ? gi1[j] : gi0[j];
          kb.d_or[kb.count++] = pk.lk_or_d.p + (size_t)LKF * j;
        }
      }
    HIPCHK(lookup_keys_batch(kb, st));
    if (nown) {
      bool alt = false;
      HIPCHK(radix_sort_pairs(pk.lkb_key[0].p, pk.lkb_idx[0].p, pk.lkb_key[1].p, pk.lkb_idx[1].p, (size_t)G * u, 0,
                              48 + gbits, pk.lkb_scr.p, st, &alt));
      const uint32_t* sidx = pk.lkb_idx[alt ? 1 : 0].p;
      // the lookups' gathers and matches on LKS streams when none needs the full sort (its
      // radix passes use the key's scratch); lookup q-th of this rank on stream q mod LKS
      bool multi = nown > 1;
      for (int j = 0; j < NLT; j++) multi = multi && (lq[j] < 0 || used[j] != 0);
      const int S = multi ? std::min(nown, ProvingKey::LKS) : 1;
      if (S > 1) {
        if (!pk.lks_a2[1]) {  // (u is the key's: these never grow)
          for (int q = 1; q < ProvingKey::LKS; q++) {
            PALLOC(pk.pool, pk.lks_a2[q], u);
            PALLOC(pk.pool, pk.lks_t2[q], u);
            PALLOC(pk.pool, pk.lks_left[q], u);
            PALLOC(pk.pool, pk.lks_rep[q], u);
            PALLOC(pk.pool, pk.lks_rows[q], u);
            HIPCHK(pk.pool.get(&pk.lks_scr[q], compact_scratch_bytes(u)));
          }
        }
        for (Stream& s : pk.lk_st) HIPCHK(s.ensure());
        for (Event& e : pk.lk_ev) HIPCHK(e.ensure());
        HIPCHK(hipEventRecord(pk.lk_ev[0], st));  // the sort is done
        for (int q = 0; q < S; q++) HIPCHK(hipStreamWaitEvent(pk.lk_st[q], pk.lk_ev[0], 0));
      }
      int qi = 0;
      for (int j = 0; j < NLT; j++) {
        if (lq[j] < 0) continue;
        const int q = S > 1 ? qi % S : 0;
        qi++;
        const LkSet z = lk_set(q);
        hipStream_t sj = S > 1 ? pk.lk_st[q] : st;
        if (used[j] == 0) {
          RCCHK(full_sort(j));
        } else {
          for (int side = 0; side < 2; side++) {
            const size_t g = (size_t)(side ? gi1[j] : gi0[j]);
            HIPCHK(lookup_gather(pk.lkb_canon.p + g * u, sidx + g * u, u, side ? z.t2 : z.a2,
                                 pk.lk_or_d.p + (size_t)LKF * j + 4, sj));
          }
        }
        RCCHK(match_fill(j, false, z, sj));
      }
      if (S > 1) {  // join
        for (int q = 0; q < S; q++) {
          HIPCHK(hipEventRecord(pk.lk_ev[q + 1], pk.lk_st[q]));
          HIPCHK(hipStreamWaitEvent(st, pk.lk_ev[q + 1], 0));
        }
      }
    }
    if (NLT) {
      HIPCHK(hipMemcpyAsync(pk.lk_cnt.p, pk.lk_counters.p, (size_t)NLT * LKC * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            st));
      HIPCHK(hipMemcpyAsync(pk.lk_or_h.p, pk.lk_or_d.p, (size_t)NLT * LKF * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));  // counters and value masks landed; rows (host) read
    }
    // a sort whose assumption failed (values wider than its window, or a window that tied
    // different values out of order) is redone with the full sort; the width is
    // remembered for the next proof
    bool redo = false;
    std::vector<char> redone(NLT, 0);  // a lookup matched against a shared table redone with it
    for (int j = 0; j < NLT; j++) {
      if (lq[j] < 0 || used[j] == 0) continue;
      const unsigned long long* f = pk.lk_or_h.p + (size_t)LKF * j;
      int hb = 0;
      for (int q = 3; q >= 0 && !hb; q--)
        if (f[q]) hb = 64 * q + 64 - __builtin_clzll(f[q]);
      if (hb == 0) hb = 1;
      const bool tie = f[4] != 0;
      pk.lk_hb[j] = tie && hb == used[j] ? 0 : hb;  // ties at the right width: full sort from now on
      if (tie || hb > used[j] || redone[tsrc[j]]) {
        RCCHK(full_sort(j));
        RCCHK(match_fill(j, true, lk_set(0), st));
        redo = true;
        redone[j] = 1;
      }
    }
    if (redo) HIPCHK(hipStreamSynchronize(st));
    {  // the blinding rows of A'_l and S'_l of every lookup this rank sorted, one upload
      HIPCHK(pk.blind_d.ensure(rows.size()));
      std::vector<CopySeg> segs;
      for (int j = 0; j < NLT; j++) {
        if (lq[j] < 0) continue;
        CircuitWs& w = *W[j / pk.cs.NL];
        const int l = j % pk.cs.NL;
        for (int which = 0; which < 2; which++)
          segs.push_back(CopySeg{pk.blind_d.p + ((size_t)2 * j + which) * (bf + 1), (which ? w.lk_sp[l] : w.lk_ap[l]) + u,
                                 (uint64_t)(bf + 1)});
      }
      RCCHK(upload_rows_batch(pk, rows.data(), rows.size(), segs, st));
    }
    bool lk_ok = true;
    for (int j = 0; j < NLT; j++) {
      const uint32_t* cnt = pk.lk_cnt.p + (size_t)LKC * j;
      if (lq[j] >= 0 && (cnt[2] != 0 || cnt[0] != cnt[1])) lk_ok = false;
    }
    if (lk_wide) {  // every rank learns whether any owner's lookup failed (none may hang in a collective)
      std::vector<Fr> mine(1, lk_ok ? Fr::zero() : Fr::one()), all;
      RCCHK(spmd_allgather_fr(mine, &all));
      for (const Fr& f : all) lk_ok = lk_ok && f.is_zero();
    }
    if (!lk_ok) return fail(H2G_ERR_ARG, "create_proof: lookup input value not in the table (ConstraintSystemFailure)");
    std::vector<const Fr*> perm_cols;  // (A'_l, S'_l) in transcript order
    std::vector<Fr*> perm_polys, perm_cosets;
    for (int ci = 0; ci < ncirc; ci++)
      for (int l = 0; l < pk.cs.NL; l++) {
        CircuitWs& w = *W[ci];
        perm_cols.push_back(w.lk_ap[l]);
        perm_cols.push_back(w.lk_sp[l]);
        perm_polys.push_back(w.lk_ap_poly[l]);
        perm_polys.push_back(w.lk_sp_poly[l]);
        perm_cosets.push_back(w.lk_apc[l]);
        perm_cosets.push_back(w.lk_spc[l]);
      }
    std::vector<int> own2(2 * NLT);
    for (int j = 0; j < NLT; j++) own2[2 * j] = own2[2 * j + 1] = lk_wide ? lk_owner[j] : g_spmd.rank;
    // A', S' against the prefix-summed Lagrange basis (params_prefix): the same commitments
    std::vector<const Fr*> com_cols = perm_cols;
    const int com_set = SRS_LAGRANGE_PREFIX;
    RCCHK(params_prefix(prm, st));
    // scalars only for the columns this rank commits (all of them but in a wide stage,
    // where a column belongs to its owner)
    size_t owned = 0;
    for (int i = 0; i < 2 * NLT; i++) owned += own2[i] == g_spmd.rank;
    HIPCHK(pk.lk_diff.ensure(std::max<size_t>(owned, 1) * n));
    PrefixDiff pd{};
    int m = 0;
    size_t slot = 0;
    for (int i = 0; i < 2 * NLT; i++) {
      if (own2[i] != g_spmd.rank) {  // another rank's column (wide stage): not read here
        com_cols[i] = perm_cols[i];
        continue;
      }
      Fr* e = pk.lk_diff.p + (slot++) * n;
      com_cols[i] = e;
      pd.a[m] = perm_cols[i];
      pd.e[m] = e;
      if (++m == PREFIX_DIFF_MAX) {
        HIPCHK(prefix_diff(pd, m, n, st));
        m = 0;
      }
    }
    if (m) HIPCHK(prefix_diff(pd, m, n, st));
    if (lk_wide) {
      RCCHK(commit_launch_owned(d, prm, com_cols.data(), own2.data(), 2 * NLT, n, com_set, st, tk.data()));
      RCCHK(xform(perm_cols, perm_polys, perm_cosets, &own2));
    } else {
      RCCHK(commit_launch_batch(d, prm, com_cols.data(), 2 * NLT, n, com_set, st, tk.data()));
      // coefficient forms and cosets, batched transforms (they overlap the commitments)
      RCCHK(xform(perm_cols, perm_polys, perm_cosets, nullptr));
    }
    lk_shard = lk_wide;
    {
      std::vector<MsmTicket*> tl;
      for (int i = 0; i < 2 * NLT; i++) tl.push_back(&tk[i]);
      RCCHK(collect_write(tl));
    }
    RCCHK(rng_ok());
  }
  if (pk.cs.NL) clk.mark("lookup permuted");
  return H2G_OK;
}

// ---- permutation_commit per circuit (permutation/prover.rs:50-197); commitments are
// written after the loop (nothing is squeezed in between, so the transcript is unchanged)
int ProofRun::permutation_products() {
  ch.beta = tr.squeeze(), ch.gamma = tr.squeeze();
  dump("beta", &beta, 1, st, true);
  dump("gamma", &gamma, 1, st, true);
  // large MSMs start as soon as their set's z is ready; small ones wait and go as a batch
  const bool perm_batched = commit_batch_chunk(prm, n, SRS_LAGRANGE) > 1;
  for (CircuitWs* w : W)
    for (int s = 0; s < pk.cs.nsets; s++) {
      all_z_lag.push_back(w->z_lag[s]);
      all_z.push_back(w->z[s]);
      all_z_coset.push_back(w->z_coset[s]);
    }
  // with row pieces the grand products go by slabs: each rank forms its MSM slab's rows of
  // every set (denominators, inversion, numerators, a slab-local running product), one host
  // all-gather of the slabs' products chains the slabs and the sets (z_0 of set s + 1 is
  // set s's last product row), the commitments take the slabs, and each set's transform
  // owner gathers the whole column
  const bool perm_slab = pieces && NST > 0;
  if (perm_slab) {
    const int me = g_spmd.rank;
    const size_t plo = shard_lo(prm.n, n, Wsp, me), phi = shard_lo(prm.n, n, Wsp, me + 1), len = phi - plo;
    std::vector<Fr*> zl(NST), zs(NST);
    for (int i = 0; i < NST; i++) {
      zl[i] = all_z_lag[i] + plo;
      zs[i] = all_z[i] + plo;
    }
    for (int ci = 0; ci < ncirc; ci++)
      for (int s = 0; s < pk.cs.nsets; s++) {
        const int c0 = s * pk.cs.chunk_len, c1 = std::min(c0 + pk.cs.chunk_len, pk.cs.P);
        for (int c = c0; c < c1 && len; c += PERM_MAXC) {
          PermCols pc;
          pc.m = std::min(PERM_MAXC, c1 - c);
          for (int j = 0; j < pc.m; j++) {
            pc.v[j] = col_vals(*W[ci], c + j) + plo;
            pc.sigma[j] = pk.sigma_lag[c + j] + plo;
          }
          HIPCHK(perm_denominators(zl[(size_t)ci * pk.cs.nsets + s], len, pc, beta, gamma, c == c0, st));
        }
      }
    if (len) HIPCHK(poly_batch_invert_multi(zl.data(), zs.data(), NST, len, st));
    for (int ci = 0; ci < ncirc; ci++) {
      Fr deltaomega = Fr::one();
      for (int s = 0; s < pk.cs.nsets; s++) {
        const int c0 = s * pk.cs.chunk_len, c1 = std::min(c0 + pk.cs.chunk_len, pk.cs.P);
        for (int c = c0; c < c1; c += PERM_MAXC) {
          PermCols pc;
          pc.m = std::min(PERM_MAXC, c1 - c);
          for (int j = 0; j < pc.m; j++) {
            pc.v[j] = col_vals(*W[ci], c + j) + plo;
            pc.beta_delta[j] = deltaomega * beta;
            deltaomega = deltaomega * fr_delta();
          }
          if (len) HIPCHK(perm_numerators(zl[(size_t)ci * pk.cs.nsets + s], len, pc, gamma, pk.om, st, plo));
        }
      }
    }
    if (len)
      HIPCHK(poly_prefix_product_multi((const Fr* const*)zl.data(), zs.data(), NST, len, pk.scr, pk.scr_len, st));
    // the slab's product of the rows that feed z (factors below n - bf - 1)
    const size_t hc = std::min(phi, n - (size_t)bf - 1);
    std::vector<Fr> tp(NST, Fr::one());
    if (hc > plo)
      for (int i = 0; i < NST; i++)
        HIPCHK(hipMemcpyAsync(&tp[i], all_z[i] + hc - 1, sizeof(Fr), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<Fr> allp;
    RCCHK(spmd_allgather_fr(tp, &allp));
    std::vector<Fr> lzp(NST);  // z at this slab's first row = z_0 * (the slabs below)
    for (int ci = 0; ci < ncirc; ci++) {
      Fr lz = Fr::one();
      for (int s = 0; s < pk.cs.nsets; s++) {
        const int i = ci * pk.cs.nsets + s;
        Fr below = Fr::one(), all = Fr::one();
        for (int r = 0; r < Wsp; r++) {
          if (r < me) below = below * allp[(size_t)r * NST + i];
          all = all * allp[(size_t)r * NST + i];
        }
        lzp[i] = lz * below;
        lz = lz * all;
      }
    }
    HIPCHK(pk.perm_lz.ensure(std::max(NST, 1)));
    HIPCHK(pk_upload(pk, pk.perm_lz.p, lzp.data(), NST * sizeof(Fr), st));
    for (int i = 0; i < NST; i++) {
      Fr* blind_rows = perm_blind.data() + (size_t)i * bf;
      for (int q = 0; q < bf; q++) blind_rows[q] = rng.random_fr();
      (void)rng.random_fr();  // blind
      HIPCHK(pk_upload(pk, pk.small, blind_rows, bf * sizeof(Fr), st));
      HIPCHK(perm_z_assemble(all_z_lag[i], n, bf, all_z[i], pk.perm_lz.p + i, pk.small, st, plo, phi));
    }
    HIPCHK(hipStreamSynchronize(st));  // lzp (host) was read
    RCCHK(commit_launch_batch(d, prm, (const Fr* const*)all_z_lag.data(), NST, n, SRS_LAGRANGE, st, perm_tk.data()));
    // each set's owner gathers its column, then transforms and distributes it
    std::vector<int> own(NST);
    for (int i = 0; i < NST; i++) own[i] = (tr_next + i) % Wsp;
    tr_next += NST;
    RCCHK(gather_to_owners(pk, all_z_lag, own, prm.n, st));
    RCCHK(xform(std::vector<const Fr*>(all_z_lag.begin(), all_z_lag.end()), all_z, all_z_coset, &own));
    RCCHK(run_deferred());  // the advice columns' transforms beside the products
  }
  if (!perm_slab) {
    // every set's denominators (into z_lag), one batched inversion over all circuits'
    // sets (z as its scratch until the iNTT fills it), then per set numerators, scan and z
    for (int ci = 0; ci < ncirc; ci++)
      for (int s = 0; s < pk.cs.nsets; s++) {
        const int c0 = s * pk.cs.chunk_len, c1 = std::min(c0 + pk.cs.chunk_len, pk.cs.P);
        for (int c = c0; c < c1; c += PERM_MAXC) {
          PermCols pc;
          pc.m = std::min(PERM_MAXC, c1 - c);
          for (int j = 0; j < pc.m; j++) {
            pc.v[j] = col_vals(*W[ci], c + j);
            pc.sigma[j] = pk.sigma_lag[c + j];
          }
          HIPCHK(perm_denominators(W[ci]->z_lag[s], n, pc, beta, gamma, c == c0, st));
        }
      }
    if (NST) dump("den0", W[0]->z_lag[0], n, st);
    HIPCHK(poly_batch_invert_multi(all_z_lag.data(), all_z.data(), NST, n, st));
    if (NST) dump("inv0", W[0]->z_lag[0], n, st);
    // (every set's numerators, then one batched scan of all sets: measured, rejected)
    for (int ci = 0; ci < ncirc; ci++) {
      CircuitWs& w = *W[ci];
      HIPCHK(hipMemcpyAsync(pk.last_z, pk.one, sizeof(Fr), hipMemcpyDeviceToDevice, st));  // z_0 starts at one
      Fr deltaomega = Fr::one();
      for (int s = 0; s < pk.cs.nsets; s++) {
        Fr* blind_rows = perm_blind.data() + ((size_t)ci * pk.cs.nsets + s) * bf;
        const int c0 = s * pk.cs.chunk_len, c1 = std::min(c0 + pk.cs.chunk_len, pk.cs.P);
        Fr* prod = w.z_lag[s];
        for (int c = c0; c < c1; c += PERM_MAXC) {
          PermCols pc;
          pc.m = std::min(PERM_MAXC, c1 - c);
          for (int j = 0; j < pc.m; j++) {
            pc.v[j] = col_vals(w, c + j);
            pc.beta_delta[j] = deltaomega * beta;
            deltaomega = deltaomega * fr_delta();
          }
          HIPCHK(perm_numerators(prod, n, pc, gamma, pk.om, st));
        }
        // z = last_z * running product, blinding rows from the rng
        if (ci == 0 && s == 0) dump("mod0", prod, n, st);
        HIPCHK(poly_prefix_product(prod, pk.pre, n, pk.scr, pk.scr_len, st));
        if (ci == 0 && s == 0) dump("pre0", pk.pre, n, st);
        for (int i = 0; i < bf; i++) blind_rows[i] = rng.random_fr();
        (void)rng.random_fr();  // blind
        HIPCHK(pk_upload(pk, pk.small, blind_rows, bf * sizeof(Fr), st));
        HIPCHK(perm_z_assemble(w.z_lag[s], n, bf, pk.pre, pk.last_z, pk.small, st));
        HIPCHK(hipMemcpyAsync(pk.last_z, w.z_lag[s] + (n - (size_t)(bf + 1)), sizeof(Fr), hipMemcpyDeviceToDevice,
                              st));
        if (ci == 0 && s == 0) {
          dump("z0", w.z_lag[s], n, st);
          dump("sigma0", pk.sigma_lag[0], n, st);
          dump("v0", col_vals(w, 0), n, st);
        }
        if (!perm_batched)
          RCCHK(commit_launch(d, prm, w.z_lag[s], n, SRS_LAGRANGE, st, &perm_tk[(size_t)ci * pk.cs.nsets + s]));
      }
    }
    RCCHK(xform(std::vector<const Fr*>(all_z_lag.begin(), all_z_lag.end()), all_z, all_z_coset, nullptr));
  }
  if (perm_batched && !perm_slab)
    RCCHK(commit_launch_batch(d, prm, (const Fr* const*)all_z_lag.data(), NST, n, SRS_LAGRANGE, st, perm_tk.data()));
  clk.mark("permutation products");
  return H2G_OK;
}

// ---- lookup products (lookup/prover.rs:182-325), every circuit's, then shuffle
// products (shuffle/prover.rs:97-206): z = [1, running product ...], bf random rows, blind
int ProofRun::lookup_shuffle_products() {
  {
    std::vector<const Fr*> z_lags;
    std::vector<Fr*> z_polys, z_cosets;
    // a wide lookup stage keeps its owners here: lookup j's product is rank j mod world's
    // (the permuted columns are already there); the others only make the RNG draws
    const bool lz_wide = lk_shard;
    auto mine = [&](int j) { return lk_owner_all[j] == g_spmd.rank; };
    size_t zrow = 0;
    // every product's random rows and blind, drawn up front in the products' order (no
    // other draws come between them) and uploaded once
    const size_t nprod = (size_t)NLT + (size_t)NSH;
    for (size_t z = 0; z < nprod; z++) {
      Fr* rows = prod_blind.data() + z * (size_t)bf;
      for (int i = 0; i < bf; i++) rows[i] = rng.random_fr();
      (void)rng.random_fr();  // product blind
    }
    if (nprod) {
      HIPCHK(pk.blind_d.ensure(nprod * (size_t)bf));
      HIPCHK(pk_upload(pk, pk.blind_d.p, prod_blind.data(), nprod * (size_t)bf * sizeof(Fr), st));
    }
    // prod: the running product's factors, or (scanned) already its prefix products
    auto finish_z = [&](const Fr* prod, Fr* z_lag, Fr* z_poly, Fr* z_coset, bool scanned, bool here,
                        bool listed) -> int {
      const Fr* rows_d = pk.blind_d.p + (zrow++) * (size_t)bf;
      if (!here) return H2G_OK;
      const Fr* pre = prod;
      if (!scanned) {
        HIPCHK(poly_prefix_product(prod, pk.pre, n, pk.scr, pk.scr_len, st));
        pre = pk.pre;
      }
      HIPCHK(perm_z_assemble(z_lag, n, bf, pre, pk.one, rows_d, st));
      if (listed) {
        z_lags.push_back(z_lag);
        z_polys.push_back(z_poly);
        z_cosets.push_back(z_coset);
      }
      return H2G_OK;
    };
    // every lookup's denominators go through one batched inversion (the per-thread
    // inversion's latency is paid once); z_poly holds the product until its iNTT,
    // z_lag serves as the inversion's scratch until z is assembled into it
    std::vector<Fr*> dens, dens_scr;
    for (int ci = 0, j = 0; ci < ncirc; ci++)
      for (int l = 0; l < pk.cs.NL; l++, j++) {
        if (!mine(j)) continue;
        CircuitWs* w = W[ci];
        HIPCHK(lookup_prod_den(w->lk_ap[l], w->lk_sp[l], beta, gamma, w->lk_z_poly[l], n, st));
        dens.push_back(w->lk_z_poly[l]);
        dens_scr.push_back(w->lk_z[l]);
      }
    if (!dens.empty()) HIPCHK(poly_batch_invert_multi(dens.data(), dens_scr.data(), (int)dens.size(), n, st));
    // numerators, then every lookup's running product in one batched scan (in place)
    for (int ci = 0, j = 0; ci < ncirc; ci++)
      for (int l = 0; l < pk.cs.NL; l++, j++)
        if (mine(j)) HIPCHK(lookup_prod_num(W[ci]->lk_a[l], W[ci]->lk_s[l], beta, gamma, W[ci]->lk_z_poly[l], n, st));
    if (!dens.empty())
      HIPCHK(poly_prefix_product_multi((const Fr* const*)dens.data(), dens.data(), (int)dens.size(), n, pk.scr,
                                       pk.scr_len, st));
    std::vector<const Fr*> lkz_lag;
    std::vector<Fr*> lkz_poly, lkz_cst;
    for (int ci = 0, j = 0; ci < ncirc; ci++)
      for (int l = 0; l < pk.cs.NL; l++, j++) {
        CircuitWs* w = W[ci];
        RCCHK(finish_z(w->lk_z_poly[l], w->lk_z[l], w->lk_z_poly[l], w->lk_zc[l], true, mine(j), !lz_wide));
        lkz_lag.push_back(w->lk_z[l]);
        lkz_poly.push_back(w->lk_z_poly[l]);
        lkz_cst.push_back(w->lk_zc[l]);
      }
    for (CircuitWs* w : W)
      for (int s = 0; s < pk.cs.NS; s++) {
        RCCHK(compress(*w, pk.seg_sh_in[s], pk.tmp_a));
        RCCHK(compress(*w, pk.seg_sh_sh[s], pk.tmp_b));
        HIPCHK(shuffle_prod_den(pk.tmp_b, gamma, pk.mod, n, st));
        HIPCHK(poly_batch_invert(pk.mod, n, pk.scr, st));
        HIPCHK(shuffle_prod_num(pk.tmp_a, gamma, pk.mod, n, st));
        RCCHK(finish_z(pk.mod, w->sh_z[s], w->sh_z_poly[s], w->sh_zc[s], false, true, true));
      }
    RCCHK(xform(z_lags, z_polys, z_cosets, nullptr));
    // product commitments: every circuit's lookups, then every circuit's shuffles
    std::vector<const Fr*> zs;
    for (CircuitWs* w : W) zs.insert(zs.end(), w->lk_z.begin(), w->lk_z.end());
    for (CircuitWs* w : W) zs.insert(zs.end(), w->sh_z.begin(), w->sh_z.end());
    std::vector<MsmTicket> zt(zs.size());
    if (lz_wide) {
      RCCHK(commit_launch_owned(d, prm, zs.data(), lk_owner_all.data(), NLT, n, SRS_LAGRANGE, st, zt.data()));
      if (NSH) RCCHK(commit_launch_batch(d, prm, zs.data() + NLT, NSH, n, SRS_LAGRANGE, st, zt.data() + NLT));
      RCCHK(xform(lkz_lag, lkz_poly, lkz_cst, &lk_owner_all));
    } else if (!zs.empty()) {
      RCCHK(commit_launch_batch(d, prm, zs.data(), (int)zs.size(), n, SRS_LAGRANGE, st, zt.data()));
    }
    for (int j = 0; j < NLT; j++) lkz_tk[j] = zt[j];
    for (int j = 0; j < NSH; j++) shz_tk[j] = zt[NLT + j];
  }
  if (pk.cs.NL + pk.cs.NS) clk.mark("lookup/shuffle products");
  return H2G_OK;
}

// ---- vanishing commit (vanishing/prover.rs:40-98), through the y squeeze
int ProofRun::vanishing_commit() {
  {
    const uint64_t at = rng.position();
    std::vector<uint32_t> drawn(van_off.size() * 8, 0);
    for (size_t i = 0; i < van_off.size(); i++) rng.fill(reinterpret_cast<uint8_t*>(&drawn[8 * i]), 32);
    if (van_early && (at != (uint64_t)pk.van_pos || drawn != van_seeds)) {
      // the early draws were not the real ones: drop that commitment, redo it below
      G1Affine unused;
      RCCHK(commit_collect(d, &van_tk, &unused));
      van_early = false;
    }
    if (rng.seeded()) {
      pk.van_pos = (int64_t)at;
      pk.van_T = (uint32_t)van_off.size();
    }
    if (!van_early) {
      van_seeds = drawn;
      HIPCHK(pk_upload(pk, pk.d_seeds.p, van_seeds.data(), van_seeds.size() * 4, st));
      HIPCHK(pk_upload(pk, pk.d_offsets.p, van_off.data(), van_off.size() * 8, st));
      // a slab-mode rank draws only its coefficients (and the halo) of the random polynomial
      HIPCHK(chacha_random_poly(pk.random_poly, n, pk.d_seeds.p, pk.d_offsets.p, (int)van_off.size(), st, sl.lo,
                                sl.hi1));
    }
    (void)rng.random_fr();  // random_blind
    RCCHK(rng_ok());
    if (!van_early) RCCHK(commit_launch(d, prm, pk.random_poly, n, SRS_G, st, &van_tk));
  }
  // the instance columns' cosets do not depend on y: they overlap the permutation /
  // vanishing MSMs (the advice went to coefficients and cosets under its own MSMs)
  for (CircuitWs* w : W)
    RCCHK(ext_cosets(d, pk, (const Fr* const*)w->inst_poly.data(), w->inst_coset.data(), pk.cs.I, st));
  {
    std::vector<MsmTicket*> tl;
    for (auto* tks : {&perm_tk, &lkz_tk, &shz_tk})
      for (auto& t : *tks) tl.push_back(&t);
    tl.push_back(&van_tk);
    RCCHK(collect_write(tl));
  }
  RCCHK(run_deferred());  // (no permutation stage ran them)
  RCCHK(xp_flush(pk, st));  // the overlapped exchanges' rows, before h(X) reads them
  clk.mark("perm+vanishing commits, cosets");
  HIPCHK(xjoin.join());  // the columns' cosets and coefficients (the transform stream)
  ch.y = tr.squeeze();
  return H2G_OK;
}

// ---- evaluate_h (evaluation.rs:317-620): one launch per circuit, each continuing the
// previous circuit's Horner chain in y; the last one divides by t(X)
int ProofRun::eval_h() {
  const bool subc = spmd_subcosets();
  if (pk.cosets) return eval_h_streamed();
  for (int ci = 0; ci < ncirc && !subc; ci++) {
    const CircuitWs& w = *W[ci];
    EvalHArgs a = eval_h_args(ci);
    a.lookups = w.d_lookups;
    a.shuffles = w.d_shuffles;
    a.query_col = w.d_load_col;
    a.z = w.d_z;
    a.perm_v = w.d_perm_v;
    a.sigma = pk.d_sigma;
    a.l0 = pk.l0;
    a.l_last = pk.l_last;
    a.l_active = pk.l_active;
    a.delta_start = beta * zeta();
    a.ext_omega = pk.eo;
    a.ext = ext;
    a.rot_scale = pk.rot_scale;
    a.t_evals = D.d_t.p;
    a.t_mask = D.t_evals.size() - 1;
    a.acc_in = ci > 0 ? pk.h_ext : nullptr;
    a.out = pk.h_ext;
    HIPCHK(evaluate_h(a, st));
  }
  if (subc) {  // rows of this rank's sub-cosets, then every sub-coset's h from its owner
    const int e = (int)(D.ek - D.k);
    for (CircuitWs* w : W) RCCHK(sub_ws_tables(pk, *w));
    for (size_t i = 0; i < pk.sub_ts.size(); i++) {
      const uint64_t t = pk.sub_ts[i];
      Fr* slot = pk.h_gather + t * n;
      for (int ci = 0; ci < ncirc; ci++) {
        const CircuitWs& w = *W[ci];
        EvalHArgs a = eval_h_args(ci);
        a.lookups = w.sub[i].lookups;
        a.shuffles = w.sub[i].shuffles;
        a.query_col = w.sub[i].load_col;
        a.z = w.sub[i].z;
        a.perm_v = w.sub[i].perm_v;
        a.sigma = pk.d_sigma_sub[i];
        a.l0 = pk.sub_l0 + i * n;
        a.l_last = pk.sub_ll + i * n;
        a.l_active = pk.sub_la + i * n;
        a.delta_start = beta * zeta() * pow_u64(D.ext_omega, t);  // X = zeta w_ext^t w^m
        a.ext_omega = pk.om;
        a.ext = n;
        a.rot_scale = 1;
        a.t_evals = D.d_t.p + t;  // t(X) is constant on a sub-coset
        a.t_mask = 0;
        a.acc_in = ci > 0 ? slot : nullptr;
        a.out = slot;
        if (pieces) {  // this rank's rows of the sub-coset
          a.row0 = pk.sub_lo;
          a.rows = pk.sub_hi - pk.sub_lo;
        }
        HIPCHK(evaluate_h(a, st));
      }
    }
    if (h_slabs) {
      if (pieces) RCCHK(h_gather_pieces(pk, st));
      RCCHK(h_by_slabs(d, pk, sl, st));
    } else {
      HIPCHK(hipStreamSynchronize(st));
      for (uint64_t t = 0; t < (1ull << e); t++)
        if (spmd_timed(3, n * sizeof(Fr), [&] {
              return g_spmd.bcast(g_spmd.ctx, pk.h_gather + t * n, n * sizeof(Fr), (int)(t % (uint64_t)g_spmd.world));
            }) != 0)
          return fail(H2G_ERR_STATE, "spmd transport: broadcast of sub-coset " + std::to_string(t) + " failed");
      HIPCHK(subcoset_scatter(pk.h_gather, pk.h_ext, n, e, st));
    }
  }
  if (!h_slabs) dump("h_ext", pk.h_ext, ext, st);
  clk.mark("evaluate_h");
  return H2G_OK;
}

// A streamed key (ProvingKey::cosets): the same evaluation sub-coset by sub-coset.  Row
// t + 2^e m of the extended coset is the point zeta w_ext^t w^m and rotations move rows by
// multiples of 2^e, so evaluate_h on sub-coset t reads sub-coset t of every column -- the
// arguments the SPMD split passes -- and every column array is one n-point slot, refilled for
// each t from its coefficient form: the key's columns once per t for all circuits, then
// circuit by circuit (the slots are shared, so a circuit's transforms follow the previous
// circuit's launch).  All on the prover's stream, one slot set: the transforms and the
// launches alternate, each filling the chip on its own (DESIGN, "Streamed cosets").
int ProofRun::eval_h_streamed() {
  const int e = (int)(D.ek - D.k);
  const Fr one = Fr::one();
  std::vector<const Fr*> ksrc;
  std::vector<Fr*> kdst;
  for (int i = 0; i < pk.cs.F; i++) ksrc.push_back(pk.fixed_poly[i]), kdst.push_back(pk.fixed_coset[i]);
  for (int i = 0; i < pk.cs.P; i++) ksrc.push_back(pk.sigma_poly[i]), kdst.push_back(pk.sigma_coset[i]);
  ksrc.push_back(pk.l0_poly), kdst.push_back(pk.l0);
  ksrc.push_back(pk.l_last_poly), kdst.push_back(pk.l_last);
  ksrc.push_back(pk.l_blind_poly), kdst.push_back(pk.l_active);  // l_blind, then 1 - l_last - l_blind in place
  std::vector<std::vector<const Fr*>> csrc(ncirc);
  std::vector<std::vector<Fr*>> cdst(ncirc);
  for (int ci = 0; ci < ncirc; ci++) {
    const CircuitWs& w = *W[ci];
    auto add = [&](const std::vector<Fr*>& polys, const std::vector<Fr*>& slots) {
      for (size_t i = 0; i < polys.size(); i++) csrc[ci].push_back(polys[i]), cdst[ci].push_back(slots[i]);
    };
    add(w.adv_poly, w.adv_coset);
    add(w.inst_poly, w.inst_coset);
    add(w.z, w.z_coset);
    add(w.lk_ap_poly, w.lk_apc);
    add(w.lk_sp_poly, w.lk_spc);
    add(w.lk_z_poly, w.lk_zc);
    add(w.sh_z_poly, w.sh_zc);
  }
  for (uint64_t t = 0; t < (1ull << e); t++) {
    RCCHK(coeff_to_subcoset_batch(d, D, ksrc.data(), kdst.data(), (int)ksrc.size(), t, st));
    HIPCHK(poly_binop(POLY_ADD, pk.l_last, pk.l_active, one, pk.l_active, n, st));
    HIPCHK(poly_binop(POLY_SUB_CONST, pk.l_active, nullptr, one, pk.l_active, n, st));
    HIPCHK(poly_binop(POLY_SCALE, pk.l_active, nullptr, fr_neg_one(), pk.l_active, n, st));
    Fr* slot = pk.h_gather + t * n;
    for (int ci = 0; ci < ncirc; ci++) {
      const CircuitWs& w = *W[ci];
      RCCHK(coeff_to_subcoset_batch(d, D, csrc[ci].data(), cdst[ci].data(), (int)csrc[ci].size(), t, st));
      EvalHArgs a = eval_h_args(ci);
      a.lookups = w.d_lookups;  // the tables of circuit_ws_add: their columns are the slots
      a.shuffles = w.d_shuffles;
      a.query_col = w.d_load_col;
      a.z = w.d_z;
      a.perm_v = w.d_perm_v;
      a.sigma = pk.d_sigma;
      a.l0 = pk.l0;
      a.l_last = pk.l_last;
      a.l_active = pk.l_active;
      a.delta_start = beta * zeta() * pow_u64(D.ext_omega, t);  // X = zeta w_ext^t w^m
      a.ext_omega = pk.om;
      a.ext = n;
      a.rot_scale = 1;
      a.t_evals = D.d_t.p + t;  // t(X) is constant on a sub-coset
      a.t_mask = 0;
      a.acc_in = ci > 0 ? slot : nullptr;
      a.out = slot;
      HIPCHK(evaluate_h(a, st));
    }
  }
  HIPCHK(subcoset_scatter(pk.h_gather, pk.h_ext, n, e, st));
  dump("h_ext", pk.h_ext, ext, st);
  clk.mark("evaluate_h");
  return H2G_OK;
}

// ---- vanishing construct (vanishing/prover.rs:102-155): h(X) pieces of size n (a rank
// that received h by slabs holds its slab of each piece already)
int ProofRun::h_commit() {
  if (!h_slabs) RCCHK(extended_to_coeff(d, D, pk.h_ext, pk.h_coeff, st));
  const int npieces = pk.cs.degree - 1;
  for (int p = 0; p < npieces; p++) (void)rng.random_fr();  // h blinds
  RCCHK(rng_ok());
  {
    std::vector<MsmTicket> tk(npieces);
    std::vector<const Fr*> h_pieces(npieces);
    for (int p = 0; p < npieces; p++) h_pieces[p] = pk.h_coeff + (size_t)p * n;
    RCCHK(commit_launch_batch(d, prm, h_pieces.data(), npieces, n, SRS_G, st, tk.data()));
    std::vector<MsmTicket*> tl;
    for (int p = 0; p < npieces; p++) tl.push_back(&tk[p]);
    RCCHK(collect_write(tl));
  }
  clk.mark("h commit");
  ch.x = tr.squeeze();
  const Fr xn = pow_u64(x, n);
  // h(X) = sum_p X^(n p) h_p(X)  (vanishing/prover.rs:166-170)
  {
    LinTerms t;
    Fr c = Fr::one();
    bool first = true;
    for (int p = 0; p < npieces; p++) {
      if (t.k == LIN_MAXT) {
        RCCHK(lincomb_range(pk.h_poly, sl.lo, sl.hi1, t, !first, st));  // a slab rank: its slab + halo
        first = false;
        t.k = 0;
      }
      t.p[t.k] = pk.h_coeff + (size_t)p * n;
      t.len[t.k] = n;
      t.coef[t.k] = c;
      t.k++;
      c = c * xn;
    }
    RCCHK(lincomb_range(pk.h_poly, sl.lo, sl.hi1, t, !first, st));
  }
  return H2G_OK;
}

// ---- the polynomial openings (prover.rs:840-889) and their evaluations
int ProofRun::openings_and_evals() {
  for (const CircuitWs* w : W) {
    for (int c = 0; c < pk.cs.A; c++) polys.push_back({w->adv_poly[c], n});
    for (int s = 0; s < pk.cs.nsets; s++) polys.push_back({w->z[s], n});
    for (int l = 0; l < pk.cs.NL; l++) {
      polys.push_back({w->lk_z_poly[l], n});
      polys.push_back({w->lk_ap_poly[l], n});
      polys.push_back({w->lk_sp_poly[l], n});
    }
    for (int s = 0; s < pk.cs.NS; s++) polys.push_back({w->sh_z_poly[s], n});
  }
  const int id_fix = (int)polys.size();
  if (coef_send || coef_recv) {  // the per-circuit coefficient columns' slabs, owners -> the others
    std::vector<Fr*> cols;     // (the columns of wide stages reached every rank from their owners)
    for (int ci = 0; ci < ncirc; ci++)
      for (int i = 0; i < per_c; i++) {
        if (i < pk.cs.A && adv_shard[(size_t)ci * pk.cs.A + i]) continue;
        if (lk_shard && i >= pk.cs.A + pk.cs.nsets && i < pk.cs.A + pk.cs.nsets + 3 * pk.cs.NL) continue;
        cols.push_back(const_cast<Fr*>(polys[(size_t)ci * per_c + i].p));
      }
    RCCHK(coef_exchange(pk, cols, st));
  }
  for (int c = 0; c < pk.cs.F; c++) polys.push_back({pk.fixed_poly[c], n});
  const int id_sig = (int)polys.size();
  for (int c = 0; c < pk.cs.P; c++) polys.push_back({pk.sigma_poly[c], n});
  const int id_h = (int)polys.size();
  polys.push_back({pk.h_poly, n});
  const int id_r = (int)polys.size();
  polys.push_back({pk.random_poly, n});
  const Fr x_next = rotate_omega(D, x, 1), x_last = rotate_omega(D, x, -(bf + 1));
  const Fr x_prev = rotate_omega(D, x, -1);
  for (int ci = 0; ci < ncirc; ci++) {  // per circuit: advice, permutation, lookups, shuffles
    for (auto& q : pk.cs.adv_q) queries.push_back({id_adv(ci) + q.index, rotate_omega(D, x, q.rot)});
    for (int s = 0; s < pk.cs.nsets; s++) {  // permutation/prover.rs:300-333
      queries.push_back({id_z(ci) + s, x});
      queries.push_back({id_z(ci) + s, x_next});
    }
    for (int s = pk.cs.nsets - 2; s >= 0; s--) queries.push_back({id_z(ci) + s, x_last});
    for (int l = 0; l < pk.cs.NL; l++) {  // lookup/prover.rs:364-405
      const int zi = id_lk(ci) + 3 * l;
      queries.push_back({zi, x});
      queries.push_back({zi + 1, x});
      queries.push_back({zi + 2, x});
      queries.push_back({zi + 1, x_prev});
      queries.push_back({zi, x_next});
    }
    for (int s = 0; s < pk.cs.NS; s++) {  // shuffle/prover.rs:234-254
      queries.push_back({id_sh(ci) + s, x});
      queries.push_back({id_sh(ci) + s, x_next});
    }
  }
  for (auto& q : pk.cs.fix_q) queries.push_back({id_fix + q.index, rotate_omega(D, x, q.rot)});
  for (int c = 0; c < pk.cs.P; c++) queries.push_back({id_sig + c, x});
  queries.push_back({id_h, x});
  queries.push_back({id_r, x});
  ev_of.resize(polys.size());
  for (auto& q : queries) ev_index(q.poly, q.pt);
  evals.resize(ev_keys.size());
  {
    const int nreq = (int)ev_keys.size();
    HIPCHK(pk.d_reqs.ensure(nreq));
    HIPCHK(pk.evals.ensure(nreq));
    HIPCHK(pk.eval_scr.ensure(poly_eval_scratch_len(nreq, n)));
    std::vector<EvalReq> reqs(nreq);
    for (int i = 0; i < nreq; i++) {  // a slab rank evaluates its coefficients [lo, hi) only
      const PolyRef& pr = polys[ev_keys[i].poly];
      const uint64_t len = pr.len > sl.lo ? std::min<uint64_t>(pr.len, sl.hi) - sl.lo : 0;
      reqs[i] = EvalReq{pr.p + (len ? sl.lo : 0), len, ev_keys[i].pt};
    }
    HIPCHK(pk_upload(pk, pk.d_reqs.p, reqs.data(), nreq * sizeof(EvalReq), st));
    HIPCHK(poly_eval_batch(pk.d_reqs.p, nreq, sl.hi - sl.lo, pk.evals.p, pk.eval_scr.p, st));
    HIPCHK(hipMemcpyAsync(evals.data(), pk.evals.p, nreq * sizeof(Fr), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (slabs) {  // p(x) = sum_r x^lo_r (slab r's partial evaluation), summed in rank order
      std::vector<std::pair<Fr, Fr>> shift;  // (point, point^lo): a few distinct points
      for (int i = 0; i < nreq; i++) {
        const Fr& pt = ev_keys[i].pt;
        size_t j = 0;
        while (j < shift.size() && !(shift[j].first == pt)) j++;
        if (j == shift.size()) shift.emplace_back(pt, pow_u64(pt, sl.lo));
        evals[i] = evals[i] * shift[j].second;
      }
      std::vector<Fr> all;
      RCCHK(spmd_allgather_fr(evals, &all));
      for (int i = 0; i < nreq; i++) {
        Fr acc = Fr::zero();
        for (int r = 0; r < g_spmd.world; r++) acc = acc + all[(size_t)r * nreq + i];
        evals[i] = acc;
      }
    }
  }
  for (int ci = 0; ci < ncirc; ci++)  // [TRANSCRIPT-17] every circuit's advice evaluations
    for (auto& q : pk.cs.adv_q) tr.write_scalar(ev(id_adv(ci) + q.index, rotate_omega(D, x, q.rot)));
  for (auto& q : pk.cs.fix_q) tr.write_scalar(ev(id_fix + q.index, rotate_omega(D, x, q.rot)));
  tr.write_scalar(ev(id_r, x));
  for (int c = 0; c < pk.cs.P; c++) tr.write_scalar(ev(id_sig + c, x));
  for (int ci = 0; ci < ncirc; ci++)
    for (int s = 0; s < pk.cs.nsets; s++) {
      tr.write_scalar(ev(id_z(ci) + s, x));
      tr.write_scalar(ev(id_z(ci) + s, x_next));
      if (s + 1 < pk.cs.nsets) tr.write_scalar(ev(id_z(ci) + s, x_last));
    }
  for (int ci = 0; ci < ncirc; ci++)
    for (int l = 0; l < pk.cs.NL; l++) {  // product, product_next, A', A'_inv, S' (lookup/prover.rs:330-361)
      const int zi = id_lk(ci) + 3 * l;
      tr.write_scalar(ev(zi, x));
      tr.write_scalar(ev(zi, x_next));
      tr.write_scalar(ev(zi + 1, x));
      tr.write_scalar(ev(zi + 1, x_prev));
      tr.write_scalar(ev(zi + 2, x));
    }
  for (int ci = 0; ci < ncirc; ci++)
    for (int s = 0; s < pk.cs.NS; s++) {
      tr.write_scalar(ev(id_sh(ci) + s, x));
      tr.write_scalar(ev(id_sh(ci) + s, x_next));
    }
  clk.mark("evaluations");
  return H2G_OK;
}

// ---- the multi-open argument (multiopen.cpp) over this proof's polynomials, queries and
// evaluations, with the proving key's scratch
MultiopenCtx ProofRun::multiopen_ctx() {
  MultiopenCtx c;
  c.d = d;
  c.prm = &prm;
  c.st = st;
  c.tr = &tr;
  c.n = n;
  c.polys = &polys;
  c.queries = &queries;
  c.ev = [this](int poly, const Fr& pt) { return ev(poly, pt); };
  c.nx = pk.nx, c.hx = pk.hx, c.lx = pk.lx, c.q1 = pk.q1, c.scr = pk.scr, c.small = pk.small;
  c.gwc_q = &pk.gwc_q;
  c.pool = &pk.pool;
  c.upload = [this](void* dst, const void* src, size_t bytes) { return pk_upload(pk, dst, src, bytes, st); };
  c.mark = [this](const char* name) { clk.mark(name); };
  c.slabs = slabs;
  c.sl = sl;
  c.slab_pk = &pk;
  return c;
}
int ProofRun::gwc() {
  MultiopenCtx c = multiopen_ctx();
  return multiopen_gwc(c);
}
int ProofRun::shplonk() {
  MultiopenCtx c = multiopen_ctx();
  return multiopen_shplonk(c);
}

// row pieces: the advice transforms run in the permutation stage when every transform of
// the proof has a rank of its own (prove_impl; keeping them in the advice stage: measured,
// rejected)
// Single-GPU proofs: the columns' transforms (lagrange_to_coeff, the coset extension) on a
// stream of their own (Device::xstream), joined before evaluate_h, their first reader.
// On the prover's stream they held back every later stage's kernels -- the lookups'
// sorts and grand products are chains of small launches that leave most of the chip idle,
// and ran only after the 2^20-point transforms ahead of them on the stream (keccak-style
// k = 18: the same 33.1 ms with every stage drained as without; 31.8-32.4 vs 33.3-34.3 ms
// on their own stream, profiles/r06/xs/ab_ordered_streams.log).  Only for circuits with
// lookups or shuffles: C3 (no lookups; its stages are MSM-bound, the chip already full)
// measured 76.1-77.3 vs 73.1-73.8 ms with it.  The stream is created by the first proof
// that uses it, after the MSM streams (the hardware-queue order matters, abi.cpp).  Stream
// priorities (transforms low, or MSMs high) measured slower (profiles/r06/xs/).
int prove_impl(Device* d, Params& prm, ProvingKey& pk, const ProveIn& in, std::vector<uint8_t>* proof) {
  hipStream_t st = d->stream;
  if (pk.cosets && g_spmd.world > 1)
    return fail(H2G_ERR_STATE, "create_proof: a streamed-coset key does not prove under an SPMD transport of " +
                                   std::to_string(g_spmd.world) + " ranks (make the key with H2G_COSETS_RESIDENT)");
  xp_drain(pk);  // a failed proof's overlapped exchanges
  RCCHK(pk_upload_arm(pk, st));
  while ((int)pk.cws.size() < in.nc) RCCHK(circuit_ws_add(pk));  // workspaces grow once
  // with the slab exchange and world a multiple of 2^e above it, every rank takes a row
  // piece of one sub-coset (sub_prepare)
  const int E_sub = 1 << (pk.dom.ek - pk.dom.k);
  const bool pieces = spmd_subcosets() && g_spmd.allgather_host && g_spmd.exchange && pk.multiopen == 0 &&
                      g_spmd_colshard && g_spmd.world >= kColshardMinWorld && g_spmd.world > E_sub &&
                      g_spmd.world % E_sub == 0;
  if (spmd_subcosets()) RCCHK(sub_prepare(pk, st, pieces));  // this rank's sub-cosets of the key's cosets
  const bool xsplit = g_spmd.world <= 1 && !spmd_subcosets() && pk.cs.NL + pk.cs.NS > 0;
  if (xsplit && !d->xstream) {  // after the MSM streams (h2g_init): the hardware-queue order, abi.cpp
    HIPCHK(hipStreamCreateWithFlags(&d->xstream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&d->xev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&d->xev_done, hipEventDisableTiming));
  }
  ProofRun run(d, prm, pk, in, proof, E_sub, pieces, xsplit);
  RCCHK(run.instances());
  RCCHK(run.advice_phases());
  RCCHK(run.lookup_permuted());
  RCCHK(run.permutation_products());
  RCCHK(run.lookup_shuffle_products());
  RCCHK(run.vanishing_commit());
  RCCHK(run.eval_h());
  RCCHK(run.h_commit());
  RCCHK(run.openings_and_evals());
  return pk.multiopen == 1 ? run.gwc() : run.shplonk();
}

// the checks and output handling every create_proof entry point shares
int create_proof_entry(Device* d, uint64_t params, uint64_t pk, ProveIn& in, uint8_t* proof, size_t proof_cap,
                       size_t* proof_len) {
  Params* ip = find_params(params);
  if (!ip) return fail(H2G_ERR_HANDLE, "unknown params");
  ProvingKey* ik = find_pk(pk);
  if (!ik) return fail(H2G_ERR_HANDLE, "unknown proving key");
  ProvingKey& K = *ik;
  if (K.params != params) return fail(H2G_ERR_ARG, "create_proof: pk was generated with other params");
  if (K.device != d->id) return fail(H2G_ERR_ARG, "create_proof: pk lives on another device");
  if (!proof_len || in.nc < 1 || in.nc > 1024) return fail(H2G_ERR_ARG, "create_proof: bad arguments");
  for (int c = 0; c < in.nc; c++) {
    if (K.cs.A && !in.src && !in.src1 && !in.asg && (!in.advice || !in.advice[c])) return fail(H2G_ERR_ARG, "create_proof: null advice");
    if (K.cs.I && (!in.instance || !in.inst_lens || !in.instance[c] || !in.inst_lens[c]))
      return fail(H2G_ERR_ARG, "create_proof: null instance");  // InvalidInstances
  }
  std::vector<uint8_t> out;
  out.reserve(32 * 256);
  int rc = prove_impl(d, *ip, K, in, &out);
  if (rc) {
    (void)hipStreamSynchronize(d->stream);
    return rc;
  }
  *proof_len = out.size();
  if (out.size() > proof_cap) return fail(H2G_ERR_ARG, "create_proof: proof buffer too small");
  if (proof) std::memcpy(proof, out.data(), out.size());
  return H2G_OK;
}

}  // namespace

extern "C" {

int h2g_create_proof(uint64_t params, uint64_t pk, const uint64_t* advice, int advice_on_device,
                     const uint64_t* instance, const uint32_t* instance_lens, const uint8_t rng_seed[32],
                     uint32_t vanishing_threads, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  NEED_DEV_P();
  if (!rng_seed) return fail(H2G_ERR_ARG, "create_proof: null rng seed");
  ProverRng rng(rng_seed);
  ProveIn in;
  in.advice = &advice;
  in.adv_dev = advice_on_device != 0;
  in.instance = &instance;
  in.inst_lens = &instance_lens;
  in.rng = &rng;
  in.vthreads = vanishing_threads;
  return create_proof_entry(d, params, pk, in, proof, proof_cap, proof_len);
}

int h2g_create_proof_phased(uint64_t params, uint64_t pk, const h2g_witness_source* witness,
                            const uint64_t* instance, const uint32_t* instance_lens, const uint8_t rng_seed[32],
                            uint32_t vanishing_threads, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  NEED_DEV_P();
  if (!rng_seed || !witness || !witness->fill) return fail(H2G_ERR_ARG, "create_proof: null argument");
  ProverRng rng(rng_seed);
  ProveIn in;
  in.src1 = witness;
  in.instance = &instance;
  in.inst_lens = &instance_lens;
  in.rng = &rng;
  in.vthreads = vanishing_threads;
  return create_proof_entry(d, params, pk, in, proof, proof_cap, proof_len);
}

int h2g_create_proof_multi(uint64_t params, uint64_t pk, const h2g_prove_inputs* p, uint8_t* proof,
                           size_t proof_cap, size_t* proof_len) {
  NEED_DEV_P();
  if (!p || p->num_circuits < 1) return fail(H2G_ERR_ARG, "create_proof: no circuits");
  if (p->witness && !p->witness->fill) return fail(H2G_ERR_ARG, "create_proof: null witness fill");
  if (!p->rng && !p->rng_seed) return fail(H2G_ERR_ARG, "create_proof: neither an rng nor a seed");
  // fill_bytes is required: the vanishing argument's ChaCha seeds are fill_bytes draws
  // (vanishing/prover.rs:69-73) whatever F::random uses
  if (p->rng && !p->rng->fill_bytes) return fail(H2G_ERR_ARG, "create_proof: the caller's rng needs fill_bytes");
  std::unique_ptr<ProverRng> rng = p->rng ? std::make_unique<ProverRng>(p->rng->fill_bytes, p->rng->random_fr, p->rng->ctx)
                                          : std::make_unique<ProverRng>(p->rng_seed);
  ProveIn in;
  in.nc = (int)std::min<uint32_t>(p->num_circuits, 1u << 20);
  in.advice = p->advice;
  in.adv_dev = p->advice_on_device != 0;
  in.src = p->witness;
  in.instance = p->instance;
  in.inst_lens = p->instance_lens;
  in.rng = rng.get();
  in.vthreads = p->vanishing_threads;
  return create_proof_entry(d, params, pk, in, proof, proof_cap, proof_len);
}

int h2g_create_proof_assigned(uint64_t params, uint64_t pk, const h2g_prove_inputs* p,
                              const h2g_assigned_source* source, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  NEED_DEV_P();
  if (!p || p->num_circuits < 1) return fail(H2G_ERR_ARG, "create_proof: no circuits");
  if (!source || !source->fill) return fail(H2G_ERR_ARG, "create_proof_assigned: null source");
  if (p->advice || p->witness)
    return fail(H2G_ERR_ARG, "create_proof_assigned: the witness comes from `source`; advice and witness must be NULL");
  if (!p->rng && !p->rng_seed) return fail(H2G_ERR_ARG, "create_proof: neither an rng nor a seed");
  if (p->rng && !p->rng->fill_bytes) return fail(H2G_ERR_ARG, "create_proof: the caller's rng needs fill_bytes");
  std::unique_ptr<ProverRng> rng = p->rng ? std::make_unique<ProverRng>(p->rng->fill_bytes, p->rng->random_fr, p->rng->ctx)
                                          : std::make_unique<ProverRng>(p->rng_seed);
  ProveIn in;
  in.nc = (int)std::min<uint32_t>(p->num_circuits, 1u << 20);
  in.asg = source;
  in.instance = p->instance;
  in.inst_lens = p->instance_lens;
  in.rng = rng.get();
  in.vthreads = p->vanishing_threads;
  return create_proof_entry(d, params, pk, in, proof, proof_cap, proof_len);
}

// a ChaCha20Rng::from_seed (rand_chacha 0.3) behind the h2g_rng callbacks: the RngCore
// a Rust host passes to create_proof, here native -- the caller-RNG path of
// h2g_create_proof_multi (no early vanishing commitment) with the seeded path's bytes
std::map<uint64_t, std::unique_ptr<ChaChaRng>> g_rngs;
int rng_fill_cb(void* ctx, uint8_t* out, size_t len) {
  static_cast<ChaChaRng*>(ctx)->fill(out, len);
  return 0;
}
int h2g_rng_chacha20(const uint8_t seed[32], h2g_rng* out, uint64_t* handle) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!seed || !out || !handle) return fail(H2G_ERR_ARG, "rng_chacha20: null argument");
  auto r = std::make_unique<ChaChaRng>(seed);
  out->ctx = r.get();
  out->fill_bytes = rng_fill_cb;
  out->random_fr = nullptr;
  *handle = g_next_handle++;
  g_rngs[*handle] = std::move(r);
  return H2G_OK;
}
int h2g_rng_free(uint64_t handle) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!g_rngs.erase(handle)) return fail(H2G_ERR_HANDLE, "rng_free: unknown handle");
  return H2G_OK;
}

int h2g_last_challenges(uint64_t* out, int max, int* count) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!count) return fail(H2G_ERR_ARG, "last_challenges: null count");
  *count = (int)g_last_challenges.size();
  if (out)
    for (int i = 0; i < *count && i < max; i++) std::memcpy(out + 4 * i, &g_last_challenges[i], sizeof(Fr));
  return H2G_OK;
}

int h2g_prover_stage_sync(int on) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  g_stage_sync = on != 0;
  return H2G_OK;
}

int h2g_prover_stages(double* ms, int max, int* count) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  const int c = (int)g_stages.size();
  for (int i = 0; i < c && i < max; i++) ms[i] = g_stages[i].second;
  if (count) *count = c;
  return H2G_OK;
}

const char* h2g_prover_stage_name(int i) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (i < 0 || i >= (int)g_stages.size()) return "";
  return g_stages[i].first;
}

}  // extern "C"
