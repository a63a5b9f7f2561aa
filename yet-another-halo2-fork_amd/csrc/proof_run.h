// proof_run.h -- one create_proof in flight (internal: prover.cpp, which defines the stages,
// prover_lookup.cpp, the lookup argument's permutation, and prover_selfcheck.cpp, the
// self-checks): the proof's inputs, the column
// sets its stages transform, ProofRun and LookupPermute.
#pragma once
#include "assigned.h"
#include "multiopen.h"

namespace h2g {
namespace prv {

extern std::vector<std::pair<const char*, double>> g_stages;  // prover.cpp (h2g_prover_stages)
extern bool g_stage_sync;  // h2g_prover_stage_sync: stage times = GPU completion times
void self_check_reset();   // prover_selfcheck.cpp: h2g_last_self_check reports nothing

// Debug aid: a build with -DH2G_DUMP_DIR='"<dir>"' writes named intermediates (raw Fr
// arrays) of create_proof to <dir>/p<pid>/<name>.bin, one directory per process (rank); no
// run-time switch in the shipped library
inline void dump(const char* name, const Fr* dptr, size_t count, hipStream_t st, bool host = false) {
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

// several blocks of blinding rows in one upload and one copy launch: `host` (count Fr) lands
// in pk.blind_d.p (sized by the caller, before it built `segs`), which `segs` read from.  Every small host-to-device copy is a ~6-us blit
// on the stream; a keccak-style proof made ~80 of them, one per column and lookup side
inline int upload_rows_batch(ProvingKey& pk, const Fr* host, size_t count, const std::vector<CopySeg>& segs,
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

// A set of columns a stage transforms: per column its Lagrange form, its coefficient form
// and its extended-domain coset, in the stage's (transcript) order
struct Cols {
  std::vector<const Fr*> lag;
  std::vector<Fr*> pol, cst;
  void add(const Fr* l, Fr* p, Fr* c) { lag.push_back(l), pol.push_back(p), cst.push_back(c); }
  void add(const std::vector<Fr*>& l, const std::vector<Fr*>& p, const std::vector<Fr*>& c) {
    for (size_t i = 0; i < l.size(); i++) add(l[i], p[i], c[i]);
  }
  int size() const { return (int)lag.size(); }
  // one circuit's columns of a kind
  void advice(const CircuitWs& w, const std::vector<int>& cols) {
    for (int c : cols) add(w.adv[c], w.adv_poly[c], w.adv_coset[c]);
  }
  void z(const CircuitWs& w) { add(w.z_lag, w.z, w.z_coset); }
  void lookup_permuted(const CircuitWs& w) {  // (A'_l, S'_l) in transcript order
    for (size_t l = 0; l < w.lk_ap.size(); l++) {
      add(w.lk_ap[l], w.lk_ap_poly[l], w.lk_apc[l]);
      add(w.lk_sp[l], w.lk_sp_poly[l], w.lk_spc[l]);
    }
  }
  void lookup_z(const CircuitWs& w) { add(w.lk_z, w.lk_z_poly, w.lk_zc); }
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
    hipStream_t st, xst;
    bool pending = false;
    bool begun = false;  // xs_begin without its xs_end: a transform failed part-way
    hipError_t join() {
      if (begun) {  // what the failed transform did queue on xst is waited for as well
        begun = false;
        if (hipEventRecord(d->xev_done, xst) == hipSuccess) pending = true;
      }
      if (!pending) return hipSuccess;
      pending = false;
      return hipStreamWaitEvent(st, d->xev_done, 0);
    }
    ~XformJoin() { (void)join(); }
  };
  XformJoin xjoin{d, st, xst};
  int xs_begin() {
    if (xst == st) return H2G_OK;
    HIPCHK(hipEventRecord(d->xev_in, st));
    HIPCHK(hipStreamWaitEvent(xst, d->xev_in, 0));
    xjoin.begun = true;
    return H2G_OK;
  }
  int xs_end() {
    if (xst == st) return H2G_OK;
    HIPCHK(hipEventRecord(d->xev_done, xst));
    xjoin.begun = false;
    xjoin.pending = true;
    return H2G_OK;
  }
  // the rotation's owners of the next M columns
  std::vector<int> next_owners(int M) {
    std::vector<int> o(M);
    for (int i = 0; i < M; i++) o[i] = (tr_next + i) % Wsp;
    tr_next += M;
    return o;
  }
  // (a rank that receives its coefficients, coef_recv, queues nothing here: it owns no
  // sub-coset, so ext_cosets has nothing to launch, and under SPMD xst is st)
  int xform(const Cols& c, const std::vector<int>* own) {
    const int M = c.size();
    if (M == 0) return H2G_OK;
    if (own || pieces) return colshard_distribute(d, pk, c.lag, c.pol, c.cst, own ? *own : next_owners(M), st);
    RCCHK(xs_begin());
    if (!coef_recv) RCCHK(lagrange_to_coeff_batch(d, D, c.lag.data(), c.pol.data(), M, xst));
    RCCHK(ext_cosets(d, pk, (const Fr* const*)c.pol.data(), c.cst.data(), M, xst));
    return xs_end();
  }
  // with row pieces the advice columns' transforms wait for the permutation stage: at the
  // advice commitments' all-gather every rank would otherwise wait for the ranks that
  // transform an advice column (their slab partials come late), and in the permutation
  // stage the ranks without a grand product's transform are idle -- run there, the advice
  // transforms overlap the products' (the owners are fixed here, in the same rotation)
  struct DeferredXform {
    Cols cols;
    std::vector<int> own;
  };
  std::vector<DeferredXform> deferred;
  // (the column transforms of the whole proof, an upper bound, against the ranks that are
  // not sub-coset leaders: C3 at 8 ranks has 3 advice + 3 grand products for 6 ranks; at 4
  // ranks two transforms would share a rank in the permutation stage, measured slower:
  // profiles/r05/emulation/defer_adv/)
  const int n_xf = ncirc * (pk.cs.A + pk.cs.nsets + 3 * pk.cs.NL + pk.cs.NS);
  const bool defer_adv = pieces && n_xf <= Wsp - E_sub;
  void xform_later(const Cols& c) { deferred.push_back(DeferredXform{c, next_owners(c.size())}); }
  int run_deferred() {
    for (DeferredXform& x : deferred) RCCHK(xform(x.cols, &x.own));
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
  // a stage's commitments, each column its owner's (own) or every rank's slab of it
  int commit_stage(const Fr* const* cols, int m, const std::vector<int>* own, int srs_set, MsmTicket* tk) {
    if (own) return commit_launch_owned(d, prm, cols, own->data(), m, n, srs_set, st, tk);
    return commit_launch_batch(d, prm, cols, m, n, srs_set, st, tk);
  }
  // ... collected together (one SPMD all-gather) and written in order: the sets' tickets, then `last`
  int collect_write(std::initializer_list<std::vector<MsmTicket>*> sets, MsmTicket* last = nullptr) {
    std::vector<MsmTicket*> tks;
    for (std::vector<MsmTicket>* s : sets)
      for (MsmTicket& t : *s) tks.push_back(&t);
    if (last) tks.push_back(last);
    std::vector<G1Affine> cms(tks.size());
    RCCHK(commit_collect_all(d, tks.data(), (int)tks.size(), cms.data()));
    for (const G1Affine& cm : cms) RCCHK(write_point(cm));
    return H2G_OK;
  }
  // blinding rows into host staging; the commitment blinds the reference draws after them
  // (unused by KZG) stay at the call sites, where the draw order can be read
  void draw_rows(Fr* rows, int count) {
    for (int i = 0; i < count; i++) rows[i] = rng.random_fr();
  }
  int assigned_convert(int ci, int ph, const std::vector<int>& cols, CircuitWs& w, const h2g_assigned_dens& dn);
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
  int launch_van_early();
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
  Cols all_z;  // every circuit's grand products, circuit-major
  const Fr* col_vals(const CircuitWs& w, int c) const {
    const auto& pc = pk.cs.perm_cols[c];
    return pc.first == COL_ADVICE ? w.adv[pc.second]
                                  : (pc.first == COL_FIXED ? pk.fixed_lag[pc.second] : w.inst_val[pc.second]);
  }
  // Set i = ci * nsets + s of the proof (circuit ci's set s) on rows [row0, row0 + len),
  // PERM_MAXC columns a launch: its denominators (values, sigma) or its numerators (values,
  // beta delta^c -- column c of the circuit's permutation takes delta^c, so the chain of a
  // circuit runs on through its sets) into z (which starts at row0)
  int perm_set(int i, bool numerators, Fr* z, size_t row0, size_t len) {
    const int ci = i / pk.cs.nsets, s = i % pk.cs.nsets;
    const int c0 = s * pk.cs.chunk_len, c1 = std::min(c0 + pk.cs.chunk_len, pk.cs.P);
    Fr deltaomega = pow_u64(fr_delta(), (uint64_t)c0);
    for (int c = c0; c < c1 && len; c += PERM_MAXC) {
      PermCols pc;
      pc.m = std::min(PERM_MAXC, c1 - c);
      for (int j = 0; j < pc.m; j++) {
        pc.v[j] = col_vals(*W[ci], c + j) + row0;
        if (numerators) {
          pc.beta_delta[j] = deltaomega * beta;
          deltaomega = deltaomega * fr_delta();
        } else {
          pc.sigma[j] = pk.sigma_lag[c + j] + row0;
        }
      }
      if (numerators) HIPCHK(perm_numerators(z, len, pc, gamma, pk.om, st, row0));
      else HIPCHK(perm_denominators(z, len, pc, beta, gamma, c == c0, st));
    }
    return H2G_OK;
  }
  const int NSH = ncirc * pk.cs.NS;
  std::vector<MsmTicket> lkz_tk = std::vector<MsmTicket>(NLT), shz_tk = std::vector<MsmTicket>(NSH);
  // the evaluate_h arguments but the domain's (whole cosets or one sub-coset) and the
  // output, which the caller fills.  tb, sigma: the pointer tables whose columns hold that
  // domain; l0, l_last, l_active: its rows of them
  EvalHArgs eval_h_args(int ci, const CircuitWs::SubTables& tb, const Fr** sigma, const Fr* l0, const Fr* l_last,
                        const Fr* l_active) const {
    EvalHArgs a;
    a.lookups = tb.lookups;
    a.shuffles = tb.shuffles;
    a.query_col = tb.load_col;
    a.z = tb.z;
    a.perm_v = tb.perm_v;
    a.sigma = sigma;
    a.l0 = l0;
    a.l_last = l_last;
    a.l_active = l_active;
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
  // ... all of them for sub-coset t into `slot` (the SPMD split's and a streamed key's):
  // row m is the point zeta w_ext^t w^m.  window: this rank's row piece only
  EvalHArgs eval_h_sub(int ci, uint64_t t, Fr* slot, const CircuitWs::SubTables& tb, const Fr** sigma,
                       const Fr* l0, const Fr* l_last, const Fr* l_active, bool window) const {
    EvalHArgs a = eval_h_args(ci, tb, sigma, l0, l_last, l_active);
    a.delta_start = beta * zeta() * pow_u64(D.ext_omega, t);  // X = zeta w_ext^t w^m
    a.ext_omega = pk.om;
    a.ext = n;
    a.rot_scale = 1;
    a.t_evals = D.d_t.p + t;  // t(X) is constant on a sub-coset
    a.t_mask = 0;
    a.acc_in = ci > 0 ? slot : nullptr;
    a.out = slot;
    if (window) {
      a.row0 = pk.sub_lo;
      a.rows = pk.sub_hi - pk.sub_lo;
    }
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
  // the self-checks (prover_selfcheck.cpp; pk.self_check, fixed for the run): mode 2's checks
  // queue behind the kernels that made what they read, into circuit ci's record sink; the
  // verdict (and, when it fails, the location) follows openings_and_evals
  const int sc_mode = pk.self_check;
  static constexpr size_t SC_REC_CAP = 4096;  // records kept per circuit; the totals stay exact
  CheckSink sc_sink(int ci) const;
  int self_check_begin();
  int sc_unusable_rows(int ci, const std::vector<int>& cols);
  int sc_lookup_permuted();
  int sc_permutation(int i);
  int sc_product(int ci, uint32_t index, const Fr* z, const Fr* num_a, const Fr* num_b, const Fr* den_a,
                 const Fr* den_b);
  int self_check();
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

// permute_expression_pair (lookup/prover.rs:410-494) for every (circuit, lookup) pair j of a
// proof: sort by Ord (canonical value), match, fill leftovers -- lookup j's A' and S' into
// its circuit's lk_ap / lk_sp (prover_lookup.cpp).
// Every lookup's two columns go through ONE radix sort (radix.hip): column g = 2 j + side
// keys on a 48-bit window of its canonical values -- bits [hb - 48, hb) below the value
// width hb the previous proof measured for that lookup (lk_hb) -- with g above the
// window, so each column's rows come out contiguous and sorted.  The gather of the
// canonical values checks the order (a window that tied different values); a lookup
// whose check or width failed, or whose width is unknown (hb 0), is sorted in full
// (four stable 64-bit limb sorts, least significant first).
struct LookupPermute {
  ProofRun& r;
  ProvingKey& pk = r.pk;
  const hipStream_t st = r.st;
  const size_t u = r.unusable;
  const int NLT = r.NLT, NL = r.pk.cs.NL;
  static constexpr int LKC = ProvingKey::LKC, LKF = ProvingKey::LKF;
  // a wide lookup stage: lookup j is rank j mod world's (its compression, sort, match and
  // fill, commitments and transforms); every rank still makes every RNG draw
  const bool wide;
  // The group plan.  lq[j]: the lookup's region in the batch buffers (-1: another rank's);
  // used[j]: the value width its window assumes (0: full sort).
  // Lookups with identical table expressions (the same table, e.g. keccak's nibble-xor
  // columns for every lookup) share one sorted table: lookup j gathers it from lookup
  // tsrc[j]'s group.  Batch groups (gi0[j] input, gi1[j] table; G of them, gbits bits): the
  // inputs [0, nown), then one per distinct table (single-owner stages, and only while every
  // lookup sorts by its window -- a full sort writes its table group).  Otherwise two
  // groups per lookup.
  std::vector<int> lq, tsrc, gi0, gi1, used;
  int nown = 0, G = 0, gbits = 0;
  bool share = false;
  struct Set {  // scratch set q (0: the key's own) for the gathers and matches
    CanonKey *a2, *t2, *left;
    uint8_t* rep;
    uint32_t* rows;
    void* scr;
  };
  Set set(int q) const {
    if (q == 0) return Set{pk.ck_a2, pk.ck_t2, pk.ck_left, pk.rep_flag, pk.rep_rows, pk.lkb_scr.p};
    return Set{pk.lks_a2[q], pk.lks_t2[q], pk.lks_left[q], pk.lks_rep[q], pk.lks_rows[q], pk.lks_scr[q]};
  }
  CircuitWs& ws(int j) const { return *r.W[j / NL]; }
  LookupPermute(ProofRun& r, bool wide) : r(r), wide(wide) {}
  int plan();          // owners and groups; buffers sized, counters and flags cleared
  int compress();      // every owned lookup's compressed input and table (lk_a, lk_s)
  int key_and_sort();  // every column's window keys, the batched sort
  int match_all();     // gather, match and fill per lookup; counters and value masks to the host
  int match_fill(int j, bool again, const Set& z, hipStream_t sj);
  int full_sort(int j);
  int check_and_redo();  // lookups whose window failed: sorted in full and matched again
  int rows_upload(const std::vector<Fr>& rows);  // A'_l and S'_l's blinding rows, one upload
  bool matched() const;  // every owned lookup's inputs were found in its table
  const uint32_t* sidx = nullptr;  // the batched sort's row indices
};

}  // namespace prv
}  // namespace h2g
