// prover_selfcheck.cpp -- the prover's self-checks (h2g_pk_set_self_check): the verdict of
// ProofRun::self_check, the location of a fault on the run's own resident data, the argument
// checks of H2G_SELFCHECK_ARGUMENTS (selfcheck.hip) and h2g_last_self_check.
//
// The verdict.  Every commitment the proof carries was computed from the polynomial the
// prover then opens, so the multi-open argument holds whatever the witness; the one condition
// of verify_proof that depends on the witness is the vanishing identity at x,
//   h(x) (x^n - 1) = the circuits' expressions at x folded in y        (vanishing.h).
// The prover holds both sides once its evaluations are back on the host: the right side is
// vanishing_expected_h over the very scalars it wrote to the transcript -- the code the
// verifier runs -- and the left is the evaluation of h_poly = sum_i x^(n i) h_i(X) at x, which
// poly_eval_batch's Horner chain computed among the proof's openings (the value the verifier
// receives as the h commitment's opening).  Equal: the proof verifies.
#include "proof_run.h"
#include "selfcheck.h"
#include "vanishing.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace {
// the records of the last create_proof* of the process (h2g_last_self_check), under g_mu as
// g_last_challenges is
std::vector<h2g_check_failure> g_sc_recs;
uint64_t g_sc_total = 0;

bool rec_less(const h2g_check_failure& a, const h2g_check_failure& b) {
  if (a.reserved != b.reserved) return a.reserved < b.reserved;
  if (a.kind != b.kind) return a.kind < b.kind;
  if (a.index != b.index) return a.index < b.index;
  return a.row < b.row;
}
}  // namespace

namespace h2g {
namespace prv {
void self_check_reset() {
  g_sc_recs.clear();
  g_sc_total = 0;
}
}  // namespace prv
}  // namespace h2g

// circuit ci's record sink: its own counter and its own SC_REC_CAP slots, so that the host can
// stamp the circuit on what the kernels wrote
CheckSink ProofRun::sc_sink(int ci) const {
  CheckSink s;
  s.rec = pk.sc_rec.p + (size_t)ci * SC_REC_CAP;
  s.total = pk.sc_total.p + ci;
  s.cap = SC_REC_CAP;
  return s;
}

int ProofRun::self_check_begin() {
  if (!sc_mode) return H2G_OK;
  HIPCHK(pk.sc_rec.ensure((size_t)ncirc * SC_REC_CAP));
  HIPCHK(pk.sc_total.ensure(ncirc));
  HIPCHK(hipMemsetAsync(pk.sc_total.p, 0, (size_t)ncirc * sizeof(unsigned long long), st));
  return H2G_OK;
}

// S1 (prover.rs:418-421): the phase's advice as it came in.  As in the reference, the columns
// asked are the unblinded ones -- their rows [u, n) go into the commitment as handed in; a
// blinded column's are overwritten by the blinding rows, whatever they held
int ProofRun::sc_unusable_rows(int ci, const std::vector<int>& cols) {
  if (sc_mode < H2G_SELFCHECK_ARGUMENTS) return H2G_OK;
  UnusableCols uc;
  for (int c : cols) {
    if (!pk.unblinded[c]) continue;
    uc.col[uc.m] = W[ci]->adv[c];
    uc.index[uc.m++] = (uint32_t)c;
    if (uc.m == SC_MAXC) {
      HIPCHK(selfcheck_unusable_rows(uc, unusable, n, sc_sink(ci), st));
      uc.m = 0;
    }
  }
  HIPCHK(selfcheck_unusable_rows(uc, unusable, n, sc_sink(ci), st));
  return H2G_OK;
}

// S2 (lookup/prover.rs:475-488): every lookup's permuted pair, behind the match that made it
int ProofRun::sc_lookup_permuted() {
  if (sc_mode < H2G_SELFCHECK_ARGUMENTS) return H2G_OK;
  for (int ci = 0; ci < ncirc; ci++)
    for (int l = 0; l < pk.cs.NL; l++)
      HIPCHK(selfcheck_permuted(W[ci]->lk_ap[l], W[ci]->lk_sp[l], unusable, (uint32_t)l, sc_sink(ci), 0, st));
  return H2G_OK;
}

// S3 / S4: a product z against the arrays it was built from (index: the lookup's, or NL + the
// shuffle's).  A shuffle's closing value is the verdict's (kind 4)
int ProofRun::sc_product(int ci, uint32_t index, const Fr* z, const Fr* num_a, const Fr* num_b, const Fr* den_a,
                         const Fr* den_b) {
  if (sc_mode < H2G_SELFCHECK_ARGUMENTS) return H2G_OK;
  ProductCheckArgs a;
  a.z = z;
  a.num_a = num_a, a.num_b = num_b, a.den_a = den_a, a.den_b = den_b;
  a.ca = num_b ? beta : gamma;
  a.cb = gamma;
  a.u = unusable;
  a.closing = num_b != nullptr;
  a.index = index;
  a.sink = sc_sink(ci);
  HIPCHK(selfcheck_product(a, 0, st));
  return H2G_OK;
}

// S5: set i = ci * nsets + s of the proof, behind the kernel that assembled its z: the
// recurrence against sigma and delta^c omega^row, z[0] against the previous set's z[u] (one
// for set 0).  nx / q1 carry a set wider than a launch (the multi-open's scratch, free until then)
int ProofRun::sc_permutation(int i) {
  if (sc_mode < H2G_SELFCHECK_ARGUMENTS) return H2G_OK;
  const int ci = i / pk.cs.nsets, s = i % pk.cs.nsets;
  const int c0 = s * pk.cs.chunk_len, c1 = std::min(c0 + pk.cs.chunk_len, pk.cs.P);
  Fr deltaomega = pow_u64(fr_delta(), (uint64_t)c0);
  for (int c = c0; c < c1; c += PERM_MAXC) {
    PermCheckArgs a;
    a.z = W[ci]->z_lag[s];
    a.first = s ? W[ci]->z_lag[s - 1] + unusable : nullptr;
    a.c.m = std::min(PERM_MAXC, c1 - c);
    for (int j = 0; j < a.c.m; j++) {
      a.c.v[j] = col_vals(*W[ci], c + j);
      a.c.sigma[j] = pk.sigma_lag[c + j];
      a.c.beta_delta[j] = deltaomega * beta;
      deltaomega = deltaomega * fr_delta();
    }
    a.beta = beta, a.gamma = gamma;
    a.om = pk.om;
    a.u = unusable;
    a.acc_l = pk.nx, a.acc_r = pk.q1;
    a.begin = c == c0;
    a.end = c + PERM_MAXC >= c1;
    a.index = (uint32_t)s;
    a.sink = sc_sink(ci);
    HIPCHK(selfcheck_permutation(a, st));
  }
  return H2G_OK;
}

int ProofRun::self_check() {
  if (!sc_mode) return H2G_OK;
  const CsHost& cs = pk.cs;
  const EvalDomain dom{n, D.omega, D.omega_inv, D.bary};
  const int id_fix = ncirc * per_c, id_sig = id_fix + cs.F, id_h = id_sig + cs.P;
  const Fr x_next = rotate_omega(dom, x, 1), x_prev = rotate_omega(dom, x, -1);
  const Fr x_last = rotate_omega(dom, x, -(bf + 1));
  // ---- the verdict: expected_h from what went to the transcript against h(x)
  VanishingEvals E;
  E.chal = challenges;
  E.theta = theta, E.beta = beta, E.gamma = gamma, E.y = y, E.x = x;
  std::vector<std::vector<std::vector<Fr>>> inst(ncirc, std::vector<std::vector<Fr>>(cs.I));
  for (int ci = 0; ci < ncirc; ci++)
    for (int i = 0; i < cs.I; i++) {
      const uint64_t* col = in.instance[ci] + 4 * n * i;
      inst[ci][i].resize(in.inst_lens[ci][i]);
      for (size_t r = 0; r < inst[ci][i].size(); r++) inst[ci][i][r] = fr_from_limbs(col + 4 * r);
    }
  E.ins_ev = instance_evals(cs, dom, x, pow_u64(x, n), inst);
  E.adv_ev.resize(ncirc), E.sets.resize(ncirc), E.lk_ev.resize(ncirc), E.sh_ev.resize(ncirc);
  for (int ci = 0; ci < ncirc; ci++) {
    for (auto& q : cs.adv_q) E.adv_ev[ci].push_back(ev(id_adv(ci) + q.index, rotate_omega(dom, x, q.rot)));
    for (int s = 0; s < cs.nsets; s++)
      E.sets[ci].push_back({ev(id_z(ci) + s, x), ev(id_z(ci) + s, x_next),
                            s + 1 < cs.nsets ? ev(id_z(ci) + s, x_last) : Fr::zero()});
    for (int l = 0; l < cs.NL; l++) {
      const int zi = id_lk(ci) + 3 * l;
      E.lk_ev[ci].push_back({ev(zi, x), ev(zi, x_next), ev(zi + 1, x), ev(zi + 1, x_prev), ev(zi + 2, x)});
    }
    for (int s = 0; s < cs.NS; s++) E.sh_ev[ci].push_back({ev(id_sh(ci) + s, x), ev(id_sh(ci) + s, x_next)});
  }
  for (auto& q : cs.fix_q) E.fix_ev.push_back(ev(id_fix + q.index, rotate_omega(dom, x, q.rot)));
  for (int c = 0; c < cs.P; c++) E.perm_ev.push_back(ev(id_sig + c, x));
  const bool holds = vanishing_expected_h(cs, dom, E) == ev(id_h, x);
  // ---- the argument checks' counters (the stream is idle: the evaluations were waited for)
  std::vector<unsigned long long> tot(ncirc, 0);
  if (sc_mode >= H2G_SELFCHECK_ARGUMENTS) {
    HIPCHK(hipMemcpy(tot.data(), pk.sc_total.p, (size_t)ncirc * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    bool any = false;
    for (unsigned long long t : tot) any = any || t != 0;
    if (holds && !any) return H2G_OK;
  } else if (holds) {
    return H2G_OK;
  }
  clk.mark("self-check verdict");
  // ---- location, on the run's own data: the Lagrange advice with its real blinding rows, the
  // fixed and instance columns, the proof's challenges in pk.consts
  const int G = (int)pk.seg_gate.size();
  std::vector<Fr> z_last(ncirc, Fr::one()), sh_last((size_t)NSH, Fr::one());
  if (!holds) {
    for (int ci = 0; ci < ncirc; ci++) {
      GateCheckArgs ga;
      ga.prog = pk.prog;
      ga.segs = pk.d_seg_gate;
      ga.ngates = G;
      ga.n_slots = pk.n_slots;
      ga.consts = pk.consts;
      ga.load_col = W[ci]->d_load_col_lag;
      ga.load_rot = pk.d_load_rot;
      ga.n = n;
      ga.u = unusable;
      ga.sink = sc_sink(ci);
      HIPCHK(check_gates(ga, st));
      if (cs.nsets)
        HIPCHK(hipMemcpyAsync(&z_last[ci], W[ci]->z_lag[cs.nsets - 1] + unusable, sizeof(Fr), hipMemcpyDeviceToHost, st));
      for (int s = 0; s < cs.NS; s++)
        HIPCHK(hipMemcpyAsync(&sh_last[(size_t)ci * cs.NS + s], W[ci]->sh_z[s] + unusable, sizeof(Fr),
                              hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(tot.data(), pk.sc_total.p, (size_t)ncirc * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  std::vector<h2g_check_failure> recs;
  uint64_t total = 0;
  for (int ci = 0; ci < ncirc; ci++) {
    const size_t got = (size_t)std::min<unsigned long long>(tot[ci], SC_REC_CAP);
    const size_t at = recs.size();
    recs.resize(at + got);
    if (got)
      HIPCHK(hipMemcpy(recs.data() + at, pk.sc_rec.p + (size_t)ci * SC_REC_CAP, got * sizeof(h2g_check_failure),
                       hipMemcpyDeviceToHost));
    for (size_t i = at; i < recs.size(); i++) recs[i].reserved = (uint32_t)ci;
    total += tot[ci];
    if (!(z_last[ci] == Fr::one())) {
      recs.push_back({H2G_CHECK_PERMUTATION, (uint32_t)(cs.nsets - 1), (uint32_t)unusable, (uint32_t)ci});
      total++;
    }
    for (int s = 0; s < cs.NS; s++)
      if (!(sh_last[(size_t)ci * cs.NS + s] == Fr::one())) {
        recs.push_back({H2G_CHECK_SHUFFLE, (uint32_t)s, H2G_CHECK_NO_ROW, (uint32_t)ci});
        total++;
      }
  }
  if (!total) {  // the identity fails and nothing above says where
    recs.push_back({H2G_CHECK_IDENTITY, 0, H2G_CHECK_NO_ROW, 0});
    total = 1;
  }
  std::sort(recs.begin(), recs.end(), rec_less);
  // a recurrence or a permuted pair that does not hold is no witness's doing
  bool internal = false;
  for (const h2g_check_failure& r : recs)
    internal = internal || r.kind == H2G_CHECK_PERMUTED_PAIR ||
               ((r.kind == H2G_CHECK_PRODUCT || r.kind == H2G_CHECK_PERMUTATION) && r.row < unusable);
  g_sc_recs = std::move(recs);
  g_sc_total = total;
  clk.mark("self-check location");
  if (internal)
    return fail(H2G_ERR_STATE, "create_proof: self-check: libh2g built an argument that does not satisfy its own "
                               "recurrence (" + std::to_string(total) + " records in h2g_last_self_check); this is "
                               "a fault of the library or the device, not of the witness");
  return fail(H2G_ERR_UNSATISFIED,
              "create_proof: self-check: the witness does not satisfy the circuit, the proof would not verify (" +
                  std::to_string(total) + " records in h2g_last_self_check)");
}

extern "C" {

int h2g_pk_set_self_check(uint64_t pk, int mode) {  // host state only: needs no device
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (mode < H2G_SELFCHECK_OFF || mode > H2G_SELFCHECK_ARGUMENTS)
    return fail(H2G_ERR_ARG, "pk_set_self_check: mode must be 0 (off), 1 (verdict) or 2 (arguments)");
  ProvingKey* it = find_pk(pk);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  it->self_check = mode;
  return H2G_OK;
}

int h2g_last_self_check(h2g_check_failure* out, size_t cap, uint64_t* total) {
  NEED_DEV_P();
  if (!total) return fail(H2G_ERR_ARG, "last_self_check: null total");
  *total = g_sc_total;
  if (out)
    for (size_t i = 0; i < g_sc_recs.size() && i < cap; i++) out[i] = g_sc_recs[i];
  return H2G_OK;
}

// test seams (tests/test_selfcheck_kernels_gpu.py): the kernels on caller arrays of any n >= 2
namespace {
int seam_run(Device* d, size_t rec_cap, const std::function<hipError_t(const CheckSink&)>& launch,
             h2g_check_failure* out, size_t cap, uint64_t* total) {
  DevArr<uint4> rec;
  DevArr<unsigned long long> tot;
  HIPCHK(rec.ensure(std::max<size_t>(rec_cap, 1)));
  HIPCHK(tot.ensure(1));
  HIPCHK(hipMemsetAsync(tot.p, 0, sizeof(unsigned long long), d->stream));
  CheckSink s;
  s.rec = rec.p;
  s.total = tot.p;
  s.cap = rec_cap;
  HIPCHK(launch(s));
  unsigned long long t = 0;
  HIPCHK(hipMemcpyAsync(&t, tot.p, sizeof(t), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  std::vector<h2g_check_failure> recs((size_t)std::min<unsigned long long>(t, rec_cap));
  if (!recs.empty()) HIPCHK(hipMemcpy(recs.data(), rec.p, recs.size() * sizeof(h2g_check_failure), hipMemcpyDeviceToHost));
  std::sort(recs.begin(), recs.end(), rec_less);
  *total = t;
  for (size_t i = 0; i < recs.size(); i++) out[i] = recs[i];
  return H2G_OK;
}
}  // namespace

int h2g_debug_selfcheck_product_dev(const void* d_z, const void* d_num_a, const void* d_num_b, const void* d_den_a,
                                    const void* d_den_b, const uint64_t beta[4], const uint64_t gamma[4], uint64_t n,
                                    uint64_t u, int max_blocks, h2g_check_failure* out, size_t cap, uint64_t* total) {
  NEED_DEV_P();
  if (!d_z || !d_num_a || !d_den_a || !beta || !gamma || !total || (cap && !out))
    return fail(H2G_ERR_ARG, "debug_selfcheck_product: null argument");
  if ((d_num_b == nullptr) != (d_den_b == nullptr))
    return fail(H2G_ERR_ARG, "debug_selfcheck_product: num_b and den_b go together");
  if (n < 2 || u < 1 || u >= n || n > (1ull << 32) || max_blocks < 0)
    return fail(H2G_ERR_ARG, "debug_selfcheck_product: need 1 <= u < n <= 2^32, n >= 2, max_blocks >= 0");
  ProductCheckArgs a;
  a.z = static_cast<const Fr*>(d_z);
  a.num_a = static_cast<const Fr*>(d_num_a), a.num_b = static_cast<const Fr*>(d_num_b);
  a.den_a = static_cast<const Fr*>(d_den_a), a.den_b = static_cast<const Fr*>(d_den_b);
  a.ca = d_num_b ? fr_from_limbs(beta) : fr_from_limbs(gamma);
  a.cb = fr_from_limbs(gamma);
  a.u = u;
  return seam_run(d, std::min<size_t>(cap, u + 1), [&](const CheckSink& s) {
    a.sink = s;
    return selfcheck_product(a, max_blocks, d->stream);
  }, out, cap, total);
}

int h2g_debug_selfcheck_permuted_dev(const void* d_a, const void* d_s, uint64_t u, int max_blocks,
                                     h2g_check_failure* out, size_t cap, uint64_t* total) {
  NEED_DEV_P();
  if (!d_a || !d_s || !total || (cap && !out)) return fail(H2G_ERR_ARG, "debug_selfcheck_permuted: null argument");
  if (u < 1 || u > (1ull << 32) || max_blocks < 0)
    return fail(H2G_ERR_ARG, "debug_selfcheck_permuted: need 1 <= u <= 2^32, max_blocks >= 0");
  return seam_run(d, std::min<size_t>(cap, u), [&](const CheckSink& s) {
    return selfcheck_permuted(static_cast<const Fr*>(d_a), static_cast<const Fr*>(d_s), u, 0, s, max_blocks, d->stream);
  }, out, cap, total);
}

int h2g_debug_selfcheck_permutation_dev(const void* d_z, const uint64_t* first, const void* const* d_values,
                                        const void* const* d_sigmas, const uint64_t* delta_pows, int m,
                                        const uint64_t beta[4], const uint64_t gamma[4], const uint64_t omega[4],
                                        uint64_t u, h2g_check_failure* out, size_t cap, uint64_t* total) {
  NEED_DEV_P();
  if (!d_z || !d_values || !d_sigmas || !delta_pows || !beta || !gamma || !omega || !total || (cap && !out))
    return fail(H2G_ERR_ARG, "debug_selfcheck_permutation: null argument");
  if (m < 1 || m > 64 || u < 1 || u > (1ull << 24))
    return fail(H2G_ERR_ARG, "debug_selfcheck_permutation: need 1 <= m <= 64, 1 <= u <= 2^24");
  // omega^i as the prover's two-level table: lo[i] = omega^i (i < 64), hi[j] = omega^(64 j);
  // one more element holds `first`
  constexpr size_t kBits = 6, kLo = (size_t)1 << kBits;
  const Fr w = fr_from_limbs(omega), b = fr_from_limbs(beta);
  const size_t nhi = (size_t)(u >> kBits) + 1;
  std::vector<Fr> tab(kLo + nhi + 1);
  tab[0] = Fr::one();
  for (size_t i = 1; i < kLo; i++) tab[i] = tab[i - 1] * w;
  const Fr w64 = tab[kLo - 1] * w;
  tab[kLo] = Fr::one();
  for (size_t j = 1; j < nhi; j++) tab[kLo + j] = tab[kLo + j - 1] * w64;
  tab[kLo + nhi] = first ? fr_from_limbs(first) : Fr::one();
  DevArr<Fr> d_tab, acc;
  HIPCHK(d_tab.ensure(tab.size()));
  HIPCHK(acc.ensure(2 * u));
  HIPCHK(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * sizeof(Fr), hipMemcpyHostToDevice, d->stream));
  // (seam_run synchronises the stream before it returns: `tab` outlives its upload)
  return seam_run(d, std::min<size_t>(cap, u), [&](const CheckSink& s) {
    for (int c = 0; c < m; c += PERM_MAXC) {  // as ProofRun::sc_permutation splits a wide set
      PermCheckArgs a;
      a.z = static_cast<const Fr*>(d_z);
      a.first = first ? d_tab.p + kLo + nhi : nullptr;
      a.c.m = std::min(PERM_MAXC, m - c);
      for (int j = 0; j < a.c.m; j++) {
        a.c.v[j] = static_cast<const Fr*>(d_values[c + j]);
        a.c.sigma[j] = static_cast<const Fr*>(d_sigmas[c + j]);
        a.c.beta_delta[j] = fr_from_limbs(delta_pows + 4 * (c + j)) * b;
      }
      a.beta = b, a.gamma = fr_from_limbs(gamma);
      a.om.lo = d_tab.p, a.om.hi = d_tab.p + kLo, a.om.bits = (int)kBits;
      a.u = u;
      a.acc_l = acc.p, a.acc_r = acc.p + u;
      a.begin = c == 0;
      a.end = c + PERM_MAXC >= m;
      a.sink = s;
      const hipError_t e = selfcheck_permutation(a, d->stream);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }, out, cap, total);
}

}  // extern "C"
