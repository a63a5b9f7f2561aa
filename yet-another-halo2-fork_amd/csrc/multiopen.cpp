// multiopen.cpp -- the KZG multi-open argument (poly/kzg/multiopen), prover and verifier side,
// over an explicit context (multiopen.h):
//   ProverSHPLONK::create_proof      poly/kzg/multiopen/shplonk/prover.rs:121-305
//   construct_intermediate_sets      poly/kzg/multiopen/shplonk.rs:48-140
//   ProverGWC::create_proof          poly/kzg/multiopen/gwc/prover.rs:40-90, gwc.rs:25-50
//   VerifierSHPLONK::verify_proof    poly/kzg/multiopen/shplonk/verifier.rs:45-140
//   VerifierGWC::verify_proof        poly/kzg/multiopen/gwc/verifier.rs:42-123
// create_proof's tail (ProofRun, prover.cpp), verify_proof's tail (verifier.cpp) and the
// standalone h2g_multiopen_prove / _verify (kzg.cpp) all run these functions.
#include "multiopen.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace {
// the Lagrange basis of the points: out[j] = coefficients of prod_{k != j} (X - p_k) / (p_j - p_k)
std::vector<std::vector<Fr>> lagrange_basis(const std::vector<Fr>& pts) {
  const size_t m = pts.size();
  std::vector<std::vector<Fr>> out(m);
  for (size_t j = 0; j < m; j++) {
    std::vector<Fr> num(1, Fr::one());
    Fr den = Fr::one();
    for (size_t k = 0; k < m; k++) {
      if (k == j) continue;
      std::vector<Fr> nn(num.size() + 1, Fr::zero());
      for (size_t i = 0; i < num.size(); i++) {
        nn[i + 1] = nn[i + 1] + num[i];
        nn[i] = nn[i] - pts[k] * num[i];
      }
      num.swap(nn);
      den = den * (pts[j] - pts[k]);
    }
    const Fr sc = inv(den);
    for (Fr& c : num) c = c * sc;
    out[j] = std::move(num);
  }
  return out;
}
Fr eval_host(const std::vector<Fr>& p, const Fr& x) {
  Fr acc = Fr::zero();
  for (size_t i = p.size(); i-- > 0;) acc = acc * x + p[i];
  return acc;
}

// The kate divisions' carries: for a_i (global indexing, valid on [lo, hi1)) and point b_i,
// carry[i] = q_i[hi'] = sum_{j >= hi'} a_i[j + 1] b_i^(j - hi') (hi' = min(hi, n - 1)), from
// every slab's partial Horner value E_s = sum_{j in [lo_s, hi'_s)} a_i[j + 1] b_i^(j - lo_s):
// C_{W-1} = 0, C_r = E_{r+1} + b^(hi'_{r+1} - lo_{r+1}) C_{r+1}.  One all-gather for all points.
template <class Buf>
int slab_carries(MultiopenCtx& c, const std::vector<Fr>& pts, Buf a, std::vector<Fr>* carry) {
  ProvingKey& pk = *c.slab_pk;
  const Slab& sl = c.sl;
  const size_t n = c.n;
  hipStream_t st = c.st;
  const size_t np = pts.size();
  const size_t hq = std::min(sl.hi, n - 1);
  const uint64_t m = hq > sl.lo ? hq - sl.lo : 0;
  std::vector<EvalReq> reqs(np);
  for (size_t i = 0; i < np; i++) reqs[i] = EvalReq{a(i) + sl.lo + 1, m, pts[i]};
  HIPCHK(pk.d_reqs.ensure(np));
  HIPCHK(pk.evals.ensure(np));
  const size_t need = poly_eval_scratch_len((int)np, m ? m : 1);
  HIPCHK(pk.eval_scr.ensure(need));
  HIPCHK(c.upload(pk.d_reqs.p, reqs.data(), np * sizeof(EvalReq)));
  HIPCHK(poly_eval_batch(pk.d_reqs.p, (int)np, m ? m : 1, pk.evals.p, pk.eval_scr.p, st));
  std::vector<Fr> mine(np);
  HIPCHK(hipMemcpyAsync(mine.data(), pk.evals.p, np * sizeof(Fr), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<Fr> all;
  RCCHK(spmd_allgather_fr(mine, &all));
  carry->assign(np, Fr::zero());
  for (size_t i = 0; i < np; i++) {
    Fr cy = Fr::zero();
    for (int s = g_spmd.world - 1; s > g_spmd.rank; s--) {
      const Slab ss = spmd_slab(n, s);
      const size_t hs = std::min(ss.hi, n - 1);
      const uint64_t ms = hs > ss.lo ? hs - ss.lo : 0;
      cy = all[(size_t)s * np + i] + pow_u64(pts[i], ms) * cy;
    }
    (*carry)[i] = cy;
  }
  return H2G_OK;
}

int write_point(MultiopenCtx& c, const G1Affine& p) {
  if (!c.tr->write_point(p)) return fail(H2G_ERR_ARG, "cannot write points at infinity to the transcript");
  return H2G_OK;
}
void mark(MultiopenCtx& c, const char* name) {
  if (c.mark) c.mark(name);
}
}  // namespace

namespace h2g {
namespace prv {

int fr_cmp(const Fr& a, const Fr& b) {  // Ord on Fr: canonical numeric order
  const Fr ca = to_canonical(a), cb = to_canonical(b);
  for (int i = 7; i >= 0; i--) {
    if (ca.l[i] < cb.l[i]) return -1;
    if (ca.l[i] > cb.l[i]) return 1;
  }
  return 0;
}

// ---- ProverGWC::create_proof_with_engine (gwc/prover.rs:40-90): the queries grouped
// by point in first-appearance order (construct_intermediate_sets, gwc.rs:25-50); per
// point W(X) = (sum_i v^i p_i(X) - sum_i v^i p_i(z)) / (X - z), committed against g.
// The points' MSMs are independent, so all are launched before the first is collected.
int multiopen_gwc(MultiopenCtx& c) {
  Transcript& tr = *c.tr;
  const std::vector<PolyRef>& polys = *c.polys;
  const std::vector<OpenQ>& queries = *c.queries;
  const size_t n = c.n;
  hipStream_t st = c.st;
  const Fr v = tr.squeeze();
  std::vector<char> done(queries.size(), 0);
  std::vector<MsmTicket> tk;
  std::vector<Fr> neg_evb;
  neg_evb.reserve(queries.size());
  StreamSyncGuard evb_guard{st};  // neg_evb is read by asynchronous copies
  for (size_t i = 0; i < queries.size(); i++) {
    if (done[i]) continue;
    const Fr z = queries[i].pt;
    const size_t g = tk.size();
    if (g >= c.gwc_q->size()) {
      Fr* q;
      PALLOC(*c.pool, q, n);
      c.gwc_q->push_back(q);
    }
    LinTerms t;
    bool first = true;
    Fr vp = Fr::one(), evb = Fr::zero();
    for (size_t j = i; j < queries.size(); j++) {
      if (done[j] || queries[j].pt != z) continue;
      done[j] = 1;
      if (t.k == LIN_MAXT - 1) {
        HIPCHK(lincomb(c.nx, n, t, !first, st));
        first = false;
        t.k = 0;
      }
      t.p[t.k] = polys[queries[j].poly].p;
      t.len[t.k] = polys[queries[j].poly].len;
      t.coef[t.k] = vp;
      t.k++;
      evb = evb + vp * c.ev(queries[j].poly, z);
      vp = vp * v;
    }
    neg_evb.push_back(Fr::zero() - evb);  // poly_batch - eval_batch (poly.rs:268-276)
    HIPCHK(c.upload(c.small + g, &neg_evb.back(), sizeof(Fr)));
    t.p[t.k] = c.small + g;
    t.len[t.k] = 1;
    t.coef[t.k] = Fr::one();
    t.k++;
    HIPCHK(lincomb(c.nx, n, t, !first, st));
    HIPCHK(kate_division(c.nx, n, z, (*c.gwc_q)[g], c.scr, st));
    tk.emplace_back();
    RCCHK(commit_launch(c.d, *c.prm, (*c.gwc_q)[g], n - 1, SRS_G, st, &tk.back()));  // commit (kzg/commitment.rs:354-366)
  }
  {
    std::vector<MsmTicket*> tl;
    for (auto& t : tk) tl.push_back(&t);
    std::vector<G1Affine> cms(tl.size());
    RCCHK(commit_collect_all(c.d, tl.data(), (int)tl.size(), cms.data()));
    for (const G1Affine& cm : cms) RCCHK(write_point(c, cm));
  }
  HIPCHK(hipStreamSynchronize(st));  // neg_evb (host) is read by the copies above
  mark(c, "gwc");
  return H2G_OK;
}

// ---- SHPLONK (shplonk/prover.rs:121-305; construct_intermediate_sets shplonk.rs:48-140)
int multiopen_shplonk(MultiopenCtx& c) {
  Transcript& tr = *c.tr;
  const std::vector<PolyRef>& polys = *c.polys;
  const std::vector<OpenQ>& queries = *c.queries;
  const size_t n = c.n;
  hipStream_t st = c.st;
  const bool slabs = c.slabs;
  const Slab sl = slabs ? c.sl : Slab{0, n, n};
  // host values the device copies read asynchronously (live until the proof returns)
  std::vector<std::vector<Fr>> corr_stage;
  Fr c0_stage;
  StreamSyncGuard corr_guard{st};
  const Fr sy = tr.squeeze();
  std::vector<Fr> super_pts;
  for (auto& q : queries) {
    bool f = false;
    for (auto& p : super_pts) f = f || p == q.pt;
    if (!f) super_pts.push_back(q.pt);
  }
  std::sort(super_pts.begin(), super_pts.end(), [](const Fr& a, const Fr& b) { return fr_cmp(a, b) < 0; });
  std::vector<int> cm_ids;
  std::vector<std::vector<Fr>> cm_pts;
  for (auto& q : queries) {
    int f = -1;
    for (size_t i = 0; i < cm_ids.size(); i++)
      if (cm_ids[i] == q.poly) f = (int)i;
    if (f < 0) {
      f = (int)cm_ids.size();
      cm_ids.push_back(q.poly);
      cm_pts.emplace_back();
    }
    auto& ps = cm_pts[f];
    if (std::find(ps.begin(), ps.end(), q.pt) == ps.end()) ps.push_back(q.pt);
  }
  for (auto& ps : cm_pts) std::sort(ps.begin(), ps.end(), [](const Fr& a, const Fr& b) { return fr_cmp(a, b) < 0; });
  std::vector<int> rs_of(cm_ids.size()), rs_rep;
  for (size_t ci = 0; ci < cm_ids.size(); ci++) {
    int f = -1;
    for (size_t r = 0; r < rs_rep.size(); r++)
      if (cm_pts[rs_rep[r]] == cm_pts[ci]) f = (int)r;
    if (f < 0) {
      f = (int)rs_rep.size();
      rs_rep.push_back((int)ci);
    }
    rs_of[ci] = f;
  }
  // r_c: the interpolation through c's evaluations, from its rotation set's Lagrange basis
  // (one set of inversions per set, not per commitment)
  std::vector<std::vector<std::vector<Fr>>> basis(rs_rep.size());
  for (size_t r = 0; r < rs_rep.size(); r++) basis[r] = lagrange_basis(cm_pts[rs_rep[r]]);
  std::vector<std::vector<Fr>> low(cm_ids.size());
  for (size_t ci = 0; ci < cm_ids.size(); ci++) {
    const auto& B = basis[rs_of[ci]];
    const size_t m = cm_pts[ci].size();
    low[ci].assign(m, Fr::zero());
    for (size_t j = 0; j < m; j++) {
      const Fr e = c.ev(cm_ids[ci], cm_pts[ci][j]);
      for (size_t i = 0; i < m; i++) low[ci][i] = low[ci][i] + B[j][i] * e;
    }
  }
  const Fr v = tr.squeeze();
  // h_x = sum_s v^s (sum_i y^i (p_i - r_i)) / Z_s (the reference divides by Z_s with one
  // kate division per point of S_s, shplonk/prover.rs:142-176).  Partial fractions instead:
  // 1 / Z_s = sum_{p in S_s} c_{s,p} / (X - p) with c_{s,p} = prod_{p' in S_s \ p} (p - p')^-1,
  // and (g_s - r_s) / (X - p) is exact for every p in S_s, so with
  // G_p = sum_{s : p in S_s} v^s c_{s,p} (g_s - r_s), h_x = sum_p G_p / (X - p): one kate
  // division per distinct point (accumulated into h_x) instead of one per (set, point).
  // Exact field arithmetic, so h_x is the same polynomial.
  {
    std::vector<Fr> vpow(rs_rep.size()), ypow(cm_ids.size());
    {
      Fr vp = Fr::one();
      for (size_t r = 0; r < rs_rep.size(); r++) {
        vpow[r] = vp;
        vp = vp * v;
        Fr yp = Fr::one();
        for (size_t ci = 0; ci < cm_ids.size(); ci++)
          if (rs_of[ci] == (int)r) {
            ypow[ci] = yp;
            yp = yp * sy;
          }
      }
    }
    // slab mode: per point a (slab + halo) buffer; gbuf(i) indexes it globally
    const size_t np = super_pts.size(), cap = sl.hi1 - sl.lo + 1;
    if (slabs) HIPCHK(c.slab_pk->slab_buf.ensure(np * cap));
    auto gbuf = [&](size_t i) { return c.slab_pk->slab_buf.p + i * cap - sl.lo; };
    if (slabs) HIPCHK(hipMemsetAsync(c.hx + sl.lo, 0, (sl.hi1 - sl.lo) * sizeof(Fr), st));
    else HIPCHK(hipMemsetAsync(c.hx, 0, n * sizeof(Fr), st));
    for (size_t pi = 0; pi < np; pi++) {
      const Fr& p = super_pts[pi];
      Fr* gp = slabs ? gbuf(pi) : c.nx;
      // alpha_s = v^s c_{s,p} for the sets containing p
      std::vector<Fr> alpha(rs_rep.size(), Fr::zero());
      std::vector<char> has(rs_rep.size(), 0);
      size_t ncorr = 0;
      for (size_t r = 0; r < rs_rep.size(); r++) {
        const std::vector<Fr>& pts = cm_pts[rs_rep[r]];
        if (std::find(pts.begin(), pts.end(), p) == pts.end()) continue;
        Fr den = Fr::one();
        for (const Fr& q : pts)
          if (!(q == p)) den = den * (p - q);
        alpha[r] = vpow[r] * inv(den);
        has[r] = 1;
        ncorr = std::max(ncorr, pts.size());
      }
      corr_stage.emplace_back(ncorr, Fr::zero());  // read by an async copy
      std::vector<Fr>& corr = corr_stage.back();
      LinTerms t;
      bool first = true;
      for (size_t ci = 0; ci < cm_ids.size(); ci++) {
        const int r = rs_of[ci];
        if (!has[r]) continue;
        if (t.k == LIN_MAXT - 1) {
          RCCHK(lincomb_range(gp, sl.lo, sl.hi1, t, !first, st));
          first = false;
          t.k = 0;
        }
        const Fr coef = alpha[r] * ypow[ci];
        t.p[t.k] = polys[cm_ids[ci]].p;
        t.len[t.k] = polys[cm_ids[ci]].len;
        t.coef[t.k] = coef;
        t.k++;
        for (size_t j = 0; j < low[ci].size(); j++) corr[j] = corr[j] + coef * low[ci][j];
      }
      HIPCHK(c.upload(c.small, corr.data(), corr.size() * sizeof(Fr)));
      t.p[t.k] = c.small;
      t.len[t.k] = corr.size();
      t.coef[t.k] = fr_neg_one();
      t.k++;
      RCCHK(lincomb_range(gp, sl.lo, sl.hi1, t, !first, st));
      if (!slabs) HIPCHK(kate_division(c.nx, n, p, c.hx, c.scr, st, true));
    }
    if (slabs) {
      // G_p / (X - p) on slabs: q[i] = sum_{j >= i} a[j + 1] p^(j - i).  The slab's own part
      // plus p^(hi' - i) C, with C = q[hi'] the quotient just above the slab = sum over the
      // higher slabs of their partial Horner values E_s (one all-gather for every point);
      // C enters as p C added to a[hi'], so the division runs unchanged on the slab.
      std::vector<Fr> carry;
      RCCHK(slab_carries(c, super_pts, [&](size_t i) { return gbuf(i); }, &carry));
      Fr halo = Fr::zero();
      for (size_t pi = 0; pi < np; pi++) {
        const size_t hq = std::min(sl.hi, n - 1);
        if (hq <= sl.lo) continue;
        HIPCHK(poly_binop(POLY_ADD_CONST, gbuf(pi) + hq, nullptr, super_pts[pi] * carry[pi], gbuf(pi) + hq, 1, st));
        HIPCHK(kate_division(gbuf(pi) + sl.lo, hq - sl.lo + 1, super_pts[pi], c.hx + sl.lo, c.scr, st, true));
        halo = halo + carry[pi];
      }
      if (sl.hi < n) {  // h_x's halo coefficient (read by the linearisation): q[hi] = sum of the carries
        corr_stage.emplace_back(1, halo);
        HIPCHK(c.upload(c.hx + sl.hi, corr_stage.back().data(), sizeof(Fr)));
      }
    }
  }
  {
    G1Affine cm;
    RCCHK(commit(c.d, *c.prm, c.hx, n, SRS_G, &cm, st));
    RCCHK(write_point(c, cm));
  }
  mark(c, "shplonk h");
  const Fr u = tr.squeeze();
  // linearisation: l_x = sum_s v^s Z_{T\S_s}(u) sum_i y^i (p_i - r_i(u)) - Z_T(u) h_x
  Fr z0 = Fr::one();
  {
    Fr vpow = Fr::one(), c0 = Fr::zero();
    LinTerms t;
    bool first = true;
    auto flush = [&]() -> int {
      RCCHK(lincomb_range(c.lx, sl.lo, sl.hi1, t, !first, st));  // a slab rank: slab + halo
      first = false;
      t.k = 0;
      return H2G_OK;
    };
    for (size_t r = 0; r < rs_rep.size(); r++) {
      const std::vector<Fr>& pts = cm_pts[rs_rep[r]];
      Fr zi = Fr::one();
      for (auto& sp : super_pts)
        if (std::find(pts.begin(), pts.end(), sp) == pts.end()) zi = (u - sp) * zi;
      if (r == 0) z0 = zi;
      Fr ypow = Fr::one();
      for (size_t ci = 0; ci < cm_ids.size(); ci++) {
        if (rs_of[ci] != (int)r) continue;
        if (t.k == LIN_MAXT - 2) RCCHK(flush());
        const Fr coef = ypow * zi * vpow;
        t.p[t.k] = polys[cm_ids[ci]].p;
        t.len[t.k] = polys[cm_ids[ci]].len;
        t.coef[t.k] = coef;
        t.k++;
        c0 = c0 - coef * eval_host(low[ci], u);
        ypow = ypow * sy;
      }
      vpow = vpow * v;
    }
    Fr zt = Fr::one();
    for (auto& sp : super_pts) zt = (u - sp) * zt;
    c0_stage = c0;
    HIPCHK(c.upload(c.small, &c0_stage, sizeof(Fr)));
    t.p[t.k] = c.small;
    t.len[t.k] = 1;
    t.coef[t.k] = Fr::one();
    t.k++;
    t.p[t.k] = c.hx;
    t.len[t.k] = n;
    t.coef[t.k] = Fr::zero() - zt;
    t.k++;
    RCCHK(flush());
  }
  if (slabs) {  // the same slab division by (X - u), one carry
    std::vector<Fr> carry;
    const std::vector<Fr> pts{u};
    RCCHK(slab_carries(c, pts, [&](size_t) { return c.lx; }, &carry));
    const size_t hq = std::min(sl.hi, n - 1);
    if (hq > sl.lo) {
      HIPCHK(poly_binop(POLY_ADD_CONST, c.lx + hq, nullptr, u * carry[0], c.lx + hq, 1, st));
      HIPCHK(kate_division(c.lx + sl.lo, hq - sl.lo + 1, u, c.q1 + sl.lo, c.scr, st));
      HIPCHK(poly_binop(POLY_SCALE, c.q1 + sl.lo, nullptr, inv(z0), c.q1 + sl.lo, hq - sl.lo, st));
    }
  } else {
    HIPCHK(kate_division(c.lx, n, u, c.q1, c.scr, st));
    HIPCHK(poly_binop(POLY_SCALE, c.q1, nullptr, inv(z0), c.q1, n - 1, st));
  }
  {
    G1Affine cm;
    RCCHK(commit(c.d, *c.prm, c.q1, n - 1, SRS_G, &cm, st));
    RCCHK(write_point(c, cm));
  }
  mark(c, "shplonk final");
  return H2G_OK;
}

// ------------------------------------------------------------------ the verifiers' scalars
// equal bases merged (GWC lists a commitment once per opening point)
void msm_merge(Msm& m) {
  std::stable_sort(m.begin(), m.end(), [](const Term& a, const Term& b) { return a.base < b.base; });
  size_t w = 0;
  for (size_t i = 0; i < m.size(); i++) {
    if (w && m[w - 1].base == m[i].base) m[w - 1].s = m[w - 1].s + m[i].s;
    else m[w++] = m[i];
  }
  m.resize(w);
}

bool multiopen_verify_terms(int scheme, const std::vector<VerifierQ>& queries, MultiopenVerifyIo& io, Msm* left_out,
                            Msm* right_out) {
  Transcript& T = *io.T;
  const std::vector<Fr>& point = io.point;
  const Fr one = Fr::one();
  Msm& left = *left_out;
  Msm& right = *right_out;
  if (scheme == MULTIOPEN_GWC) {
    // VerifierGWC::verify_proof: queries grouped by point in first-appearance order
    const Fr v = T.squeeze();
    std::vector<int> group_pt;
    std::vector<std::vector<const VerifierQ*>> groups;
    for (const auto& q : queries) {
      size_t g = 0;
      while (g < group_pt.size() && group_pt[g] != q.pt) g++;
      if (g == group_pt.size()) {
        group_pt.push_back(q.pt);
        groups.emplace_back();
      }
      groups[g].push_back(&q);
    }
    if (io.expect_groups >= 0 && groups.size() != (size_t)io.expect_groups) return false;
    std::vector<uint32_t> ws(groups.size());
    for (auto& w : ws) w = io.read_point();
    const Fr u = T.squeeze();
    if (!io.ok()) return false;
    Fr eval_multi = Fr::zero(), upow = one;
    for (size_t g = 0; g < groups.size(); g++) {
      Fr evb = Fr::zero(), vpow = one;
      for (const VerifierQ* q : groups[g]) {
        io.add_obj(right, q->key, vpow * upow);
        evb = evb + vpow * q->eval;
        vpow = vpow * v;
      }
      eval_multi = eval_multi + upow * evb;
      right.push_back({ws[g], upow * point[group_pt[g]]});  // witness_with_aux
      left.push_back({ws[g], upow});                        // witness
      upow = upow * u;
    }
    right.push_back({BASE_G1, Fr::zero() - eval_multi});
    return true;
  }
  // construct_intermediate_sets: commitments in first-appearance order with their point
  // sets; commitments with equal point sets share a rotation set
  struct Cm {
    uint32_t key;
    std::vector<int> pts;   // sorted (by index: only the sets' identity matters)
    std::vector<Fr> evals;  // by pts
  };
  std::vector<Cm> cms;
  for (const auto& q : queries) {
    size_t i = 0;
    while (i < cms.size() && cms[i].key != q.key) i++;
    if (i == cms.size()) cms.push_back({q.key, {}, {}});
    Cm& cm = cms[i];
    size_t p = 0;
    while (p < cm.pts.size() && cm.pts[p] < q.pt) p++;
    if (p < cm.pts.size() && cm.pts[p] == q.pt) {
      // the same (commitment, point) twice: the later evaluation, as verify_proof has always
      // done here (the reference's get_eval finds the first, shplonk.rs:57-63; the two differ
      // only when a caller gives one pair two different evaluations)
      cm.evals[p] = q.eval;
    } else {
      cm.pts.insert(cm.pts.begin() + p, q.pt);
      cm.evals.insert(cm.evals.begin() + p, q.eval);
    }
  }
  std::vector<std::vector<int>> set_pts;
  std::vector<std::vector<const Cm*>> set_cms;
  for (const auto& cm : cms) {
    size_t s = 0;
    while (s < set_pts.size() && set_pts[s] != cm.pts) s++;
    if (s == set_pts.size()) {
      set_pts.push_back(cm.pts);
      set_cms.emplace_back();
    }
    set_cms[s].push_back(&cm);
  }
  std::vector<int> super;
  for (const auto& q : queries)
    if (std::find(super.begin(), super.end(), q.pt) == super.end()) super.push_back(q.pt);
  const Fr sy = T.squeeze();
  const Fr v = T.squeeze();
  const uint32_t h1 = io.read_point();
  const Fr u = T.squeeze();
  const uint32_t h2 = io.read_point();
  if (!io.ok()) return false;
  Fr z0 = Fr::zero(), z0_diff_inv = Fr::zero(), r_outer = Fr::zero(), vpow = one;
  for (size_t s = 0; s < set_pts.size(); s++) {
    const std::vector<int>& pts_s = set_pts[s];
    Fr z_diff = one;
    for (int p : super)
      if (std::find(pts_s.begin(), pts_s.end(), p) == pts_s.end()) z_diff = z_diff * (u - point[p]);
    if (s == 0) {
      z0 = one;
      for (int p : pts_s) z0 = z0 * (u - point[p]);
      z0_diff_inv = inv(z_diff);
      z_diff = one;
    } else {
      z_diff = z_diff * z0_diff_inv;
    }
    // the Lagrange basis of this set's points at u (the interpolated r(X) is only used at u)
    std::vector<Fr> basis(pts_s.size());
    for (size_t j = 0; j < pts_s.size(); j++) {
      Fr num = one, den = one;
      for (size_t k = 0; k < pts_s.size(); k++) {
        if (k == j) continue;
        num = num * (u - point[pts_s[k]]);
        den = den * (point[pts_s[j]] - point[pts_s[k]]);
      }
      basis[j] = num * inv(den);
    }
    Fr r_inner = Fr::zero(), ypow = one;
    const Fr scale = vpow * z_diff;
    for (const Cm* cm : set_cms[s]) {
      Fr ru = Fr::zero();
      for (size_t j = 0; j < pts_s.size(); j++) ru = ru + cm->evals[j] * basis[j];
      r_inner = r_inner + ypow * ru;
      io.add_obj(right, cm->key, ypow * scale);
      ypow = ypow * sy;
    }
    r_outer = r_outer + vpow * r_inner * z_diff;
    vpow = vpow * v;
  }
  right.push_back({BASE_G1, Fr::zero() - r_outer});
  right.push_back({h1, Fr::zero() - z0});
  right.push_back({h2, u});
  left.push_back({h2, one});
  return true;
}

}  // namespace prv
}  // namespace h2g
