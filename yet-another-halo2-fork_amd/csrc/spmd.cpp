// spmd.cpp -- multi-GPU plumbing of create_proof: the shard and SPMD transports, the ranks'
// consistency digest, slabs, sub-cosets, row pieces, column ownership and the exchanges.
#include "prover_state.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace h2g {
hipError_t link_delay(hipStream_t after, hipEvent_t done, double us);  // calib.hip
}


namespace {
bool g_comm_overlap = false;  // h2g_comm_set_exchange_overlap: column exchanges on the second communicator
// overlapped exchanges (h2g_set_spmd_exchange_async); NULL post: exchanges complete on return
h2g_spmd_exchange_post g_xpost = nullptr;
h2g_spmd_exchange_wait g_xwait = nullptr;
}  // namespace

namespace h2g {
namespace prv {
h2g_shard_transport g_shard{nullptr, 1, nullptr, nullptr};
uint64_t g_shard_seq = 0;
// SPMD sharding (h2g_set_spmd_transport): every rank proves, rank r computes slab r
h2g_spmd_transport g_spmd{nullptr, 1, 0, nullptr, nullptr};
uint64_t g_spmd_seq = 0;
SpmdStats g_spmd_stats;
SpmdCheck g_spmd_check;
bool g_spmd_colshard = true;
// SPMD slab weights (h2g_spmd_set_weights): prefix sums, world + 1 entries; empty = uniform
std::vector<uint64_t> g_spmd_wprefix;

}  // namespace prv
}  // namespace h2g

namespace {
int spmd_exchange(const void* d_send, const size_t* sb, void* d_recv, const size_t* rb) {
  uint64_t bytes = 0;
  for (int r = 0; r < g_spmd.world; r++) bytes += sb[r] + rb[r];
  return spmd_timed(2, bytes, [&] { return g_spmd.exchange(g_spmd.ctx, d_send, sb, d_recv, rb); });
}
void spmd_witness_settle() {
  SpmdCheck& c = g_spmd_check;
  if (!c.pend) return;
  (void)hipEventSynchronize(c.pend_ev);
  Blake2b h("h2g-spmd-witness");
  h.update(c.wit, 64);
  h.update(reinterpret_cast<const uint8_t*>(c.pend), (size_t)c.pend_n * sizeof(unsigned long long));
  h.digest(c.wit);
  c.pend = nullptr;
  c.pend_n = 0;
}
}  // namespace

namespace h2g {
namespace prv {
void spmd_digest(uint64_t out[4]) {
  uint8_t a[64] = {}, b[64] = {}, d[64];
  spmd_witness_settle();
  if (g_spmd_check.tr) g_spmd_check.tr->state_digest(a);
  if (g_spmd_check.rng) g_spmd_check.rng->draws_digest(b);
  Blake2b h("h2g-spmd-check\0\0");
  h.update(a, 64);
  h.update(b, 64);
  h.update(g_spmd_check.wit, 64);
  h.digest(d);
  std::memcpy(out, d, 32);
}

// ------------------------------------------------------------------ SPMD sub-cosets
// Row y = t + 2^e m of the extended coset (e = extended_k - k) is the point
// zeta w_ext^t w^m, so sub-coset t of a column is an n-point NTT of its coefficients
// twisted by w_ext^(t j), and evaluate_h on rows of one sub-coset reads only sub-coset t of
// every column: rotations move rows by multiples of 2^e (evaluation.rs:317-620 evaluates
// the same expressions row by row; the row split does not change any value).
bool spmd_subcosets() { return g_spmd.world > 1 && g_spmd.bcast != nullptr; }

Slab spmd_slab(size_t n, int r) {
  Slab s;
  s.lo = shard_lo(n, n, g_spmd.world, r);
  s.hi = shard_lo(n, n, g_spmd.world, r + 1);
  s.hi1 = std::min(s.hi + 1, n);
  return s;
}
// every rank's `mine` (same count on each), rank order
int spmd_allgather_fr(const std::vector<Fr>& mine, std::vector<Fr>* all) {
  const size_t W = (size_t)g_spmd.world, cnt = mine.size();
  all->assign(W * cnt, Fr::zero());
  if (!cnt) return H2G_OK;
  if (spmd_timed(1, cnt * sizeof(Fr) * (W + 1),
                 [&] { return g_spmd.allgather_host(g_spmd.ctx, mine.data(), cnt * sizeof(Fr), all->data()); }) != 0)
    return fail(H2G_ERR_STATE, "spmd transport: host all-gather failed");
  return H2G_OK;
}
// out[i] (+)= sum_k coef_k p_k[i] for i in [lo, hi) only (global indices; out, p_k full-length)
int lincomb_range(Fr* out, size_t lo, size_t hi, LinTerms t, bool accumulate, hipStream_t st) {
  if (hi <= lo) return H2G_OK;
  for (int k = 0; k < t.k; k++) {
    t.len[k] = t.len[k] > lo ? std::min<uint64_t>(t.len[k], hi) - lo : 0;
    t.p[k] = t.len[k] ? t.p[k] + lo : t.p[k];
  }
  HIPCHK(lincomb(out + lo, hi - lo, t, accumulate, st));
  return H2G_OK;
}
// the key's cosets cut to this rank's sub-cosets, once per (world, rank, pieces)
int sub_prepare(ProvingKey& pk, hipStream_t st, bool pieces) {
  const int64_t key = ((int64_t)g_spmd.world * 65536 + g_spmd.rank) * 2 + (pieces ? 1 : 0);
  if (pk.sub_key == key) return H2G_OK;
  const int e = (int)(pk.dom.ek - pk.dom.k);
  const uint64_t E = 1ull << e;
  const size_t n = pk.n;
  pk.sub_ts.clear();
  pk.sub_pieces = pieces;
  if (pieces) {  // world = G E: rank r takes piece r / E of sub-coset r mod E
    const uint64_t G = (uint64_t)g_spmd.world / E, p = (uint64_t)g_spmd.rank / E;
    pk.sub_ts.push_back((uint64_t)g_spmd.rank % E);
    pk.sub_lo = (uint64_t)n * p / G;
    pk.sub_hi = (uint64_t)n * (p + 1) / G;
  } else {
    for (uint64_t t = (uint64_t)g_spmd.rank; t < E; t += (uint64_t)g_spmd.world) pk.sub_ts.push_back(t);
    pk.sub_lo = 0;
    pk.sub_hi = n;
  }
  // the rows a piece reads around its own: every query rotation, z(omega X), z(omega^last X),
  // the lookups' A'(omega^-1 X)
  pk.rot_lo = std::min(-1, -(pk.cs.bf + 1));
  pk.rot_hi = 1;
  for (const Query& q : pk.loads) {
    pk.rot_lo = std::min(pk.rot_lo, q.rot);
    pk.rot_hi = std::max(pk.rot_hi, q.rot);
  }
  const size_t nt = pk.sub_ts.size();
  auto cut = [&](const Fr* full, Fr** out) -> int {
    if (!*out) HIPCHK(pk.pool.get((void**)out, pk.ext * sizeof(Fr)));  // room for any rank's slots
    for (size_t i = 0; i < nt; i++) HIPCHK(subcoset_gather(full, *out + i * n, n, pk.sub_ts[i], e, st));
    return H2G_OK;
  };
  pk.sub_fixed.resize(pk.cs.F, nullptr);
  pk.sub_sigma.resize(pk.cs.P, nullptr);
  for (int f = 0; f < pk.cs.F; f++) RCCHK(cut(pk.fixed_coset[f], &pk.sub_fixed[f]));
  for (int c = 0; c < pk.cs.P; c++) RCCHK(cut(pk.sigma_coset[c], &pk.sub_sigma[c]));
  RCCHK(cut(pk.l0, &pk.sub_l0));
  RCCHK(cut(pk.l_last, &pk.sub_ll));
  RCCHK(cut(pk.l_active, &pk.sub_la));
  pk.d_sigma_sub.assign(nt, nullptr);
  for (size_t i = 0; i < nt; i++) {
    std::vector<const Fr*> sg(pk.cs.P + 1, nullptr);
    for (int c = 0; c < pk.cs.P; c++) sg[c] = pk.sub_sigma[c] + i * n;
    PALLOC(pk.pool, pk.d_sigma_sub[i], sg.size());
    HIPCHK(hipMemcpy(pk.d_sigma_sub[i], sg.data(), sg.size() * sizeof(Fr*), hipMemcpyHostToDevice));
  }
  if (!pk.h_gather) PALLOC(pk.pool, pk.h_gather, pk.ext);
  HIPCHK(hipStreamSynchronize(st));
  pk.sub_key = key;
  return H2G_OK;
}

// a circuit workspace's evaluate_h tables for each owned sub-coset (cf. circuit_ws_add)
int sub_ws_tables(const ProvingKey& pk, CircuitWs& w) {
  if (w.sub_key == pk.sub_key) return H2G_OK;
  const size_t n = pk.n, nt = pk.sub_ts.size();
  w.sub.assign(nt, CircuitWs::SubTables{});
  for (size_t i = 0; i < nt; i++) {
    const size_t off = i * n;
    auto col = [&](const Query& q) -> const Fr* {
      if (q.type == COL_ADVICE) return w.adv_coset[q.index] + off;
      if (q.type == COL_FIXED) return pk.sub_fixed[q.index] + off;
      return w.inst_coset[q.index] + off;
    };
    std::vector<const Fr*> lc(pk.n_loads + 1, nullptr);
    for (int j = 0; j < pk.n_loads; j++) lc[j] = col(pk.loads[j]);
    std::vector<EvalLookup> el(pk.cs.NL + 1);
    std::vector<EvalShuffle> es(pk.cs.NS + 1);
    for (int l = 0; l < pk.cs.NL; l++)
      el[l] = EvalLookup{pk.seg_lk_in[l], pk.seg_lk_tab[l], w.lk_zc[l] + off, w.lk_apc[l] + off, w.lk_spc[l] + off};
    for (int l = 0; l < pk.cs.NS; l++) es[l] = EvalShuffle{pk.seg_sh_in[l], pk.seg_sh_sh[l], w.sh_zc[l] + off};
    std::vector<const Fr*> zt(pk.cs.nsets + 1, nullptr), pv(pk.cs.P + 1, nullptr);
    for (int q = 0; q < pk.cs.nsets; q++) zt[q] = w.z_coset[q] + off;
    for (int c = 0; c < pk.cs.P; c++) pv[c] = col(Query{pk.cs.perm_cols[c].first, pk.cs.perm_cols[c].second, 0});
    CircuitWs::SubTables& S = w.sub[i];
    PALLOC(w.pool, S.load_col, lc.size());
    PALLOC(w.pool, S.lookups, el.size());
    PALLOC(w.pool, S.shuffles, es.size());
    PALLOC(w.pool, S.z, zt.size());
    PALLOC(w.pool, S.perm_v, pv.size());
    HIPCHK(hipMemcpy(S.load_col, lc.data(), lc.size() * sizeof(Fr*), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.lookups, el.data(), el.size() * sizeof(EvalLookup), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.shuffles, es.data(), es.size() * sizeof(EvalShuffle), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.z, zt.data(), zt.size() * sizeof(Fr*), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.perm_v, pv.data(), pv.size() * sizeof(Fr*), hipMemcpyHostToDevice));
  }
  w.sub_key = pk.sub_key;
  return H2G_OK;
}

// the extended-coset columns evaluate_h reads (coeff_to_extended, domain.rs:230-244):
// whole cosets, or under the SPMD sub-coset split this rank's sub-cosets (slot i of dst =
// sub-coset sub_ts[i]; a rank past 2^e owns none and computes nothing)
int ext_cosets(Device* d, const ProvingKey& pk, const Fr* const* src, Fr* const* dst, int count, hipStream_t st) {
  if (pk.cosets) return H2G_OK;  // streamed: eval_h fills the slots from src, sub-coset by sub-coset
  if (!spmd_subcosets()) return coeff_to_extended_batch(d, pk.dom, src, dst, count, st);
  const size_t n = pk.n, nt = pk.sub_ts.size();
  std::vector<const Fr*> s2;
  std::vector<Fr*> d2;
  for (int c = 0; c < count; c++)
    for (size_t i = 0; i < nt; i++) {
      Fr* o = dst[c] + i * n;
      HIPCHK(subcoset_twist(src[c], o, n, pk.eo, pk.sub_ts[i], pk.ext - 1, st));
      s2.push_back(o);
      d2.push_back(o);
    }
  const Fr one = Fr::one();
  for (size_t b0 = 0; b0 < s2.size(); b0 += NTT_MAX_BATCH)
    RCCHK(ntt_dev_impl_batch(d, s2.data() + b0, n, d2.data() + b0, (int)std::min<size_t>(NTT_MAX_BATCH, s2.size() - b0),
                             n, (int)pk.dom.k, pk.dom.omega, 1, pk.dom.g_coset, pk.dom.g_coset_inv, 0, one, 0, one,
                             one, st));
  return H2G_OK;
}

// SPMD h(X) by coefficient slabs (h2g_spmd_transport.exchange): the owner of sub-coset t
// holds h's evaluations H(zeta w_ext^t w^m) in h_gather slot t.  An n-point inverse NTT
// (1/n, times zeta^-j) and the twist w_ext^(-t j) give the folded coefficients
// F_t[j] = sum_p h_{j+np} zeta^(np) rho^(t p) (rho = w_ext^n); slab r of every F_t goes
// to rank r, which inverts the E-point transform over t for its coefficients:
// h_{j+np} = zeta^(-np) E^-1 sum_t rho^(-t p) F_t[j] (extended_to_coeff, domain.rs:271-293,
// split into pieces of n, vanishing/prover.rs:122-128).  Exact, so the pieces equal the
// single-GPU ones.
int h_by_slabs(Device* d, ProvingKey& pk, const Slab& sl, hipStream_t st) {
  const Domain& D = pk.dom;
  const size_t n = pk.n, ext = pk.ext;
  const int W = g_spmd.world, me = g_spmd.rank;
  const int e = (int)(D.ek - D.k);
  const int E = 1 << e;
  const int np = pk.cs.degree - 1;
  if (E > HSLAB_MAX_E || np > E) return fail(H2G_ERR_ARG, "create_proof: too many sub-cosets for the h slab exchange");
  // the sub-cosets this rank interpolates (with row pieces: the leaders, ranks < E)
  std::vector<uint64_t> ts = pk.sub_ts;
  if (pk.sub_pieces && me >= E) ts.clear();
  const size_t nt = ts.size();
  // sizes: slab r of each owned sub-coset to rank r; every owner's blocks to me
  std::vector<size_t> sb(W), rb(W), soff(W + 1, 0);
  std::vector<Slab> slabs(W);
  for (int r = 0; r < W; r++) {
    slabs[r] = spmd_slab(n, r);
    sb[r] = nt * (slabs[r].hi1 - slabs[r].lo) * sizeof(Fr);
    soff[r + 1] = soff[r] + sb[r] / sizeof(Fr);
    int own = 0;
    for (int t = r; t < E; t += W) own++;
    rb[r] = (size_t)own * (sl.hi1 - sl.lo) * sizeof(Fr);
  }
  size_t rtot = 0;
  for (int r = 0; r < W; r++) rtot += rb[r] / sizeof(Fr);
  HIPCHK(pk.x_send.ensure(soff[W]));
  HIPCHK(pk.x_recv.ensure(rtot));
  const Fr one = Fr::one();
  for (size_t i = 0; i < nt; i++) {
    const uint64_t t = ts[i];
    Fr* f = pk.h_coeff + i * n;  // scratch until the combine
    RCCHK(ntt_dev_impl(d, pk.h_gather + t * n, n, f, n, (int)D.k, D.omega_inv, 0, one, one, 1, D.ifft_div, 1,
                       D.g_coset_inv, D.g_coset, st));
    HIPCHK(subcoset_twist(f, f, n, pk.eo, (ext - t) & (ext - 1), ext - 1, st));
    for (int r = 0; r < W; r++) {
      const size_t cnt = slabs[r].hi1 - slabs[r].lo;
      if (cnt)
        HIPCHK(hipMemcpyAsync(pk.x_send.p + soff[r] + i * cnt, f + slabs[r].lo, cnt * sizeof(Fr), hipMemcpyDeviceToDevice,
                              st));
    }
  }
  // combine coefficients coef[p E + t] = zeta^(-n p) rho^(-t p) / E
  std::vector<Fr> coef((size_t)np * E);
  {
    Fr ef = Fr::zero();
    for (int i = 0; i < E; i++) ef = ef + one;
    const Fr einv = inv(ef);
    const Fr rho_inv = inv(pow_u64(D.ext_omega, n));
    const Fr zinv_n = pow_u64(inv(zeta()), n);
    Fr zp = einv;
    for (int p = 0; p < np; p++) {
      Fr w = zp;
      const Fr step = pow_u64(rho_inv, (uint64_t)p);
      for (int t = 0; t < E; t++) {
        coef[(size_t)p * E + t] = w;
        w = w * step;
      }
      zp = zp * zinv_n;
    }
  }
  HIPCHK(pk_upload(pk, pk.small, coef.data(), coef.size() * sizeof(Fr), st));
  HIPCHK(hipStreamSynchronize(st));  // the send staging is complete; coef (host) was read
  if (spmd_exchange(pk.x_send.p, sb.data(), pk.x_recv.p, rb.data()) != 0)
    return fail(H2G_ERR_STATE, "spmd transport: exchange of h slabs failed");
  HSlabArgs a;
  a.recv = pk.x_recv.p;
  int pos = 0;
  for (int o = 0; o < W; o++)
    for (int t = o; t < E; t += W) a.idx[t] = pos++;
  a.E = E;
  a.np = np;
  a.cnt = sl.hi1 - sl.lo;
  a.n = n;
  a.lo = sl.lo;
  a.coef = pk.small;
  a.out = pk.h_coeff;
  HIPCHK(h_slab_combine(a, st));
  return H2G_OK;
}

// SPMD with more ranks than sub-cosets (E = 2^e): ranks 0 .. E-1 own the sub-cosets and
// hold every coefficient column whole; ranks E.. skipped those iNTTs and receive their slab
// [lo, hi1) of each column (column c from owner c mod E), one all-to-all per proof.
int coef_exchange(ProvingKey& pk, const std::vector<Fr*>& cols, hipStream_t st) {
  const size_t n = pk.n;
  const int W = g_spmd.world, me = g_spmd.rank;
  const int E = 1 << (pk.dom.ek - pk.dom.k);
  const int nc = (int)cols.size();
  std::vector<Slab> slabs(W);
  for (int r = 0; r < W; r++) slabs[r] = spmd_slab(n, r);
  auto ncols_of = [&](int o) {  // columns owner o sends
    int c = 0;
    for (int i = o; i < nc; i += E) c++;
    return c;
  };
  std::vector<size_t> sb(W, 0), rb(W, 0);
  size_t stot = 0, rtot = 0;
  for (int r = 0; r < W; r++) {
    if (me < E && r >= E) sb[r] = (size_t)ncols_of(me) * (slabs[r].hi1 - slabs[r].lo) * sizeof(Fr);
    if (me >= E && r < E) rb[r] = (size_t)ncols_of(r) * (slabs[me].hi1 - slabs[me].lo) * sizeof(Fr);
    stot += sb[r] / sizeof(Fr);
    rtot += rb[r] / sizeof(Fr);
  }
  HIPCHK(pk.x_send.ensure(stot));
  HIPCHK(pk.x_recv.ensure(rtot));
  if (me < E) {  // pack: per destination, my columns' slabs
    size_t off = 0;
    for (int r = E; r < W; r++) {
      const size_t cnt = slabs[r].hi1 - slabs[r].lo;
      for (int c = me; c < nc; c += E) {
        if (cnt) HIPCHK(hipMemcpyAsync(pk.x_send.p + off, cols[c] + slabs[r].lo, cnt * sizeof(Fr),
                                       hipMemcpyDeviceToDevice, st));
        off += cnt;
      }
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  if (spmd_exchange(pk.x_send.p, sb.data(), pk.x_recv.p, rb.data()) != 0)
    return fail(H2G_ERR_STATE, "spmd transport: exchange of coefficient slabs failed");
  if (me >= E) {  // unpack: owner by owner, its columns in order
    const size_t cnt = slabs[me].hi1 - slabs[me].lo;
    size_t off = 0;
    for (int o = 0; o < E; o++)
      for (int c = o; c < nc; c += E) {
        if (cnt) HIPCHK(hipMemcpyAsync(cols[c] + slabs[me].lo, pk.x_recv.p + off, cnt * sizeof(Fr),
                                       hipMemcpyDeviceToDevice, st));
        off += cnt;
      }
  }
  return H2G_OK;
}

// The rows of the extended domain rank r holds: (sub-coset t, its slot, first row a,
// count len; rows wrap mod n) -- whole sub-cosets t = r, r + world, ... when world <= 2^e,
// else its piece of sub-coset r mod 2^e with the halo of rotations around it
struct RowPiece {
  uint64_t t;
  int slot;
  uint64_t a, len;
};
std::vector<RowPiece> pieces_of(const ProvingKey& pk, int r) {
  const int W = g_spmd.world;
  const uint64_t E = 1ull << (pk.dom.ek - pk.dom.k), n = pk.n;
  std::vector<RowPiece> v;
  if (pk.sub_pieces) {
    const uint64_t G = (uint64_t)W / E, p = (uint64_t)r / E;
    const uint64_t lo = n * p / G, hi = n * (p + 1) / G;
    const uint64_t len = std::min<uint64_t>(n, hi - lo + (uint64_t)(pk.rot_hi - pk.rot_lo));
    const uint64_t a = (uint64_t)(((int64_t)lo + (int64_t)n + pk.rot_lo) % (int64_t)n);
    v.push_back({(uint64_t)r % E, 0, a, len});
  } else {
    int slot = 0;
    for (uint64_t t = (uint64_t)r; t < E; t += (uint64_t)W) v.push_back({t, slot++, 0, n});
  }
  return v;
}

// SPMD column ownership (SURVEY 8e's round-robin whole columns): column i of a stage is
// rank owner[i]'s, which alone forms its coefficients (the n-point iNTT, prover.rs:673-689 /
// lookup/prover.rs:131,311) and its E = 2^e sub-cosets (n-point NTTs of the twisted
// coefficients: the cosets of evaluation.rs:344-361) in its scratch.  One all-to-all then
// hands every rank the rows of every column it evaluates h on (pieces_of) and its
// coefficient slab [lo, hi1) (what the evaluations and SHPLONK read).  Message from o to r:
// per column of o in index order, r's pieces (in order, wrapped rows as two runs), then r's
// coefficient slab.  Used for wide stages (the owners also commit) and, with row pieces,
// for every stage (the transforms then never run twice).
int colshard_distribute(Device* d, ProvingKey& pk, const std::vector<const Fr*>& lag, const std::vector<Fr*>& poly,
                        const std::vector<Fr*>& coset, const std::vector<int>& owner, hipStream_t st) {
  const size_t n = pk.n;
  const int W = g_spmd.world, me = g_spmd.rank;
  const int E = 1 << (pk.dom.ek - pk.dom.k);
  const int M = (int)lag.size();
  std::vector<Slab> slabs(W);
  std::vector<std::vector<RowPiece>> pcs(W);
  for (int r = 0; r < W; r++) {
    slabs[r] = spmd_slab(n, r);
    pcs[r] = pieces_of(pk, r);
  }
  auto rows_of = [&](int r) {
    uint64_t w = 0;
    for (const RowPiece& pc : pcs[r]) w += pc.len;
    return w;
  };
  std::vector<int> mine;  // this rank's columns, index order
  for (int i = 0; i < M; i++)
    if (owner[i] == me) mine.push_back(i);
  std::vector<size_t> sb(W, 0), rb(W, 0), soff(W + 1, 0);
  for (int r = 0; r < W; r++) {
    if (r != me) {
      sb[r] = mine.size() * (rows_of(r) + (slabs[r].hi1 - slabs[r].lo)) * sizeof(Fr);
      size_t cols_r = 0;
      for (int i = 0; i < M; i++) cols_r += owner[i] == r;
      rb[r] = cols_r * (rows_of(me) + (slabs[me].hi1 - slabs[me].lo)) * sizeof(Fr);
    }
    soff[r + 1] = soff[r] + sb[r] / sizeof(Fr);
  }
  size_t rtot = 0;
  for (int r = 0; r < W; r++) rtot += rb[r] / sizeof(Fr);
  // overlapped: this exchange's own staging (the next stage packs while it is in flight);
  // otherwise the shared one
  ProvingKey::XPending* xp = nullptr;
  if (g_xpost) {
    if (pk.xp_used == pk.xp.size()) pk.xp.emplace_back();
    xp = &pk.xp[pk.xp_used];
    HIPCHK(xp->send.ensure(soff[W]));
    HIPCHK(xp->recv.ensure(rtot));
    HIPCHK(xp->done.ensure());
  } else {
    HIPCHK(pk.x_send.ensure(soff[W]));
    HIPCHK(pk.x_recv.ensure(rtot));
  }
  HIPCHK(pk.cs_scr.ensure(mine.size() * (size_t)E * n));
  // (every buffer the copy lists below point into is sized by now)
  Fr* const xs = xp ? xp->send.p : pk.x_send.p;
  Fr* const xr = xp ? xp->recv.p : pk.x_recv.p;
  // rows [a, a + len) mod n of one sub-coset: one or two runs
  auto runs = [&](const RowPiece& pc, auto&& fn) {
    const uint64_t first = std::min<uint64_t>(pc.len, n - pc.a);
    fn(pc.a, 0, first);
    if (pc.len > first) fn(0, first, pc.len - first);
  };
  // coefficients, then the twists and the n-point NTTs of every sub-coset of every column
  if (!mine.empty()) {
    std::vector<const Fr*> l2;
    std::vector<Fr*> p2, io;
    for (int i : mine) {
      l2.push_back(lag[i]);
      p2.push_back(poly[i]);
    }
    RCCHK(lagrange_to_coeff_batch(d, pk.dom, l2.data(), p2.data(), (int)l2.size(), st));
    for (size_t q = 0; q < mine.size(); q++)
      for (int t = 0; t < E; t++) {
        Fr* o = pk.cs_scr.p + (q * E + t) * n;
        HIPCHK(subcoset_twist(poly[mine[q]], o, n, pk.eo, (uint64_t)t, pk.ext - 1, st));
        io.push_back(o);
      }
    const Fr one = Fr::one();
    for (size_t b0 = 0; b0 < io.size(); b0 += NTT_MAX_BATCH)
      RCCHK(ntt_dev_impl_batch(d, (const Fr* const*)io.data() + b0, n, io.data() + b0,
                               (int)std::min<size_t>(NTT_MAX_BATCH, io.size() - b0), n, (int)pk.dom.k, pk.dom.omega, 1,
                               pk.dom.g_coset, pk.dom.g_coset_inv, 0, one, 0, one, one, st));
  }
  std::vector<CopySeg>& pack = pk.h_segs[0];
  std::vector<CopySeg>& unpack = pk.h_segs[1];
  pack.clear();
  unpack.clear();
  for (int r = 0; r < W; r++) {
    size_t pos = soff[r];
    for (size_t q = 0; q < mine.size(); q++) {
      const int i = mine[q];
      for (const RowPiece& pc : pcs[r]) {
        const Fr* src = pk.cs_scr.p + (q * E + pc.t) * n;
        runs(pc, [&](uint64_t row, uint64_t at, uint64_t cnt) {
          if (r == me) pack.push_back(CopySeg{src + row, coset[i] + (size_t)pc.slot * n + row, cnt});
          else pack.push_back(CopySeg{src + row, xs + pos + at, cnt});
        });
        if (r != me) pos += pc.len;
      }
      if (r == me) continue;
      const size_t cnt = slabs[r].hi1 - slabs[r].lo;
      if (cnt) pack.push_back(CopySeg{poly[i] + slabs[r].lo, xs + pos, cnt});
      pos += cnt;
    }
  }
  size_t off = 0;  // unpack, source by source
  const size_t mycnt = slabs[me].hi1 - slabs[me].lo;
  for (int o = 0; o < W; o++) {
    if (o == me) continue;
    for (int i = 0; i < M; i++) {
      if (owner[i] != o) continue;
      for (const RowPiece& pc : pcs[me]) {
        runs(pc, [&](uint64_t row, uint64_t at, uint64_t cnt) {
          unpack.push_back(CopySeg{xr + off + at, coset[i] + (size_t)pc.slot * n + row, cnt});
        });
        off += pc.len;
      }
      if (mycnt) unpack.push_back(CopySeg{xr + off, poly[i] + slabs[me].lo, mycnt});
      off += mycnt;
    }
  }
  RCCHK(copy_list_run(pk, pack, st));
  if (xp) {  // behind the pack on the stream; the receiver's rows land before h(X) (xp_flush)
    uint64_t bytes = 0;
    for (int r = 0; r < W; r++) bytes += sb[r] + rb[r];
    if (spmd_timed(2, bytes, [&] { return g_xpost(g_spmd.ctx, xs, sb.data(), xr, rb.data(), st, xp->done.h); }) != 0)
      return fail(H2G_ERR_STATE, "spmd transport: exchange of column sub-cosets failed (post)");
    xp->unpack.swap(unpack);
    xp->live = true;
    pk.xp_used++;
    return H2G_OK;
  }
  HIPCHK(hipStreamSynchronize(st));
  if (spmd_exchange(xs, sb.data(), xr, rb.data()) != 0)
    return fail(H2G_ERR_STATE, "spmd transport: exchange of column sub-cosets failed");
  RCCHK(copy_list_run(pk, unpack, st));
  return H2G_OK;
}

// the overlapped exchanges' received rows into their columns: every posted exchange waited
// for (the transport's deadline applies), the stream made to wait for its completion
// event, its unpack list queued -- before anything reads the cosets or the slabs
int xp_flush(ProvingKey& pk, hipStream_t st) {
  for (size_t k = 0; k < pk.xp_used; k++) {
    ProvingKey::XPending& x = pk.xp[k];
    if (!x.live) continue;
    x.live = false;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = g_xwait ? g_xwait(g_spmd.ctx, x.done) : (int)hipEventSynchronize(x.done);
    g_spmd_stats.ms[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != 0) {
      pk.xp_used = 0;
      return fail(H2G_ERR_STATE, "spmd transport: exchange of column sub-cosets failed (wait)");
    }
    HIPCHK(hipStreamWaitEvent(st, x.done, 0));
    RCCHK(copy_list_run(pk, x.unpack, st));
  }
  pk.xp_used = 0;
  return H2G_OK;
}

// a failed proof's exchanges still in flight: wait for them before their staging is reused
// or freed -- one bound for all of them together (10 s), and an exchange still pending past
// it is abandoned, not reused: its staging and event move to xp_lost (released with the
// key) so that the next proof posts into fresh buffers a late transfer cannot write
// 
void xp_drain(ProvingKey& pk) {
  const auto t0 = std::chrono::steady_clock::now();
  for (ProvingKey::XPending& x : pk.xp) {
    if (!x.live) continue;
    x.live = false;
    while (hipEventQuery(x.done) == hipErrorNotReady &&
           std::chrono::steady_clock::now() - t0 < std::chrono::seconds(10))
      std::this_thread::sleep_for(std::chrono::microseconds(200));
    if (hipEventQuery(x.done) == hipErrorNotReady) {
      pk.xp_lost.push_back(std::move(x));
      x = ProvingKey::XPending{};
    }
  }
  pk.xp_used = 0;
}

// pieces: the leader of sub-coset t (rank t) receives the h rows of the sub-coset's other
// pieces (ranks t + 2^e p), which arrive in rank order -- the rows' own order -- straight
// into its h_gather slot
int h_gather_pieces(ProvingKey& pk, hipStream_t st) {
  const int W = g_spmd.world, me = g_spmd.rank;
  const int E = 1 << (pk.dom.ek - pk.dom.k);
  const size_t n = pk.n;
  const uint64_t t = (uint64_t)me % (uint64_t)E;
  std::vector<size_t> sb(W, 0), rb(W, 0);
  const int G = W / E;
  if (me >= E) sb[t] = (pk.sub_hi - pk.sub_lo) * sizeof(Fr);
  else
    for (int p = 1; p < G; p++) rb[me + E * p] = (size_t)(n * (p + 1) / G - n * p / G) * sizeof(Fr);
  Fr* slot = pk.h_gather + t * n;
  HIPCHK(hipStreamSynchronize(st));
  if (spmd_exchange(slot + pk.sub_lo, sb.data(), slot + n / G, rb.data()) != 0)
    return fail(H2G_ERR_STATE, "spmd transport: exchange of h pieces failed");
  return H2G_OK;
}

// column i's rows go from every rank's MSM slab [shard_lo(P, n, W, r), shard_lo(.., r + 1))
// to its owner owner[i] (which then holds the whole column): one exchange; message from r
// to o: the slab rows of every column o owns, index order
int gather_to_owners(ProvingKey& pk, const std::vector<Fr*>& cols, const std::vector<int>& owner, size_t P,
                     hipStream_t st) {
  const size_t n = pk.n;
  const int W = g_spmd.world, me = g_spmd.rank;
  const int M = (int)cols.size();
  std::vector<size_t> lo(W + 1);
  for (int r = 0; r <= W; r++) lo[r] = shard_lo(P, n, W, r);
  std::vector<size_t> sb(W, 0), rb(W, 0), soff(W + 1, 0);
  for (int r = 0; r < W; r++) {
    if (r != me) {
      size_t mine = 0, theirs = 0;
      for (int i = 0; i < M; i++) {
        mine += owner[i] == r;     // r's columns: I send my slab of each
        theirs += owner[i] == me;  // my columns: r sends its slab of each
      }
      sb[r] = mine * (lo[me + 1] - lo[me]) * sizeof(Fr);
      rb[r] = theirs * (lo[r + 1] - lo[r]) * sizeof(Fr);
    }
    soff[r + 1] = soff[r] + sb[r] / sizeof(Fr);
  }
  size_t rtot = 0;
  for (int r = 0; r < W; r++) rtot += rb[r] / sizeof(Fr);
  HIPCHK(pk.x_send.ensure(soff[W]));
  HIPCHK(pk.x_recv.ensure(rtot));
  std::vector<CopySeg>& pack = pk.h_segs[0];
  std::vector<CopySeg>& unpack = pk.h_segs[1];
  pack.clear();
  unpack.clear();
  const size_t my = lo[me + 1] - lo[me];
  for (int r = 0; r < W; r++) {
    if (r == me || !my) continue;
    size_t pos = soff[r];
    for (int i = 0; i < M; i++)
      if (owner[i] == r) {
        pack.push_back(CopySeg{cols[i] + lo[me], pk.x_send.p + pos, my});
        pos += my;
      }
  }
  size_t off = 0;
  for (int r = 0; r < W; r++) {
    if (r == me) continue;
    const size_t cnt = lo[r + 1] - lo[r];
    for (int i = 0; i < M; i++)
      if (owner[i] == me && cnt) {
        unpack.push_back(CopySeg{pk.x_recv.p + off, cols[i] + lo[r], cnt});
        off += cnt;
      }
  }
  RCCHK(copy_list_run(pk, pack, st));
  HIPCHK(hipStreamSynchronize(st));
  if (spmd_exchange(pk.x_send.p, sb.data(), pk.x_recv.p, rb.data()) != 0)
    return fail(H2G_ERR_STATE, "spmd transport: exchange of product slabs failed");
  RCCHK(copy_list_run(pk, unpack, st));
  return H2G_OK;
}

// SPMD: an advice phase's m column checksums (pk.wsum_d.p, filled by the copy_columns that
// brought the columns in) to the host behind the stream; folded into the consistency
// digest by the next collective (spmd_witness_settle) -- only when sharded
int spmd_witness_prepare(ProvingKey& pk, int m, hipStream_t st) {
  if (g_spmd.world <= 1 || m <= 0) return H2G_OK;
  spmd_witness_settle();  // an earlier phase's, before its pinned buffer is reused
  HIPCHK(pk.wsum_d.ensure(m));
  HIPCHK(pk.wsum_h.ensure(m));
  HIPCHK(pk.wsum_ev.ensure());
  HIPCHK(hipMemsetAsync(pk.wsum_d.p, 0, (size_t)m * sizeof(unsigned long long), st));
  return H2G_OK;
}
int spmd_witness_fold(ProvingKey& pk, int m, hipStream_t st) {
  if (g_spmd.world <= 1 || m <= 0) return H2G_OK;
  HIPCHK(hipMemcpyAsync(pk.wsum_h.p, pk.wsum_d.p, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(pk.wsum_ev, st));
  g_spmd_check.pend = pk.wsum_h.p;
  g_spmd_check.pend_n = m;
  g_spmd_check.pend_ev = pk.wsum_ev;
  return H2G_OK;
}

}  // namespace prv
}  // namespace h2g

extern "C" {

int h2g_set_shard_transport(const h2g_shard_transport* t) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (t && t->world > 1) {
    if (!t->launch || !t->collect || t->world > 4096) return fail(H2G_ERR_ARG, "set_shard_transport: bad transport");
    g_shard = *t;
    g_spmd = h2g_spmd_transport{nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr};
  } else {
    g_shard = h2g_shard_transport{nullptr, 1, nullptr, nullptr};
  }
  g_shard_seq = 0;
  return H2G_OK;
}

int h2g_spmd_set_weights(const uint32_t* weights, int world) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  g_spmd_wprefix.clear();
  if (!weights || world <= 1) return H2G_OK;
  if (world > 4096) return fail(H2G_ERR_ARG, "spmd_set_weights: bad world");
  std::vector<uint64_t> pre(1, 0);
  for (int r = 0; r < world; r++) {
    if (weights[r] == 0) return fail(H2G_ERR_ARG, "spmd_set_weights: every rank needs a nonzero weight");
    pre.push_back(pre.back() + weights[r]);
  }
  g_spmd_wprefix = pre;
  return H2G_OK;
}

int h2g_spmd_stats(double* out, int max, int reset) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  for (int k = 0; k < 4; k++) {
    const double v[3] = {g_spmd_stats.ms[k], (double)g_spmd_stats.calls[k], (double)g_spmd_stats.bytes[k]};
    for (int j = 0; j < 3; j++)
      if (out && 3 * k + j < max) out[3 * k + j] = v[j];
  }
  if (reset) g_spmd_stats = SpmdStats{};
  return H2G_OK;
}

int h2g_spmd_set_column_owners(int on) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  g_spmd_colshard = on != 0;
  return H2G_OK;
}

int h2g_set_spmd_exchange_async(h2g_spmd_exchange_post post, h2g_spmd_exchange_wait wait) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (post && (!g_spmd.exchange || g_spmd.world < 2))
    return fail(H2G_ERR_STATE, "set_spmd_exchange_async: install an SPMD transport with an exchange first");
  g_xpost = post;
  g_xwait = post ? wait : nullptr;
  return H2G_OK;
}

int h2g_event_wait(void* done) {
  if (!done) return fail(H2G_ERR_ARG, "event_wait: null event");
  HIPCHK(hipEventSynchronize(static_cast<hipEvent_t>(done)));
  return H2G_OK;
}

int h2g_debug_link_delay(void* stream, void* done, double us) {
  if (!done) return fail(H2G_ERR_ARG, "debug_link_delay: null event");
  HIPCHK(link_delay(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(done), us));
  return H2G_OK;
}

int h2g_set_spmd_transport(const h2g_spmd_transport* t) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  g_xpost = nullptr;
  g_xwait = nullptr;
  if (t && t->world > 1) {
    if (!t->allgather || t->world > 4096 || t->rank < 0 || t->rank >= t->world)
      return fail(H2G_ERR_ARG, "set_spmd_transport: bad transport");
    g_spmd = *t;
    g_shard = h2g_shard_transport{nullptr, 1, nullptr, nullptr};
  } else {
    g_spmd = h2g_spmd_transport{nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr};
  }
  g_spmd_seq = 0;
  return H2G_OK;
}

/* ---- native multi-GPU exchange (csrc/comm.cpp) --------------------------------------- */
int h2g_comm_unique_id(uint8_t id[256]) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!id) return fail(H2G_ERR_ARG, "comm_unique_id: null id");
  return comm_unique_id(id);
}

int h2g_comm_init(const uint8_t id[256], int world, int rank) {
  NEED_DEV_P();
  if (!id) return fail(H2G_ERR_ARG, "comm_init: null id");
  return comm_init(id, world, rank);
}

int h2g_comm_set_timeout(double seconds) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  return comm_set_timeout(seconds);
}

int h2g_comm_info(int32_t* rccl_count, int32_t* rccl_rank) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  int c = 0, r = -1;
  RCCHK(comm_rccl_info(&c, &r));
  if (rccl_count) *rccl_count = c;
  if (rccl_rank) *rccl_rank = r;
  return H2G_OK;
}

int h2g_comm_destroy(void) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (g_shard.launch == comm_launch) g_shard = h2g_shard_transport{nullptr, 1, nullptr, nullptr};
  if (g_spmd.allgather == comm_allgather_partial) g_spmd = h2g_spmd_transport{nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr};
  if (g_xpost == comm_exchange_post) g_xpost = nullptr, g_xwait = nullptr;
  return comm_destroy();
}

int h2g_comm_set_exchange_overlap(int on) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  g_comm_overlap = on != 0;
  return H2G_OK;
}

int h2g_comm_set_serve_timeout(double seconds) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  return comm_set_serve_timeout(seconds);
}

int h2g_comm_keepalive(void) {
  NEED_DEV_P();
  return comm_keepalive();
}

int h2g_comm_spmd_install(int split_subcosets) {
  NEED_DEV_P();
  if (comm_world() < 2) return fail(H2G_ERR_STATE, "comm_spmd_install: needs a communicator (h2g_comm_init)");
  g_spmd = h2g_spmd_transport{comm_spmd_ctx(), comm_world(), comm_rank(), comm_allgather_partial,
                              split_subcosets ? comm_bcast : nullptr, comm_allgather_host,
                              split_subcosets ? comm_exchange : nullptr};
  // the column-ownership exchanges overlap the later stages on the second communicator
  // only when asked (h2g_comm_set_exchange_overlap): two communicators in flight from two
  // streams has not run on multi-GPU hardware yet, so blocking is the default
  g_xpost = split_subcosets && g_comm_overlap ? comm_exchange_post : nullptr;
  g_xwait = g_xpost ? comm_exchange_wait : nullptr;
  g_shard = h2g_shard_transport{nullptr, 1, nullptr, nullptr};
  g_spmd_seq = 0;
  return H2G_OK;
}

int h2g_comm_spmd_uninstall(void) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (g_spmd.allgather == comm_allgather_partial) g_spmd = h2g_spmd_transport{nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr};
  if (g_xpost == comm_exchange_post) g_xpost = nullptr, g_xwait = nullptr;
  g_spmd_seq = 0;
  return H2G_OK;
}

int h2g_comm_install(uint64_t params) {
  NEED_DEV_P();
  Params* ip = find_params(params);
  if (!ip) return fail(H2G_ERR_HANDLE, "unknown params");
  if (comm_world() < 2 || comm_rank() != 0) return fail(H2G_ERR_STATE, "comm_install: needs rank 0 of a communicator");
  g_shard = h2g_shard_transport{comm_transport_ctx(ip->n), comm_world(), comm_launch, comm_collect};
  g_shard_seq = 0;
  return H2G_OK;
}

int h2g_comm_stop(void) {
  NEED_DEV_P();
  if (g_shard.launch == comm_launch) g_shard = h2g_shard_transport{nullptr, 1, nullptr, nullptr};
  return comm_stop();
}

/* ranks 1..: answer rank 0's MSM slabs against `params` until it stops the session */
int h2g_comm_serve(uint64_t params, uint64_t* served) {
  NEED_DEV_P();
  Params* ip = find_params(params);
  if (!ip) return fail(H2G_ERR_HANDLE, "unknown params");
  Params& prm = *ip;
  if (prm.device != d->id) return fail(H2G_ERR_ARG, "comm_serve: params live on another device");
  static_assert(COMM_OP_STOP == commwait::REQ_STOP && COMM_OP_MSM == commwait::REQ_MSM &&
                    COMM_OP_PING == commwait::REQ_PING,
                "serve loop request codes");
  int32_t set = 0;
  uint64_t lo = 0, cnt = 0;
  const void* slab = nullptr;
  hipStream_t ready = nullptr;
  auto next = [&](int* op) -> int {  // the idle deadline applies (h2g_comm_set_serve_timeout)
    int32_t o = 0;
    RCCHK(comm_next_request(&o, &set, &lo, &cnt, &slab, &ready));
    *op = o;
    return H2G_OK;
  };
  auto answer = [&](int op) -> int {
    if (op != COMM_OP_MSM || set < SRS_G || set > SRS_LAGRANGE_PREFIX || lo > prm.n || cnt > prm.n - lo)
      return fail(H2G_ERR_STATE, "comm_serve: malformed request");
    // the slab's windows of the prefix basis (built on the first set-2 request inside the
    // slab), never the full-size table on a peer that only serves slabs
    if (set == SRS_LAGRANGE_PREFIX) RCCHK(params_prefix(prm, d->stream, lo, cnt));
    uint64_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (cnt) {
      size_t toff = 0;
      MsmTicket t;
      RCCHK(msm_fixed_launch(d, slab, prm.tables(set, lo, cnt, &toff), toff, cnt, ready, &t));
      RCCHK(msm_collect(d, &t, out));
    }
    uint64_t nz = 0;
    for (uint64_t v : out) nz |= v;
    RCCHK(comm_send_partial(out, nz == 0));
    return H2G_OK;
  };
  unsigned long long count = 0;
  RCCHK(commwait::serve_requests(next, answer, &count));
  if (served) *served = count;
  return H2G_OK;
}

}  // extern "C"
