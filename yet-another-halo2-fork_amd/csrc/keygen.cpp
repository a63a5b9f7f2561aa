// keygen.cpp -- circuit analysis, the gate compiler, keygen and the h2g_pk_* entry points.
#include "prover_state.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace {
// ------------------------------------------------------------------ circuit analysis
struct CircuitView {
  const h2g_circuit* c;
  const int32_t* node(int i) const { return c->nodes + 4 * i; }
};

int node_degree(const CircuitView& v, int i, std::vector<int>& memo) {
  if (memo[i] >= 0) return memo[i];
  const int32_t* nd = v.node(i);
  int d = 0;
  switch (nd[0]) {
    case OP_CONST:
    case OP_CHALLENGE: d = 0; break;
    case OP_QUERY: d = 1; break;
    case OP_NEG: d = node_degree(v, nd[1], memo); break;
    case OP_SUM: d = std::max(node_degree(v, nd[1], memo), node_degree(v, nd[2], memo)); break;
    default: d = node_degree(v, nd[1], memo) + node_degree(v, nd[2], memo); break;
  }
  return memo[i] = d;
}

// structurally equal expressions (the same operations on the same queries, constants and
// challenges by index)
bool same_expr(const CircuitView& v, int a, int b) {
  if (a == b) return true;
  const int32_t* x = v.node(a);
  const int32_t* y = v.node(b);
  if (x[0] != y[0]) return false;
  switch (x[0]) {
    case OP_CONST:
    case OP_CHALLENGE: return x[1] == y[1];
    case OP_QUERY: return x[1] == y[1] && x[2] == y[2] && x[3] == y[3];
    case OP_NEG: return same_expr(v, x[1], y[1]);
    default: return same_expr(v, x[1], y[1]) && same_expr(v, x[2], y[2]);
  }
}

void add_query(std::vector<Query>& l, const Query& q) {
  if (std::find(l.begin(), l.end(), q) == l.end()) l.push_back(q);
}

void collect(const CircuitView& v, int i, CsHost& cs) {  // keygen.rs:217-249, lhs before rhs
  const int32_t* nd = v.node(i);
  switch (nd[0]) {
    case OP_CONST:
    case OP_CHALLENGE: return;
    case OP_QUERY: {
      const Query q{nd[1], nd[2], nd[3]};
      add_query(nd[1] == COL_ADVICE ? cs.adv_q : (nd[1] == COL_FIXED ? cs.fix_q : cs.ins_q), q);
      return;
    }
    case OP_NEG: collect(v, nd[1], cs); return;
    default:
      collect(v, nd[1], cs);
      collect(v, nd[2], cs);
      return;
  }
}

// Gate expressions -> straight-line program over LDS value slots (tree code
// generation, larger subtree first to bound live slots; a - b fused as SUB).
struct GateCompiler {
  const CircuitView& v;
  std::vector<int4> prog;
  std::vector<Query> loads;
  std::vector<int> free_slots;
  int n_slots = 0;
  std::vector<int> need;
  explicit GateCompiler(const CircuitView& cv) : v(cv), need(cv.c->num_nodes, -1) {}
  int alloc() {
    if (!free_slots.empty()) {
      const int s = free_slots.back();
      free_slots.pop_back();
      return s;
    }
    return n_slots++;
  }
  void release(int s) { free_slots.push_back(s); }
  int regs(int i) {  // Sethi-Ullman register need
    if (need[i] >= 0) return need[i];
    const int32_t* nd = v.node(i);
    int r = 1;
    if (nd[0] == OP_NEG) r = regs(nd[1]);
    else if (nd[0] == OP_SUM || nd[0] == OP_PROD) {
      const int a = regs(nd[1]), b = regs(nd[2]);
      r = a == b ? a + 1 : std::max(a, b);
    }
    return need[i] = r;
  }
  int load_index(const Query& q) {
    for (size_t i = 0; i < loads.size(); i++)
      if (loads[i] == q) return (int)i;
    loads.push_back(q);
    return (int)loads.size() - 1;
  }
  // program segment: Horner (acc = acc * factor + e) over the expressions `roots`
  int2 compile_list(const int32_t* roots, int m) {
    const int off = (int)prog.size();
    for (int i = 0; i < m; i++) {
      const int s = gen(roots[i]);
      prog.push_back(make_int4(G_HORNER, 0, s, 0));
      release(s);
    }
    return make_int2(off, (int)prog.size() - off);
  }
  int gen(int i) {
    const int32_t* nd = v.node(i);
    switch (nd[0]) {
      case OP_CONST: {
        const int s = alloc();
        prog.push_back(make_int4(G_CONST, s, nd[1], 0));
        return s;
      }
      case OP_CHALLENGE: {  // challenge values follow the constants in pk.consts
        const int s = alloc();
        prog.push_back(make_int4(G_CONST, s, (int)v.c->num_constants + nd[1], 0));
        return s;
      }
      case OP_QUERY: {
        const int s = alloc();
        prog.push_back(make_int4(G_LOAD, s, load_index(Query{nd[1], nd[2], nd[3]}), 0));
        return s;
      }
      case OP_NEG: {
        const int a = gen(nd[1]);
        release(a);
        const int s = alloc();
        prog.push_back(make_int4(G_NEG, s, a, 0));
        return s;
      }
      default: {
        int lhs = nd[1], rhs = nd[2];
        int op = nd[0] == OP_SUM ? G_ADD : G_MUL;
        if (nd[0] == OP_SUM && v.node(rhs)[0] == OP_NEG) {  // a + (-b) -> a - b
          op = G_SUB;
          rhs = v.node(rhs)[1];
        }
        int a, b;
        if (regs(rhs) > regs(lhs)) {
          b = gen(rhs);
          a = gen(lhs);
        } else {
          a = gen(lhs);
          b = gen(rhs);
        }
        release(a);
        release(b);
        const int s = alloc();
        prog.push_back(make_int4(op, s, a, b));
        return s;
      }
    }
  }
};

bool check_nodes(const h2g_circuit* c, std::string* why) {
  const int64_t n = 1ll << c->k;
  for (uint32_t i = 0; i < c->num_nodes; i++) {
    const int32_t* nd = c->nodes + 4 * i;
    switch (nd[0]) {
      case OP_CONST:
        if (nd[1] < 0 || (uint32_t)nd[1] >= c->num_constants) return *why = "constant index", false;
        break;
      case OP_QUERY: {
        const uint32_t lim = nd[1] == COL_ADVICE ? c->num_advice : nd[1] == COL_FIXED ? c->num_fixed
                                                                   : nd[1] == COL_INSTANCE ? c->num_instance : 0;
        if (nd[2] < 0 || (uint32_t)nd[2] >= lim) return *why = "query column", false;
        if (nd[3] <= -n || nd[3] >= n) return *why = "rotation", false;
        break;
      }
      case OP_NEG:
        if (nd[1] < 0 || (uint32_t)nd[1] >= i) return *why = "node child must precede its parent", false;
        break;
      case OP_SUM:
      case OP_PROD:
        if (nd[1] < 0 || nd[2] < 0 || (uint32_t)nd[1] >= i || (uint32_t)nd[2] >= i)
          return *why = "node child must precede its parent", false;
        break;
      case OP_CHALLENGE:
        if (nd[1] < 0 || (uint32_t)nd[1] >= c->num_challenges) return *why = "challenge index", false;
        break;
      default: return *why = "node op", false;
    }
  }
  for (uint32_t g = 0; g < c->num_gates; g++)
    if (c->gate_roots[g] < 0 || (uint32_t)c->gate_roots[g] >= c->num_nodes) return *why = "gate root", false;
  auto check_args = [&](uint32_t na, const uint32_t* sizes, const int32_t* roots, const char* what) -> bool {
    if (na && (!sizes || !roots)) return *why = std::string("null ") + what, false;
    size_t off = 0;
    for (uint32_t l = 0; l < na; l++) {
      if (sizes[l] == 0) return *why = std::string(what) + " without expressions", false;
      for (uint32_t i = 0; i < 2 * sizes[l]; i++)
        if (roots[off + i] < 0 || (uint32_t)roots[off + i] >= c->num_nodes)
          return *why = std::string(what) + " root", false;
      off += 2 * sizes[l];
    }
    return true;
  };
  return check_args(c->num_lookups, c->lookup_sizes, c->lookup_roots, "lookup") &&
         check_args(c->num_shuffles, c->shuffle_sizes, c->shuffle_roots, "shuffle");
}

// per-argument root lists: (inputs, tables) of lookup l / (inputs, shuffles) of shuffle l
struct ArgRoots {
  const int32_t* in;
  const int32_t* other;
  int m;
};
std::vector<ArgRoots> arg_roots(uint32_t na, const uint32_t* sizes, const int32_t* roots) {
  std::vector<ArgRoots> out;
  size_t off = 0;
  for (uint32_t l = 0; l < na; l++) {
    const int m = (int)sizes[l];
    out.push_back({roots + off, roots + off + m, m});
    off += 2 * (size_t)m;
  }
  return out;
}

}  // namespace

namespace h2g {
namespace prv {
std::map<uint64_t, std::unique_ptr<ProvingKey>> g_pks;

// ------------------------------------------------------------------ keygen
// one more circuit workspace (create_proof over pk.cws.size() + 1 circuits)
int circuit_ws_add(ProvingKey& pk) {
  auto w = std::make_unique<CircuitWs>();
  const size_t n = pk.n;
  const size_t ext = pk.cosets ? pk.n : pk.ext;  // streamed: a coset array is one sub-coset slot
  auto vec_alloc = [&](std::vector<Fr*>& v, int cnt, size_t len) -> hipError_t {
    v.assign(cnt, nullptr);
    for (int i = 0; i < cnt; i++) {
      hipError_t e = w->pool.get((void**)&v[i], len * sizeof(Fr));
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  };
  HIPCHK(vec_alloc(w->adv, pk.cs.A, n));
  HIPCHK(vec_alloc(w->adv_poly, pk.cs.A, n));
  HIPCHK(vec_alloc(w->adv_coset, pk.cs.A, ext));
  HIPCHK(vec_alloc(w->inst_val, pk.cs.I, n));
  HIPCHK(vec_alloc(w->inst_poly, pk.cs.I, n));
  HIPCHK(vec_alloc(w->inst_coset, pk.cs.I, ext));
  HIPCHK(vec_alloc(w->z, pk.cs.nsets, n));
  HIPCHK(vec_alloc(w->z_lag, pk.cs.nsets, n));
  HIPCHK(vec_alloc(w->z_coset, pk.cs.nsets, ext));
  HIPCHK(vec_alloc(w->lk_a, pk.cs.NL, n));
  HIPCHK(vec_alloc(w->lk_s, pk.cs.NL, n));
  HIPCHK(vec_alloc(w->lk_ap, pk.cs.NL, n));
  HIPCHK(vec_alloc(w->lk_sp, pk.cs.NL, n));
  HIPCHK(vec_alloc(w->lk_ap_poly, pk.cs.NL, n));
  HIPCHK(vec_alloc(w->lk_sp_poly, pk.cs.NL, n));
  HIPCHK(vec_alloc(w->lk_z, pk.cs.NL, n));
  HIPCHK(vec_alloc(w->lk_z_poly, pk.cs.NL, n));
  HIPCHK(vec_alloc(w->lk_zc, pk.cs.NL, ext));
  HIPCHK(vec_alloc(w->lk_apc, pk.cs.NL, ext));
  HIPCHK(vec_alloc(w->lk_spc, pk.cs.NL, ext));
  HIPCHK(vec_alloc(w->sh_z, pk.cs.NS, n));
  HIPCHK(vec_alloc(w->sh_z_poly, pk.cs.NS, n));
  HIPCHK(vec_alloc(w->sh_zc, pk.cs.NS, ext));
  // pointer tables: the load table's columns for this circuit (fixed columns are shared)
  auto col = [&](const Query& q, bool coset) -> const Fr* {
    if (q.type == COL_ADVICE) return coset ? w->adv_coset[q.index] : w->adv[q.index];
    if (q.type == COL_FIXED) return coset ? pk.fixed_coset[q.index] : pk.fixed_lag[q.index];
    return coset ? w->inst_coset[q.index] : w->inst_val[q.index];
  };
  std::vector<const Fr*> lc(pk.n_loads + 1, nullptr), ll(pk.n_loads + 1, nullptr);
  for (int i = 0; i < pk.n_loads; i++) {
    lc[i] = col(pk.loads[i], true);
    ll[i] = col(pk.loads[i], false);
  }
  std::vector<EvalLookup> el(pk.cs.NL + 1);
  std::vector<EvalShuffle> es(pk.cs.NS + 1);
  for (int l = 0; l < pk.cs.NL; l++) el[l] = EvalLookup{pk.seg_lk_in[l], pk.seg_lk_tab[l], w->lk_zc[l], w->lk_apc[l], w->lk_spc[l]};
  for (int l = 0; l < pk.cs.NS; l++) es[l] = EvalShuffle{pk.seg_sh_in[l], pk.seg_sh_sh[l], w->sh_zc[l]};
  std::vector<const Fr*> zt(pk.cs.nsets + 1), pv(pk.cs.P + 1);
  for (int s = 0; s < pk.cs.nsets; s++) zt[s] = w->z_coset[s];
  for (int i = 0; i < pk.cs.P; i++) pv[i] = col(Query{pk.cs.perm_cols[i].first, pk.cs.perm_cols[i].second, 0}, true);
  PALLOC(w->pool, w->d_load_col, lc.size());
  PALLOC(w->pool, w->d_load_col_lag, ll.size());
  PALLOC(w->pool, w->d_lookups, el.size());
  PALLOC(w->pool, w->d_shuffles, es.size());
  PALLOC(w->pool, w->d_z, zt.size());
  PALLOC(w->pool, w->d_perm_v, pv.size());
  HIPCHK(hipMemcpy(w->d_load_col, lc.data(), lc.size() * sizeof(Fr*), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(w->d_load_col_lag, ll.data(), ll.size() * sizeof(Fr*), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(w->d_lookups, el.data(), el.size() * sizeof(EvalLookup), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(w->d_shuffles, es.data(), es.size() * sizeof(EvalShuffle), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(w->d_z, zt.data(), zt.size() * sizeof(Fr*), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(w->d_perm_v, pv.data(), pv.size() * sizeof(Fr*), hipMemcpyHostToDevice));
  pk.cws.push_back(std::move(w));
  return H2G_OK;
}

// the coset mode of a key-options struct (NULL: resident)
int key_options_mode(const h2g_key_options* opts, const char* who, int* mode) {
  *mode = H2G_COSETS_RESIDENT;
  if (!opts) return H2G_OK;
  if (opts->size < sizeof(h2g_key_options)) return fail(H2G_ERR_ARG, std::string(who) + ": key options: bad size");
  if (opts->cosets != H2G_COSETS_RESIDENT && opts->cosets != H2G_COSETS_STREAMED)
    return fail(H2G_ERR_ARG, std::string(who) + ": key options: unknown coset mode");
  *mode = (int)opts->cosets;
  return H2G_OK;
}

// two-level power table of w for exponents < 2^L
int build_pow_table(Pool& pool, const Fr& w, int L, PowTable* t, hipStream_t st) {
  const int bits = (L + 1) / 2;
  const size_t nlo = (size_t)1 << bits, nhi = (size_t)1 << (L - bits > 0 ? L - bits : 0);
  std::vector<Fr> lo(nlo), hi(nhi);
  lo[0] = Fr::one();
  for (size_t i = 1; i < nlo; i++) lo[i] = lo[i - 1] * w;
  const Fr wb = lo[nlo - 1] * w;  // w^(2^bits)
  hi[0] = Fr::one();
  for (size_t i = 1; i < nhi; i++) hi[i] = hi[i - 1] * wb;
  Fr *dlo, *dhi;
  PALLOC(pool, dlo, nlo);
  PALLOC(pool, dhi, nhi);
  HIPCHK(hipMemcpyAsync(dlo, lo.data(), nlo * sizeof(Fr), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dhi, hi.data(), nhi * sizeof(Fr), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  t->lo = dlo;
  t->hi = dhi;
  t->bits = bits;
  return H2G_OK;
}

// the constraint system's shape and a host copy of its expressions
int cs_host_build(const h2g_circuit* c, CsHost* out) {
  CsHost& cs = *out;
  cs = CsHost{};
  std::string why;
  if (c->num_gates && (!c->gate_roots || !c->nodes)) return fail(H2G_ERR_ARG, "keygen: null gates");
  if (!check_nodes(c, &why)) return fail(H2G_ERR_ARG, "keygen: bad expression graph: " + why);
  if (!c->transcript_repr) return fail(H2G_ERR_ARG, "keygen: null transcript_repr");
  if (c->k > FR_S) return fail(H2G_ERR_ARG, "keygen: k too large");
  const CircuitView cv{c};
  const size_t n = (size_t)1 << c->k;
  cs.k = c->k;
  cs.A = (int)c->num_advice;
  cs.F = (int)c->num_fixed;
  cs.I = (int)c->num_instance;
  cs.P = (int)c->num_perm_columns;
  cs.transcript_repr = fr_from_limbs(c->transcript_repr);
  cs.adv_phase.assign(cs.A, 0);
  if (c->advice_phase)
    for (int i = 0; i < cs.A; i++) cs.adv_phase[i] = c->advice_phase[i];
  cs.ch_phase.assign(c->num_challenges, 0);
  if (c->num_challenges && !c->challenge_phase) return fail(H2G_ERR_ARG, "keygen: null challenge_phase");
  for (uint32_t i = 0; i < c->num_challenges; i++) cs.ch_phase[i] = c->challenge_phase[i];
  cs.max_phase = 0;
  for (int i = 0; i < cs.A; i++) cs.max_phase = std::max(cs.max_phase, (int)cs.adv_phase[i]);
  for (uint8_t ph : cs.ch_phase)
    if ((int)ph > cs.max_phase) return fail(H2G_ERR_ARG, "keygen: challenge phase after the last advice phase");
  if (cs.P && !c->perm_columns) return fail(H2G_ERR_ARG, "keygen: null permutation columns");
  for (int i = 0; i < cs.P; i++) {
    const int t = c->perm_columns[2 * i], ix = c->perm_columns[2 * i + 1];
    const int lim = t == COL_ADVICE ? cs.A : t == COL_FIXED ? cs.F : t == COL_INSTANCE ? cs.I : 0;
    if (ix < 0 || ix >= lim) return fail(H2G_ERR_ARG, "keygen: permutation column out of range");
    cs.perm_cols.emplace_back(t, ix);
  }
  // degree, queries, blinding factors (circuit.rs:143-170,292-320; keygen.rs:191-260)
  std::vector<int> memo(c->num_nodes, -1);
  const std::vector<ArgRoots> lks = arg_roots(c->num_lookups, c->lookup_sizes, c->lookup_roots);
  const std::vector<ArgRoots> shs = arg_roots(c->num_shuffles, c->shuffle_sizes, c->shuffle_roots);
  cs.NL = (int)lks.size();
  cs.NS = (int)shs.size();
  cs.degree = 3;
  for (uint32_t g = 0; g < c->num_gates; g++) cs.degree = std::max(cs.degree, node_degree(cv, c->gate_roots[g], memo));
  for (const auto& a : lks) {  // lookup_argument_required_degree (circuit.rs:327-373)
    int di = 1, dt = 1;
    for (int i = 0; i < a.m; i++) {
      di = std::max(di, node_degree(cv, a.in[i], memo));
      dt = std::max(dt, node_degree(cv, a.other[i], memo));
    }
    cs.degree = std::max(cs.degree, std::max(4, 2 + di + dt));
  }
  for (const auto& a : shs) {  // shuffle_argument_required_degree (circuit.rs:375-389)
    int di = 1, ds = 1;
    for (int i = 0; i < a.m; i++) {
      di = std::max(di, node_degree(cv, a.in[i], memo));
      ds = std::max(ds, node_degree(cv, a.other[i], memo));
    }
    cs.degree = std::max(cs.degree, 2 + std::max(di, ds));
  }
  // queries: gates, lookups (inputs then tables), shuffles, permutation (keygen.rs:320-345)
  for (uint32_t g = 0; g < c->num_gates; g++) collect(cv, c->gate_roots[g], cs);
  for (const auto& a : lks) {
    for (int i = 0; i < a.m; i++) collect(cv, a.in[i], cs);
    for (int i = 0; i < a.m; i++) collect(cv, a.other[i], cs);
  }
  for (const auto& a : shs) {
    for (int i = 0; i < a.m; i++) collect(cv, a.in[i], cs);
    for (int i = 0; i < a.m; i++) collect(cv, a.other[i], cs);
  }
  for (auto& pc : cs.perm_cols)
    add_query(pc.first == COL_ADVICE ? cs.adv_q : (pc.first == COL_FIXED ? cs.fix_q : cs.ins_q),
              Query{pc.first, pc.second, 0});
  int maxq = 1;
  if (cs.A) {
    std::vector<int> cnt(cs.A, 0);
    for (auto& q : cs.adv_q) cnt[q.index]++;
    maxq = *std::max_element(cnt.begin(), cnt.end());
  }
  cs.bf = std::max(3, maxq) + 2;
  if ((int64_t)n < cs.bf + 3) return fail(H2G_ERR_ARG, "keygen: not enough rows available");
  cs.chunk_len = cs.degree - 2;
  cs.nsets = (cs.P + cs.chunk_len - 1) / cs.chunk_len;
  // the host copy of the expression graph
  if (c->num_nodes) cs.nodes.assign(c->nodes, c->nodes + 4 * (size_t)c->num_nodes);
  if (c->num_constants && !c->constants) return fail(H2G_ERR_ARG, "keygen: null constants");
  cs.constants.resize(c->num_constants);
  for (uint32_t i = 0; i < c->num_constants; i++) cs.constants[i] = fr_from_limbs(c->constants + 4 * i);
  if (c->num_gates) cs.gate_roots.assign(c->gate_roots, c->gate_roots + c->num_gates);
  for (const auto& a : lks) {
    cs.lk_in.emplace_back(a.in, a.in + a.m);
    cs.lk_tab.emplace_back(a.other, a.other + a.m);
  }
  for (const auto& a : shs) {
    cs.sh_in.emplace_back(a.in, a.in + a.m);
    cs.sh_sh.emplace_back(a.other, a.other + a.m);
  }
  return H2G_OK;
}

int keygen_impl(Device* d, Params& prm, const h2g_circuit* c, ProvingKey& pk, const PkImage* img = nullptr) {
  hipStream_t st = d->stream;
  if (c->k != prm.k) return fail(H2G_ERR_ARG, "keygen: circuit k != params k");
  RCCHK(cs_host_build(c, &pk.cs));
  if (!img && c->num_fixed && !c->fixed_values) return fail(H2G_ERR_ARG, "keygen: null fixed values");
  const CircuitView cv{c};
  const std::vector<ArgRoots> lks = arg_roots(c->num_lookups, c->lookup_sizes, c->lookup_roots);
  const std::vector<ArgRoots> shs = arg_roots(c->num_shuffles, c->shuffle_sizes, c->shuffle_roots);
  pk.device = d->id;
  pk.n = (size_t)1 << pk.cs.k;
  pk.unblinded.assign(pk.cs.A, 0);
  if (c->unblinded)
    for (int i = 0; i < pk.cs.A; i++) pk.unblinded[i] = c->unblinded[i];
  pk.num_consts = (int)c->num_constants;
  RCCHK(domain_init(&pk.dom, (uint32_t)pk.cs.degree, pk.cs.k));
  pk.ext = (size_t)1 << pk.dom.ek;
  pk.rot_scale = 1ull << (pk.dom.ek - pk.cs.k);
  const size_t n = pk.n, ext = pk.ext;
  Pool& pool = pk.pool;
  RCCHK(build_pow_table(pool, pk.dom.omega, (int)pk.cs.k, &pk.om, st));
  RCCHK(build_pow_table(pool, pk.dom.ext_omega, (int)pk.dom.ek, &pk.eo, st));

  // workspace first (keygen uses some of it as scratch)
  auto falloc = [&](Fr** p, size_t cnt) { return pool.get((void**)p, cnt * sizeof(Fr)); };
  pk.scr_len = std::max(n + 64, kate_scratch_len(n) + poly_prefix_scratch_len(n) + 64);
  HIPCHK(falloc(&pk.mod, n));
  HIPCHK(falloc(&pk.pre, n));
  HIPCHK(falloc(&pk.scr, pk.scr_len));
  HIPCHK(falloc(&pk.random_poly, n));
  HIPCHK(falloc(&pk.h_ext, ext));
  HIPCHK(falloc(&pk.h_coeff, ext));
  HIPCHK(falloc(&pk.h_poly, n));
  HIPCHK(falloc(&pk.nx, n));
  HIPCHK(falloc(&pk.q1, n));
  HIPCHK(falloc(&pk.hx, n));
  HIPCHK(falloc(&pk.lx, n));
  HIPCHK(falloc(&pk.small, 4096));
  HIPCHK(falloc(&pk.last_z, 1));
  auto vec_alloc = [&](std::vector<Fr*>& v, int cnt, size_t len) -> hipError_t {
    v.assign(cnt, nullptr);
    for (int i = 0; i < cnt; i++) {
      hipError_t e = falloc(&v[i], len);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  };
  HIPCHK(falloc(&pk.one, 1));
  {
    const Fr one = Fr::one();
    HIPCHK(hipMemcpy(pk.one, &one, sizeof(Fr), hipMemcpyHostToDevice));
  }
  if (pk.cs.NL + pk.cs.NS) {
    HIPCHK(falloc(&pk.tmp_a, n));
    HIPCHK(falloc(&pk.tmp_b, n));
  }
  if (pk.cs.NL) {  // permute_expression_pair scratch (the batched sort's buffers grow per proof)
    PALLOC(pool, pk.ck_a2, n);
    PALLOC(pool, pk.ck_t2, n);
    PALLOC(pool, pk.ck_left, n);
    PALLOC(pool, pk.rep_flag, n);
    PALLOC(pool, pk.left_flag, n);
    PALLOC(pool, pk.rep_rows, n);
    PALLOC(pool, pk.counters, 8);
    pk.lk_hb.assign(pk.cs.NL, 64);
  }

  // a streamed key holds one sub-coset slot where a resident key holds a coset; a coset
  // that comes with a key image is checked like the resident key's, in scratch, and dropped
  const bool streamed = pk.cosets != 0;
  const size_t clen = streamed ? n : ext;
  auto image_coset = [&](Fr* resident, const uint8_t* src) -> int {
    Fr* dst = streamed ? pk.h_ext : resident;
    HIPCHK(img->upload(dst, src, ext, st));
    if (streamed && img->bad_raw) HIPCHK(fr_count_unreduced(dst, ext, img->bad_raw, st));
    return H2G_OK;
  };
  if (streamed) HIPCHK(falloc(&pk.h_gather, ext));
  // fixed columns
  HIPCHK(vec_alloc(pk.fixed_lag, pk.cs.F, n));
  HIPCHK(vec_alloc(pk.fixed_poly, pk.cs.F, n));
  HIPCHK(vec_alloc(pk.fixed_coset, pk.cs.F, clen));
  for (int i = 0; i < pk.cs.F; i++) {
    if (img) {
      HIPCHK(img->upload(pk.fixed_lag[i], img->fixed_lag[i], n, st));
      HIPCHK(img->upload(pk.fixed_poly[i], img->fixed_poly[i], n, st));
      RCCHK(image_coset(pk.fixed_coset[i], img->fixed_coset[i]));
      continue;
    }
    HIPCHK(hipMemcpyAsync(pk.fixed_lag[i], c->fixed_values + 4 * n * i, n * sizeof(Fr), hipMemcpyHostToDevice, st));
    RCCHK(lagrange_to_coeff(d, pk.dom, pk.fixed_lag[i], pk.fixed_poly[i], st));
    if (!streamed) RCCHK(coeff_to_extended(d, pk.dom, pk.fixed_poly[i], pk.fixed_coset[i], st));
  }
  // l_0, l_last, l_active (keygen.rs:147-175)
  HIPCHK(falloc(&pk.l0, clen));
  HIPCHK(falloc(&pk.l_last, clen));
  HIPCHK(falloc(&pk.l_active, clen));
  if (img) {
    RCCHK(image_coset(pk.l0, img->l0));
    RCCHK(image_coset(pk.l_last, img->l_last));
    RCCHK(image_coset(pk.l_active, img->l_active));
  }
  if (!img || streamed) {
    const Fr one = Fr::one();
    std::vector<Fr> ones(pk.cs.bf, one);
    // the Lagrange polynomial(s) of `count` rows from row0: coefficient form, and (resident)
    // its extended coset
    auto lagrange_unit = [&](size_t row0, int count, Fr* poly, Fr* out) -> int {
      HIPCHK(hipMemsetAsync(pk.pre, 0, n * sizeof(Fr), st));
      HIPCHK(hipMemcpyAsync(pk.pre + row0, ones.data(), count * sizeof(Fr), hipMemcpyHostToDevice, st));
      RCCHK(lagrange_to_coeff(d, pk.dom, pk.pre, poly, st));
      if (out) RCCHK(coeff_to_extended(d, pk.dom, poly, out, st));
      HIPCHK(hipStreamSynchronize(st));
      return H2G_OK;
    };
    if (streamed) {
      HIPCHK(falloc(&pk.l0_poly, n));
      HIPCHK(falloc(&pk.l_last_poly, n));
      HIPCHK(falloc(&pk.l_blind_poly, n));
      RCCHK(lagrange_unit(0, 1, pk.l0_poly, nullptr));
      RCCHK(lagrange_unit(n - pk.cs.bf, pk.cs.bf, pk.l_blind_poly, nullptr));
      RCCHK(lagrange_unit(n - pk.cs.bf - 1, 1, pk.l_last_poly, nullptr));
    } else {
      RCCHK(lagrange_unit(0, 1, pk.mod, pk.l0));
      RCCHK(lagrange_unit(n - pk.cs.bf, pk.cs.bf, pk.mod, pk.h_ext));  // l_blind
      RCCHK(lagrange_unit(n - pk.cs.bf - 1, 1, pk.mod, pk.l_last));
      HIPCHK(poly_binop(POLY_ADD, pk.l_last, pk.h_ext, one, pk.l_active, ext, st));
      HIPCHK(poly_binop(POLY_SUB_CONST, pk.l_active, nullptr, one, pk.l_active, ext, st));
      HIPCHK(poly_binop(POLY_SCALE, pk.l_active, nullptr, fr_neg_one(), pk.l_active, ext, st));
    }
  }
  // permutation: Assembly on the host, sigma polynomials on the device
  HIPCHK(vec_alloc(pk.sigma_lag, pk.cs.P, n));
  HIPCHK(vec_alloc(pk.sigma_poly, pk.cs.P, n));
  HIPCHK(vec_alloc(pk.sigma_coset, pk.cs.P, clen));
  if (pk.cs.P && img) {
    for (int i = 0; i < pk.cs.P; i++) {
      HIPCHK(img->upload(pk.sigma_lag[i], img->sigma_lag[i], n, st));
      HIPCHK(img->upload(pk.sigma_poly[i], img->sigma_poly[i], n, st));
      RCCHK(image_coset(pk.sigma_coset[i], img->sigma_coset[i]));
    }
    HIPCHK(hipStreamSynchronize(st));
  } else if (pk.cs.P) {
    const size_t cells = (size_t)pk.cs.P * n;
    std::vector<uint32_t> mcol(cells), mrow(cells), acol(cells), arow(cells);
    std::vector<uint64_t> sizes(cells, 1);
    for (int cI = 0; cI < pk.cs.P; cI++)
      for (size_t r = 0; r < n; r++) {
        mcol[cI * n + r] = acol[cI * n + r] = (uint32_t)cI;
        mrow[cI * n + r] = arow[cI * n + r] = (uint32_t)r;
      }
    auto pos = [&](int t, int ix) -> int {
      for (int i = 0; i < pk.cs.P; i++)
        if (pk.cs.perm_cols[i].first == t && pk.cs.perm_cols[i].second == ix) return i;
      return -1;
    };
    for (uint32_t ci = 0; ci < c->num_copies; ci++) {  // Assembly::copy (permutation/keygen.rs:59-97)
      const int32_t* cp = c->copies + 6 * ci;
      const int lc = pos(cp[0], cp[1]), rc = pos(cp[3], cp[4]);
      if (lc < 0 || rc < 0) return fail(H2G_ERR_ARG, "keygen: copy on a column not in the permutation");
      if (cp[2] < 0 || cp[5] < 0 || (size_t)cp[2] >= n || (size_t)cp[5] >= n)
        return fail(H2G_ERR_ARG, "keygen: copy row out of bounds");
      const size_t li = lc * n + cp[2], ri = rc * n + cp[5];
      size_t lcyc = acol[li] * n + arow[li], rcyc = acol[ri] * n + arow[ri];
      if (lcyc == rcyc) continue;
      if (sizes[lcyc] < sizes[rcyc]) std::swap(lcyc, rcyc);
      sizes[lcyc] += sizes[rcyc];
      size_t i = rcyc;
      for (;;) {
        acol[i] = (uint32_t)(lcyc / n);
        arow[i] = (uint32_t)(lcyc % n);
        i = (size_t)mcol[i] * n + mrow[i];
        if (i == rcyc) break;
      }
      std::swap(mcol[li], mcol[ri]);
      std::swap(mrow[li], mrow[ri]);
    }
    std::vector<Fr> dpow(pk.cs.P + 1);
    dpow[0] = Fr::one();
    for (int i = 1; i <= pk.cs.P; i++) dpow[i] = dpow[i - 1] * fr_delta();
    uint32_t *dmc, *dmr;
    Fr* ddp;
    HIPCHK(hipMalloc(&dmc, cells * 4));
    HIPCHK(hipMalloc(&dmr, cells * 4));
    HIPCHK(hipMalloc(&ddp, dpow.size() * sizeof(Fr)));
    HIPCHK(hipMemcpyAsync(dmc, mcol.data(), cells * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dmr, mrow.data(), cells * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ddp, dpow.data(), dpow.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
    for (int i = 0; i < pk.cs.P; i++) {
      HIPCHK(sigma_from_mapping(pk.sigma_lag[i], dmc + i * n, dmr + i * n, n, ddp, pk.om, st));
      RCCHK(lagrange_to_coeff(d, pk.dom, pk.sigma_lag[i], pk.sigma_poly[i], st));
      if (!streamed) RCCHK(coeff_to_extended(d, pk.dom, pk.sigma_poly[i], pk.sigma_coset[i], st));
    }
    HIPCHK(hipStreamSynchronize(st));
    (void)hipFree(dmc);
    (void)hipFree(dmr);
    (void)hipFree(ddp);
  }
  // expression programs: gates (Horner in y), then each lookup's / shuffle's expression
  // lists (Horner in theta), sharing one slot allocation and one load table
  {
    GateCompiler gc(cv);
    pk.seg_gates = gc.compile_list(c->gate_roots, (int)c->num_gates);
    for (const auto& a : lks) {
      pk.seg_lk_in.push_back(gc.compile_list(a.in, a.m));
      pk.seg_lk_tab.push_back(gc.compile_list(a.other, a.m));
    }
    pk.lk_trep.assign(lks.size(), 0);
    for (size_t l = 0; l < lks.size(); l++) {
      pk.lk_trep[l] = (int)l;
      for (size_t r = 0; r < l; r++) {
        bool same = lks[r].m == lks[l].m;
        for (int i = 0; same && i < lks[l].m; i++) same = same_expr(cv, lks[r].other[i], lks[l].other[i]);
        if (same) {
          pk.lk_trep[l] = (int)r;
          break;
        }
      }
    }
    for (const auto& a : shs) {
      pk.seg_sh_in.push_back(gc.compile_list(a.in, a.m));
      pk.seg_sh_sh.push_back(gc.compile_list(a.other, a.m));
    }
    // the gates once more, one segment each (h2g_check_witness); the slots they need are
    // those of the folded list
    for (uint32_t g = 0; g < c->num_gates; g++) pk.seg_gate.push_back(gc.compile_list(c->gate_roots + g, 1));
    if (gc.n_slots > evaluate_h_max_slots())
      return fail(H2G_ERR_ARG, "keygen: expressions need more than " + std::to_string(evaluate_h_max_slots()) +
                                   " live values");
    pk.prog_len = (int)gc.prog.size();
    pk.n_slots = gc.n_slots;
    PALLOC(pool, pk.prog, gc.prog.size() + 1);
    HIPCHK(hipMemcpy(pk.prog, gc.prog.data(), gc.prog.size() * sizeof(int4), hipMemcpyHostToDevice));
    PALLOC(pool, pk.d_seg_gate, pk.seg_gate.size() + 1);
    if (!pk.seg_gate.empty())
      HIPCHK(hipMemcpy(pk.d_seg_gate, pk.seg_gate.data(), pk.seg_gate.size() * sizeof(int2), hipMemcpyHostToDevice));
    PALLOC(pool, pk.consts, c->num_constants + c->num_challenges + 1);
    if (c->num_constants)
      HIPCHK(hipMemcpy(pk.consts, c->constants, c->num_constants * sizeof(Fr), hipMemcpyHostToDevice));
    pk.n_loads = (int)gc.loads.size();
    pk.loads = gc.loads;
    std::vector<int> lr(pk.n_loads + 1, 0);
    for (int i = 0; i < pk.n_loads; i++) lr[i] = gc.loads[i].rot;
    PALLOC(pool, pk.d_load_rot, lr.size());
    HIPCHK(hipMemcpy(pk.d_load_rot, lr.data(), lr.size() * sizeof(int), hipMemcpyHostToDevice));
    std::vector<const Fr*> sg(pk.cs.P + 1);
    for (int i = 0; i < pk.cs.P; i++) sg[i] = pk.sigma_coset[i];
    PALLOC(pool, pk.d_sigma, sg.size());
    HIPCHK(hipMemcpy(pk.d_sigma, sg.data(), sg.size() * sizeof(Fr*), hipMemcpyHostToDevice));
  }
  RCCHK(circuit_ws_add(pk));  // circuit 0's workspace
  HIPCHK(hipStreamSynchronize(st));
  return H2G_OK;
}
}  // namespace prv
}  // namespace h2g

extern "C" {

int h2g_keygen(uint64_t params, const h2g_circuit* circuit, uint64_t* pk_out) {
  return h2g_keygen_opts(params, circuit, nullptr, pk_out);
}

int h2g_keygen_opts(uint64_t params, const h2g_circuit* circuit, const h2g_key_options* opts, uint64_t* pk_out) {
  NEED_DEV_P();
  Params* it = find_params(params);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown params");
  if (!circuit || !pk_out) return fail(H2G_ERR_ARG, "keygen: null argument");
  int cosets = H2G_COSETS_RESIDENT;
  RCCHK(key_options_mode(opts, "keygen", &cosets));
  auto pk = std::make_unique<ProvingKey>();
  pk->params = params;
  pk->cosets = cosets;
  int rc = keygen_impl(d, *it, circuit, *pk);
  // the lookup commitments' basis (params_prefix) now, not inside the first proof
  if (!rc && circuit->num_lookups > 0) rc = params_prefix(*it, d->stream);
  if (rc) return rc;
  *pk_out = g_next_handle++;
  g_pks[*pk_out] = std::move(pk);
  return H2G_OK;
}

int h2g_pk_free(uint64_t pk) {
  NEED_DEV_P();
  ProvingKey* it = find_pk(pk);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  (void)hipStreamSynchronize(d->stream);
  xp_drain(*it);
  g_pks.erase(pk);
  return H2G_OK;
}

/* VerifyingKey::fixed_commitments() (plonk.rs:228-231) and the permutation VerifyingKey's
 * commitments (plonk/permutation.rs:18-47): commit_lagrange of the fixed and sigma columns
 * (keygen.rs, permutation/keygen.rs:269), computed once */
int h2g_pk_vk_commitments(uint64_t pk_h, uint64_t* fixed, uint64_t* perm) {
  NEED_DEV_P();
  ProvingKey* it = find_pk(pk_h);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  ProvingKey& pk = *it;
  Params* pit = find_params(pk.params);
  if (!pit) return fail(H2G_ERR_HANDLE, "pk_vk_commitments: the key's params were freed");
  if (pk.vk_fixed.size() != (size_t)pk.cs.F || pk.vk_perm.size() != (size_t)pk.cs.P) {
    std::vector<G1Affine> f(pk.cs.F), q(pk.cs.P);
    for (int i = 0; i < pk.cs.F; i++) RCCHK(commit(d, *pit, pk.fixed_lag[i], pk.n, SRS_LAGRANGE, &f[i], d->stream));
    for (int i = 0; i < pk.cs.P; i++) RCCHK(commit(d, *pit, pk.sigma_lag[i], pk.n, SRS_LAGRANGE, &q[i], d->stream));
    pk.vk_fixed = f;
    pk.vk_perm = q;
  }
  if (fixed && pk.cs.F) std::memcpy(fixed, pk.vk_fixed.data(), pk.vk_fixed.size() * sizeof(G1Affine));
  if (perm && pk.cs.P) std::memcpy(perm, pk.vk_perm.data(), pk.vk_perm.size() * sizeof(G1Affine));
  return H2G_OK;
}

int h2g_pk_set_multiopen(uint64_t pk, int scheme) {
  NEED_DEV_P();
  ProvingKey* it = find_pk(pk);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  if (scheme != 0 && scheme != 1) return fail(H2G_ERR_ARG, "pk_set_multiopen: scheme must be 0 (SHPLONK) or 1 (GWC)");
  it->multiopen = scheme;
  return H2G_OK;
}

int h2g_pk_set_transcript(uint64_t pk, int kind) {
  NEED_DEV_P();
  ProvingKey* it = find_pk(pk);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  if (kind != TRANSCRIPT_BLAKE2B && kind != TRANSCRIPT_KECCAK256)
    return fail(H2G_ERR_ARG, "pk_set_transcript: kind must be 0 (Blake2bWrite) or 1 (Keccak256Write)");
  it->transcript = kind;
  return H2G_OK;
}

int h2g_pk_info(uint64_t pk, int32_t info[8]) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  ProvingKey* it = find_pk(pk);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  const ProvingKey& p = *it;
  const int32_t v[8] = {p.cs.degree, p.cs.bf, (int32_t)p.dom.ek, p.cs.nsets, (int32_t)p.cs.adv_q.size(),
                        (int32_t)p.cs.fix_q.size(), (int32_t)p.cs.ins_q.size(), p.n_slots};
  std::memcpy(info, v, sizeof(v));
  return H2G_OK;
}

/* out[0] the coset mode, out[1] the device bytes the key holds now (its arrays and the
 * per-proof workspaces grown so far), out[2] those of them in arrays of 2^extended_k
 * elements, out[3] 0.  The extended arrays are counted from the key's shape: h_ext, h_coeff
 * and (once allocated) h_gather in either mode -- the multi-open workspaces hold none --
 * and, resident only, one per coset column of the key and of every circuit workspace, plus
 * whatever the SPMD sub-coset split cut from them. */
int h2g_pk_memory(uint64_t pk_h, uint64_t out[4]) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  ProvingKey* it = find_pk(pk_h);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  if (!out) return fail(H2G_ERR_ARG, "pk_memory: null output");
  const ProvingKey& p = *it;
  uint64_t total = p.pool.bytes;
  for (const auto& w : p.cws) total += w->pool.bytes;
  total += p.lk_counters.len * sizeof(uint32_t) + p.lk_flags.len + p.lk_diff.len * sizeof(Fr) +
           p.lk_or_d.len * sizeof(unsigned long long) + p.wsum_d.len * sizeof(unsigned long long) +
           p.d_reqs.len * sizeof(EvalReq) + (p.evals.len + p.eval_scr.len + p.cs_scr.len + p.perm_lz.len) * sizeof(Fr) +
           p.lkb_canon.len * sizeof(CanonKey) + (p.lkb_key[0].len + p.lkb_key[1].len) * sizeof(uint64_t) +
           (p.lkb_idx[0].len + p.lkb_idx[1].len) * sizeof(uint32_t) + p.lkb_scr.len +
           (p.slab_buf.len + p.x_send.len + p.x_recv.len + p.blind_d.len) * sizeof(Fr) +
           p.d_segs.len * sizeof(CopySeg) + p.d_seeds.len * sizeof(uint32_t) + p.d_offsets.len * sizeof(uint64_t) +
           (p.asg_num.len + p.asg_den.len) * sizeof(Fr) + p.asg_idx.len * sizeof(uint64_t);
  uint64_t ext_arrays = 2 + (p.h_gather ? 1 : 0);  // h_ext, h_coeff, h_gather
  if (!p.cosets) {
    const uint64_t per_ws = (uint64_t)p.cs.A + p.cs.I + p.cs.nsets + 3 * (uint64_t)p.cs.NL + p.cs.NS;
    ext_arrays += (uint64_t)p.cs.F + p.cs.P + 3 + per_ws * p.cws.size();
    for (const Fr* s : p.sub_fixed) ext_arrays += s != nullptr;
    for (const Fr* s : p.sub_sigma) ext_arrays += s != nullptr;
    ext_arrays += (p.sub_l0 != nullptr) + (p.sub_ll != nullptr) + (p.sub_la != nullptr);
  }
  out[0] = (uint64_t)p.cosets;
  out[1] = total;
  out[2] = ext_arrays * p.ext * sizeof(Fr);
  out[3] = 0;
  return H2G_OK;
}

int h2g_pk_lookup_sort_hints(uint64_t pk, int32_t* out, int max, int* count) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  ProvingKey* it = find_pk(pk);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  if (!count || max < 0 || (max > 0 && !out)) return fail(H2G_ERR_ARG, "pk_lookup_sort_hints: bad arguments");
  const std::vector<int>& hb = it->lk_hb;
  *count = (int)hb.size();
  for (int i = 0; i < max && i < (int)hb.size(); i++) out[i] = (int32_t)hb[i];
  return H2G_OK;
}

}  // extern "C"
