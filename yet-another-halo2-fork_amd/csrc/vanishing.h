// vanishing.h -- the vanishing argument's identity at x, shared by the verifier (verifier.cpp,
// proof_terms) and the prover's self-check (prover_selfcheck.cpp): from a proof's evaluations,
// challenges and instances, the value h(x) must have,
//   expected_h = (sum of every circuit's gate, permutation, lookup and shuffle expressions at x,
//                 folded in y) / (x^n - 1)
// (halo2_backend/src/plonk/verifier.rs:258-393, vanishing/verifier.rs:84-113).  Host only.
#pragma once
#include "prover_state.h"

namespace h2g {
namespace prv {

// the evaluation domain's constants the identity needs (Domain / the verifier's Shape)
struct EvalDomain {
  size_t n;
  Fr omega, omega_inv, bary;  // bary = 1 / n
};

inline Fr rotate_omega(const EvalDomain& d, const Fr& x, int64_t rot) {
  return x * pow_u64(rot >= 0 ? d.omega : d.omega_inv, (uint64_t)(rot >= 0 ? rot : -rot));
}
// l_i_range (domain.rs:425-450): L_rot(x) for rot in [lo, hi)
inline std::vector<Fr> l_i_range(const EvalDomain& d, const Fr& x, const Fr& xn, int64_t lo, int64_t hi) {
  const Fr common = (xn - Fr::one()) * d.bary;
  std::vector<Fr> out;
  if (hi <= lo) return out;
  out.reserve((size_t)(hi - lo));
  Fr w = rotate_omega(d, Fr::one(), lo);
  for (int64_t rot = lo; rot < hi; rot++) {
    out.push_back(inv(x - w) * common * w);
    w = w * d.omega;
  }
  return out;
}

// One proof's values at x, in the transcript's order; per circuit where the first index is c
struct VanishingEvals {
  struct SetEv {
    Fr e0, e1, e2;  // z(x), z(omega x), z(omega^last x) (zero for the last set)
  };
  struct LkEv {
    Fr z, zn, ap, api, sp;
  };
  struct ShEv {
    Fr z, zn;
  };
  std::vector<std::vector<Fr>> adv_ev, ins_ev;  // [c][query]
  std::vector<Fr> fix_ev, perm_ev, chal;
  std::vector<std::vector<SetEv>> sets;
  std::vector<std::vector<LkEv>> lk_ev;
  std::vector<std::vector<ShEv>> sh_ev;
  Fr theta, beta, gamma, y, x;
};

// instance evaluations (QUERY_INSTANCE = false): inner products with l_i_range.  inst[c][i]:
// the values of circuit c's instance column i
inline std::vector<std::vector<Fr>> instance_evals(const CsHost& cs, const EvalDomain& d, const Fr& x, const Fr& xn,
                                                   const std::vector<std::vector<std::vector<Fr>>>& inst) {
  std::vector<std::vector<Fr>> ins_ev(inst.size(), std::vector<Fr>(cs.ins_q.size(), Fr::zero()));
  if (cs.ins_q.empty()) return ins_ev;
  int min_rot = 0, max_rot = 0;
  for (const auto& q : cs.ins_q) {
    min_rot = std::min(min_rot, q.rot);
    max_rot = std::max(max_rot, q.rot);
  }
  size_t max_len = 0;
  for (const auto& ci : inst)
    for (const auto& col : ci) max_len = std::max(max_len, col.size());
  const std::vector<Fr> l_is = l_i_range(d, x, xn, -(int64_t)max_rot, (int64_t)max_len + (int64_t)(-min_rot));
  for (size_t c = 0; c < inst.size(); c++)
    for (size_t qi = 0; qi < cs.ins_q.size(); qi++) {
      const auto& q = cs.ins_q[qi];
      const size_t off = (size_t)(max_rot - q.rot);
      const std::vector<Fr>& vals = inst[c][q.index];
      Fr acc = Fr::zero();
      for (size_t j = 0; j < vals.size() && off + j < l_is.size(); j++) acc = acc + vals[j] * l_is[off + j];
      ins_ev[c][qi] = acc;
    }
  return ins_ev;
}

// every circuit's expressions at x, one Horner chain in y, over x^n - 1
inline Fr vanishing_expected_h(const CsHost& cs, const EvalDomain& d, const VanishingEvals& e) {
  const int NC = (int)e.adv_ev.size(), nsets = cs.nsets, NL = cs.NL, NS = cs.NS;
  const Fr &x = e.x, &y = e.y, &theta = e.theta, &beta = e.beta, &gamma = e.gamma;
  const Fr xn = pow_u64(x, d.n);
  const Fr one = Fr::one();
  const std::vector<Fr> l_evals = l_i_range(d, x, xn, -(int64_t)(cs.bf + 1), 1);
  const Fr l_last = l_evals[0];
  Fr l_blind = Fr::zero();
  for (int i = 1; i < 1 + cs.bf; i++) l_blind = l_blind + l_evals[i];
  const Fr l_0 = l_evals[1 + cs.bf];
  const Fr active = one - (l_last + l_blind);
  auto qindex = [](const std::vector<Query>& qs, int type, int index, int rot) -> int {
    for (size_t i = 0; i < qs.size(); i++)
      if (qs[i].type == type && qs[i].index == index && qs[i].rot == rot) return (int)i;
    return -1;
  };
  Fr h_eval = Fr::zero();
  auto push = [&](const Fr& v) { h_eval = h_eval * y + v; };
  const size_t num_nodes = cs.nodes.size() / 4;
  std::vector<Fr> val(num_nodes);
  const Fr delta = fr_delta();
  for (int c = 0; c < NC; c++) {
    auto qeval = [&](int t, int i, int r) -> Fr {
      if (t == COL_ADVICE) {
        const int q = qindex(cs.adv_q, t, i, r);
        return q < 0 ? Fr::zero() : e.adv_ev[c][q];
      }
      if (t == COL_FIXED) {
        const int q = qindex(cs.fix_q, t, i, r);
        return q < 0 ? Fr::zero() : e.fix_ev[q];
      }
      const int q = qindex(cs.ins_q, t, i, r);
      return q < 0 ? Fr::zero() : e.ins_ev[c][q];
    };
    for (size_t i = 0; i < num_nodes; i++) {  // children precede parents (check_nodes)
      const int32_t* nd = &cs.nodes[4 * i];
      switch (nd[0]) {
        case OP_CONST: val[i] = cs.constants[nd[1]]; break;
        case OP_QUERY: val[i] = qeval(nd[1], nd[2], nd[3]); break;
        case OP_NEG: val[i] = Fr::zero() - val[nd[1]]; break;
        case OP_SUM: val[i] = val[nd[1]] + val[nd[2]]; break;
        case OP_PROD: val[i] = val[nd[1]] * val[nd[2]]; break;
        default: val[i] = e.chal[nd[1]]; break;  // OP_CHALLENGE
      }
    }
    for (int32_t g : cs.gate_roots) push(val[g]);
    if (nsets) {  // permutation/verifier.rs:120-210
      const std::vector<VanishingEvals::SetEv>& st = e.sets[c];
      push(l_0 * (one - st[0].e0));
      push((st[nsets - 1].e0 * st[nsets - 1].e0 - st[nsets - 1].e0) * l_last);
      for (int i = 1; i < nsets; i++) push((st[i].e0 - st[i - 1].e2) * l_0);
      for (int ci = 0; ci < nsets; ci++) {
        const int lo = ci * cs.chunk_len, hi = std::min(cs.P, lo + cs.chunk_len);
        Fr left = st[ci].e1;
        for (int j = lo; j < hi; j++)
          left = left * (qeval(cs.perm_cols[j].first, cs.perm_cols[j].second, 0) + beta * e.perm_ev[j] + gamma);
        Fr right = st[ci].e0;
        Fr cur = beta * x * pow_u64(delta, (uint64_t)lo);
        for (int j = lo; j < hi; j++) {
          right = right * (qeval(cs.perm_cols[j].first, cs.perm_cols[j].second, 0) + cur + gamma);
          cur = cur * delta;
        }
        push((left - right) * active);
      }
    }
    auto compress = [&](const std::vector<int32_t>& roots) {
      Fr acc = Fr::zero();
      for (int32_t r : roots) acc = acc * theta + val[r];
      return acc;
    };
    for (int l = 0; l < NL; l++) {  // lookup/verifier.rs:98-160
      const VanishingEvals::LkEv& v = e.lk_ev[c][l];
      push(l_0 * (one - v.z));
      push(l_last * (v.z * v.z - v.z));
      const Fr left = v.zn * (v.ap + beta) * (v.sp + gamma);
      const Fr right = v.z * (compress(cs.lk_in[l]) + beta) * (compress(cs.lk_tab[l]) + gamma);
      push((left - right) * active);
      push(l_0 * (v.ap - v.sp));
      push((v.ap - v.sp) * (v.ap - v.api) * active);
    }
    for (int l = 0; l < NS; l++) {  // shuffle/verifier.rs
      const VanishingEvals::ShEv& v = e.sh_ev[c][l];
      push(l_0 * (one - v.z));
      push(l_last * (v.z * v.z - v.z));
      push(active * (v.zn * (compress(cs.sh_sh[l]) + gamma) - v.z * (compress(cs.sh_in[l]) + gamma)));
    }
  }
  return h_eval * inv(xn - one);
}

}  // namespace prv
}  // namespace h2g
