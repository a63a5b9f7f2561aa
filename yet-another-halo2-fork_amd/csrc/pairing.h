// pairing.h -- host-side BN254 optimal ate pairing (verifier only; plain C++17, no device code).
//
// DualMSM::check (halo2_backend/src/poly/kzg/msm.rs:188-206) decides
// e(left, s_g2) == e(right, g2); a batch verifier needs exactly one such check for a valid
// batch, so this is a straightforward affine Miller loop, written to be compared with
// oracle/py/pairing_ref.py value for value:
//   Fq2  = Fq[u] / (u^2 + 1)                        (g2.h)
//   Fq6  = Fq2[v] / (v^3 - xi), xi = 9 + u
//   Fq12 = Fq6[w] / (w^2 - v) = Fq2[w] / (w^6 - xi), stored as the 6 Fq2 coefficients of
//          1, w, .., w^5 (pairing_ref's layout); the Fq6 halves are the even and the odd ones
// G2 is the D-type twist y^2 = x^3 + 3 / xi, mapped into E(Fq12) as (x w^2, y w^3).
// Miller loop over 6u + 2 with affine line functions l = -yp + (lam xp) w + (yt - lam xt) w^3,
// the two Frobenius-twisted closing lines, shared squarings over several pairs, then the final
// exponentiation (p^12 - 1) / r = (p^6 - 1)(p^2 + 1) * (p^4 - p^2 + 1) / r: the easy part by
// conjugation, inversion and Frobenius, the hard part by plain square-and-multiply.
// A line splits into what its G2 points decide (LineCoeffs: lam and c = yt - lam xt) and its
// evaluation at the G1 point; g2_line_table keeps the first part for a fixed G2 point, which
// is all the device pairing (pairing_dev.hip) needs of G2.
#pragma once
#include <utility>
#include <vector>

#include "g2.h"

namespace h2g {

inline Fq2 fq2_zero() { return {Fq::zero(), Fq::zero()}; }
inline Fq2 fq2_one() { return {Fq::one(), Fq::zero()}; }
inline Fq2 fq2_neg(const Fq2& a) { return {Fq::zero() - a.c0, Fq::zero() - a.c1}; }
inline Fq2 fq2_conj(const Fq2& a) { return {a.c0, Fq::zero() - a.c1}; }
inline Fq2 fq2_scale(const Fq2& a, const Fq& k) { return {a.c0 * k, a.c1 * k}; }
// a * xi = (a0 + a1 u)(9 + u) = 9 a0 - a1 + (9 a1 + a0) u
inline Fq2 fq2_mul_xi(const Fq2& a) {
  const Fq a0_8 = dbl(dbl(dbl(a.c0))), a1_8 = dbl(dbl(dbl(a.c1)));
  return {a0_8 + a.c0 - a.c1, a1_8 + a.c1 + a.c0};
}
// a^e, e as `words` little-endian 32-bit limbs
inline Fq2 fq2_pow_words(const Fq2& a, const uint32_t* e, int words) {
  Fq2 acc = fq2_one();
  for (int i = words - 1; i >= 0; i--)
    for (int b = 31; b >= 0; b--) {
      acc = fq2_sqr(acc);
      if ((e[i] >> b) & 1) acc = fq2_mul(acc, a);
    }
  return acc;
}

// ---------------------------------------------------------------- Fq6 = Fq2[v] / (v^3 - xi)
struct Fq6 {
  Fq2 c[3];
};
inline Fq6 fq6_add(const Fq6& a, const Fq6& b) {
  return {{fq2_add(a.c[0], b.c[0]), fq2_add(a.c[1], b.c[1]), fq2_add(a.c[2], b.c[2])}};
}
inline Fq6 fq6_sub(const Fq6& a, const Fq6& b) {
  return {{fq2_sub(a.c[0], b.c[0]), fq2_sub(a.c[1], b.c[1]), fq2_sub(a.c[2], b.c[2])}};
}
inline Fq6 fq6_neg(const Fq6& a) { return {{fq2_neg(a.c[0]), fq2_neg(a.c[1]), fq2_neg(a.c[2])}}; }
inline Fq6 fq6_mul(const Fq6& a, const Fq6& b) {
  const Fq2 t0 = fq2_mul(a.c[0], b.c[0]), t1 = fq2_mul(a.c[1], b.c[1]), t2 = fq2_mul(a.c[2], b.c[2]);
  const Fq2 m01 = fq2_add(fq2_mul(a.c[0], b.c[1]), fq2_mul(a.c[1], b.c[0]));
  const Fq2 m02 = fq2_add(fq2_mul(a.c[0], b.c[2]), fq2_mul(a.c[2], b.c[0]));
  const Fq2 m12 = fq2_add(fq2_mul(a.c[1], b.c[2]), fq2_mul(a.c[2], b.c[1]));
  return {{fq2_add(t0, fq2_mul_xi(m12)), fq2_add(m01, fq2_mul_xi(t2)), fq2_add(m02, t1)}};
}
inline Fq6 fq6_mul_v(const Fq6& a) { return {{fq2_mul_xi(a.c[2]), a.c[0], a.c[1]}}; }
inline Fq6 fq6_inv(const Fq6& a) {
  // adjugate: A = a0^2 - xi a1 a2, B = xi a2^2 - a0 a1, C = a1^2 - a0 a2; norm = a0 A + xi (a2 B + a1 C)
  const Fq2 A = fq2_sub(fq2_sqr(a.c[0]), fq2_mul_xi(fq2_mul(a.c[1], a.c[2])));
  const Fq2 B = fq2_sub(fq2_mul_xi(fq2_sqr(a.c[2])), fq2_mul(a.c[0], a.c[1]));
  const Fq2 C = fq2_sub(fq2_sqr(a.c[1]), fq2_mul(a.c[0], a.c[2]));
  const Fq2 nrm = fq2_add(fq2_mul(a.c[0], A), fq2_mul_xi(fq2_add(fq2_mul(a.c[2], B), fq2_mul(a.c[1], C))));
  const Fq2 ni = fq2_inv(nrm);
  return {{fq2_mul(A, ni), fq2_mul(B, ni), fq2_mul(C, ni)}};
}

// ---------------------------------------------------------------- Fq12 = Fq2[w] / (w^6 - xi)
struct Fq12 {
  Fq2 c[6];  // coefficients of 1, w, .., w^5
};
inline Fq12 fq12_one() {
  Fq12 r;
  r.c[0] = fq2_one();
  for (int i = 1; i < 6; i++) r.c[i] = fq2_zero();
  return r;
}
inline bool fq12_eq(const Fq12& a, const Fq12& b) {
  for (int i = 0; i < 6; i++)
    if (!fq2_eq(a.c[i], b.c[i])) return false;
  return true;
}
inline bool fq12_is_one(const Fq12& a) { return fq12_eq(a, fq12_one()); }
inline Fq6 fq12_even(const Fq12& a) { return {{a.c[0], a.c[2], a.c[4]}}; }
inline Fq6 fq12_odd(const Fq12& a) { return {{a.c[1], a.c[3], a.c[5]}}; }
inline Fq12 fq12_from(const Fq6& e, const Fq6& o) { return {{e.c[0], o.c[0], e.c[1], o.c[1], e.c[2], o.c[2]}}; }
inline Fq12 fq12_mul(const Fq12& a, const Fq12& b) {
  Fq2 t[11];
  for (auto& x : t) x = fq2_zero();
  for (int i = 0; i < 6; i++) {
    if (fq2_is_zero(a.c[i])) continue;
    for (int j = 0; j < 6; j++) {
      if (fq2_is_zero(b.c[j])) continue;  // the Miller loop's lines have three coefficients
      t[i + j] = fq2_add(t[i + j], fq2_mul(a.c[i], b.c[j]));
    }
  }
  Fq12 r;
  for (int k = 0; k < 6; k++) r.c[k] = k + 6 < 11 ? fq2_add(t[k], fq2_mul_xi(t[k + 6])) : t[k];
  return r;
}
inline Fq12 fq12_sqr(const Fq12& a) { return fq12_mul(a, a); }
// (e + o w)^-1 = (e - o w) / (e^2 - v o^2)
inline Fq12 fq12_inv(const Fq12& a) {
  const Fq6 e = fq12_even(a), o = fq12_odd(a);
  const Fq6 d = fq6_inv(fq6_sub(fq6_mul(e, e), fq6_mul_v(fq6_mul(o, o))));
  return fq12_from(fq6_mul(e, d), fq6_neg(fq6_mul(o, d)));
}
// a^(p^6): w^(p^6) = -w
inline Fq12 fq12_conj(const Fq12& a) {
  Fq12 r = a;
  for (int i = 1; i < 6; i += 2) r.c[i] = fq2_neg(a.c[i]);
  return r;
}

// gamma[i] = xi^(i (p - 1) / 6): w^p = gamma[1] w, so (sum c_i w^i)^p = sum conj(c_i) gamma[i] w^i
struct PairingConsts {
  Fq2 gamma[6];
  PairingConsts() {
    static constexpr uint32_t P16[8] = {0x2414d4e1u, 0x34b01759u, 0xe6bda1c2u, 0xee9591c2u,
                                        0xc0403964u, 0xf40d60f3u, 0xd032f006u, 0x0810b7bdu};  // (p - 1) / 6
    const Fq2 xi{from_u64<FqParams>(9), Fq::one()};
    gamma[0] = fq2_one();
    gamma[1] = fq2_pow_words(xi, P16, 8);
    for (int i = 2; i < 6; i++) gamma[i] = fq2_mul(gamma[i - 1], gamma[1]);
  }
};
inline const PairingConsts& pairing_consts() {
  static const PairingConsts c;
  return c;
}
inline Fq12 fq12_frobenius(const Fq12& a) {
  const PairingConsts& k = pairing_consts();
  Fq12 r;
  for (int i = 0; i < 6; i++) r.c[i] = fq2_mul(fq2_conj(a.c[i]), k.gamma[i]);
  return r;
}
inline Fq12 fq12_pow_words(const Fq12& a, const uint32_t* e, int words) {
  Fq12 acc = fq12_one();
  bool started = false;
  for (int i = words - 1; i >= 0; i--)
    for (int b = 31; b >= 0; b--) {
      if (started) acc = fq12_sqr(acc);
      if ((e[i] >> b) & 1) {
        acc = started ? fq12_mul(acc, a) : a;
        started = true;
      }
    }
  return acc;
}

// ---------------------------------------------------------------- Miller loop
struct PairingPair {
  G1Affine p;
  G2Affine q;
};
// what a Miller-loop line keeps of its G2 points: l(xp, yp) = -yp + (lam xp) w + c w^3
struct LineCoeffs {
  Fq2 lam, c;
};
// 6u + 2 = 2^64 + ATE_LO; a line table has one doubling line per bit of ATE_LO, one addition
// line per set bit and the two closing lines
static constexpr uint64_t ATE_LO = 0x9d797039be763ba8ull;
static constexpr int ATE_LINES = 64 + 36 + 2;
namespace pairing_detail {
// the line through the twisted points t and q (the tangent when they are equal), the part that
// the G2 points alone decide: its slope lam and c = yt - lam xt, and t <- t + q.
// false: a vertical line (points outside the r-torsion)
inline bool line_coeffs(G2Affine* t, const G2Affine& q, LineCoeffs* out) {
  Fq2 lam;
  if (fq2_eq(t->x, q.x) && fq2_eq(t->y, q.y)) {
    const Fq2 x2 = fq2_sqr(t->x);
    if (fq2_is_zero(t->y)) return false;
    lam = fq2_mul(fq2_add(fq2_dbl(x2), x2), fq2_inv(fq2_dbl(t->y)));
  } else if (fq2_eq(t->x, q.x)) {
    return false;
  } else {
    lam = fq2_mul(fq2_sub(q.y, t->y), fq2_inv(fq2_sub(q.x, t->x)));
  }
  out->lam = lam;
  out->c = fq2_sub(t->y, fq2_mul(lam, t->x));
  const Fq2 x3 = fq2_sub(fq2_sub(fq2_sqr(lam), t->x), q.x);
  const Fq2 y3 = fq2_sub(fq2_mul(lam, fq2_sub(t->x, x3)), t->y);
  t->x = x3;
  t->y = y3;
  return true;
}
// that line at the G1 point (xp, yp): l = -yp + (lam xp) w + c w^3
inline void line_eval(const LineCoeffs& lc, const Fq& xp, const Fq& yp, Fq12* out) {
  for (auto& c : out->c) c = fq2_zero();
  out->c[0] = {Fq::zero() - yp, Fq::zero()};
  out->c[1] = fq2_scale(lc.lam, xp);
  out->c[3] = lc.c;
}
inline bool line(G2Affine* t, const G2Affine& q, const Fq& xp, const Fq& yp, Fq12* out) {
  LineCoeffs lc;
  if (!line_coeffs(t, q, &lc)) return false;
  line_eval(lc, xp, yp, out);
  return true;
}
inline G2Affine frob_twist(const G2Affine& q) {
  const PairingConsts& k = pairing_consts();
  return {fq2_mul(fq2_conj(q.x), k.gamma[2]), fq2_mul(fq2_conj(q.y), k.gamma[3])};
}
}  // namespace pairing_detail

// prod_i f_{6u+2, Q_i}(P_i) with the closing lines; pairs with an identity on either side
// contribute 1.  false: a vertical line was met (a G2 point outside the r-torsion).
inline bool miller_loop(const std::vector<PairingPair>& pairs, Fq12* out) {
  std::vector<const PairingPair*> live;
  for (const auto& pr : pairs)
    if (!pr.p.is_identity() && !pr.q.is_identity()) live.push_back(&pr);
  Fq12 f = fq12_one(), ln;
  std::vector<G2Affine> t;
  for (const auto* pr : live) t.push_back(pr->q);
  for (int i = 63; i >= 0; i--) {
    f = fq12_sqr(f);
    for (size_t j = 0; j < live.size(); j++) {
      if (!pairing_detail::line(&t[j], t[j], live[j]->p.x, live[j]->p.y, &ln)) return false;
      f = fq12_mul(f, ln);
    }
    if ((ATE_LO >> i) & 1)
      for (size_t j = 0; j < live.size(); j++) {
        if (!pairing_detail::line(&t[j], live[j]->q, live[j]->p.x, live[j]->p.y, &ln)) return false;
        f = fq12_mul(f, ln);
      }
  }
  for (size_t j = 0; j < live.size(); j++) {
    const G2Affine q1 = pairing_detail::frob_twist(live[j]->q);
    G2Affine nq2 = pairing_detail::frob_twist(q1);
    nq2.y = fq2_neg(nq2.y);
    if (!pairing_detail::line(&t[j], q1, live[j]->p.x, live[j]->p.y, &ln)) return false;
    f = fq12_mul(f, ln);
    if (!pairing_detail::line(&t[j], nq2, live[j]->p.x, live[j]->p.y, &ln)) return false;
    f = fq12_mul(f, ln);
  }
  *out = f;
  return true;
}

// The lines of miller_loop for one fixed G2 point, in the loop's order: for every bit of
// ATE_LO from the top the doubling line, then the addition line where the bit is set, then the
// two Frobenius-twisted closing lines (ATE_LINES in all).  With both G2 arguments of a check
// fixed, the Miller loop needs no G2 arithmetic: pairing_dev.hip reads these tables.
// false: a vertical line was met (a G2 point outside the r-torsion), or q is the identity.
inline bool g2_line_table(const G2Affine& q, std::vector<LineCoeffs>* out) {
  out->clear();
  if (q.is_identity()) return false;
  G2Affine t = q;
  LineCoeffs lc;
  for (int i = 63; i >= 0; i--) {
    if (!pairing_detail::line_coeffs(&t, t, &lc)) return false;
    out->push_back(lc);
    if ((ATE_LO >> i) & 1) {
      if (!pairing_detail::line_coeffs(&t, q, &lc)) return false;
      out->push_back(lc);
    }
  }
  const G2Affine q1 = pairing_detail::frob_twist(q);
  G2Affine nq2 = pairing_detail::frob_twist(q1);
  nq2.y = fq2_neg(nq2.y);
  if (!pairing_detail::line_coeffs(&t, q1, &lc)) return false;
  out->push_back(lc);
  if (!pairing_detail::line_coeffs(&t, nq2, &lc)) return false;
  out->push_back(lc);
  return true;
}

// f_{6u+2, Q}(P) with the closing lines from Q's line table: the value miller_loop gives for
// the one pair (P, Q), and the order of operations the device kernel follows; 1 when P is the
// identity
inline Fq12 miller_from_lines(const std::vector<LineCoeffs>& tab, const G1Affine& p) {
  Fq12 f = fq12_one(), ln;
  if (p.is_identity() || tab.size() != (size_t)ATE_LINES) return f;
  size_t k = 0;
  for (int i = 63; i >= 0; i--) {
    f = fq12_sqr(f);
    pairing_detail::line_eval(tab[k++], p.x, p.y, &ln);
    f = fq12_mul(f, ln);
    if ((ATE_LO >> i) & 1) {
      pairing_detail::line_eval(tab[k++], p.x, p.y, &ln);
      f = fq12_mul(f, ln);
    }
  }
  for (int j = 0; j < 2; j++) {
    pairing_detail::line_eval(tab[k++], p.x, p.y, &ln);
    f = fq12_mul(f, ln);
  }
  return f;
}

inline Fq12 final_exponentiation(const Fq12& f) {
  // (p^4 - p^2 + 1) / r, 761 bits
  static constexpr uint32_t HARD[24] = {
      0xccdf42b1u, 0xe81bb482u, 0xf49c36d4u, 0x5abf5cc4u, 0x1da014fdu, 0xf1154e7eu, 0x87cdbacfu, 0xdcc7b44cu,
      0x954bcf8au, 0xaaa441e3u, 0xd5095f23u, 0x6b887d56u, 0xf3fd90c6u, 0x79581e16u, 0xd189227du, 0x3b1b1355u,
      0x61876f6bu, 0x4e529a58u, 0xd5b12278u, 0x6c0eb522u, 0x83177fafu, 0x331ec151u, 0x0b0759adu, 0x01baaa71u};
  const Fq12 a = fq12_mul(fq12_conj(f), fq12_inv(f));           // f^(p^6 - 1)
  const Fq12 b = fq12_mul(fq12_frobenius(fq12_frobenius(a)), a);  // ^(p^2 + 1)
  return fq12_pow_words(b, HARD, 24);
}

// e(P, Q); 1 when either is the identity.  false on a vertical line.
inline bool pairing(const G1Affine& p, const G2Affine& q, Fq12* out) {
  Fq12 f;
  const std::vector<PairingPair> one(1, PairingPair{p, q});
  if (!miller_loop(one, &f)) return false;
  *out = final_exponentiation(f);
  return true;
}

// prod_i e(P_i, Q_i) == 1, one final exponentiation; e(identity, Q) = 1
inline bool pairing_check(const std::vector<PairingPair>& pairs) {
  Fq12 f;
  if (!miller_loop(pairs, &f)) return false;
  return fq12_is_one(final_exponentiation(f));
}

}  // namespace h2g
