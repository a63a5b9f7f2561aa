// pairing_host.cpp -- csrc/pairing.h driven on the host (test harness only).
//
// Built by tests/test_pairing_host_cpu.py with hipcc for the host side only.  Reads one
// operation per line from stdin, "op values...", every Fq as a canonical hexadecimal integer
// (an Fq12: 12 values, c0.c0 c0.c1 c1.c0 ..; a G1 point: x y, the identity 0 0; a G2 point:
// x.c0 x.c1 y.c0 y.c1) and prints the result's values the same way on one line.
//   f12mul a b | f12inv a | f12frob a          -> Fq12
//   pairing P Q                                -> Fq12, or VERT
//   check n (P Q) x n                          -> 0 / 1
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "pairing.h"

using namespace h2g;

static bool rd(std::istringstream& in, Fq& v) {
  std::string s;
  if (!(in >> s) || s.size() > 64) return false;
  Fq c = Fq::zero();
  int nib = 0;
  for (int i = (int)s.size() - 1; i >= 0; i--, nib++) {
    const char ch = s[i];
    const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
    if (d < 0) return false;
    c.l[nib / 8] |= (uint32_t)d << (4 * (nib % 8));
  }
  v = from_canonical(c);
  return true;
}
static bool rd2(std::istringstream& in, Fq2& v) { return rd(in, v.c0) && rd(in, v.c1); }
static bool rd12(std::istringstream& in, Fq12& v) {
  for (auto& c : v.c)
    if (!rd2(in, c)) return false;
  return true;
}
static bool rdg1(std::istringstream& in, G1Affine& p) { return rd(in, p.x) && rd(in, p.y); }
static bool rdg2(std::istringstream& in, G2Affine& q) { return rd2(in, q.x) && rd2(in, q.y); }
static void wr(const Fq& v) {
  const Fq c = to_canonical(v);
  for (int i = 7; i >= 0; i--) printf("%08x", c.l[i]);
}
static void wr12(const Fq12& v) {
  for (int i = 0; i < 6; i++) {
    if (i) printf(" ");
    wr(v.c[i].c0), printf(" "), wr(v.c[i].c1);
  }
}

static bool run(const std::string& op, std::istringstream& in) {
  Fq12 a, b;
  if (op == "f12mul") {
    if (!rd12(in, a) || !rd12(in, b)) return false;
    wr12(fq12_mul(a, b));
  } else if (op == "f12inv") {
    if (!rd12(in, a)) return false;
    wr12(fq12_inv(a));
  } else if (op == "f12frob") {
    if (!rd12(in, a)) return false;
    wr12(fq12_frobenius(a));
  } else if (op == "pairing") {
    G1Affine p;
    G2Affine q;
    if (!rdg1(in, p) || !rdg2(in, q)) return false;
    if (pairing(p, q, &a)) wr12(a);
    else printf("VERT");
  } else if (op == "check") {
    int n;
    if (!(in >> n) || n < 0 || n > 64) return false;
    std::vector<PairingPair> pairs(n);
    for (auto& pr : pairs)
      if (!rdg1(in, pr.p) || !rdg2(in, pr.q)) return false;
    printf("%d", (int)pairing_check(pairs));
  } else {
    return false;
  }
  return true;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    if (!run(op, in)) printf("ERR %s", op.c_str());
    printf("\n");
  }
  return 0;
}
