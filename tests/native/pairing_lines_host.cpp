// pairing_lines_host.cpp -- csrc/pairing.h's line tables driven on the host (test harness only).
//
// Built by tests/test_pairing_lines_cpu.py with hipcc for the host side only.  Reads one
// operation per line from stdin, every Fq as a canonical hexadecimal integer (a G1 point: x y,
// the identity 0 0; a G2 point: x.c0 x.c1 y.c0 y.c1), and prints the result on one line.
//   lines Q          -> the number of lines of Q's table, or VERT
//   miller P Q       -> the Miller value assembled from Q's table at P (12 values), or VERT
//   loop P Q         -> miller_loop's value for the one pair (12 values), or VERT
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
  G1Affine p;
  G2Affine q;
  std::vector<LineCoeffs> tab;
  if (op == "lines") {
    if (!rdg2(in, q)) return false;
    if (g2_line_table(q, &tab)) printf("%zu", tab.size());
    else printf("VERT");
  } else if (op == "miller") {
    if (!rdg1(in, p) || !rdg2(in, q)) return false;
    if (g2_line_table(q, &tab)) wr12(miller_from_lines(tab, p));
    else printf("VERT");
  } else if (op == "loop") {
    if (!rdg1(in, p) || !rdg2(in, q)) return false;
    Fq12 f;
    if (miller_loop(std::vector<PairingPair>(1, PairingPair{p, q}), &f)) wr12(f);
    else printf("VERT");
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
