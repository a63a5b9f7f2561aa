// f29_acc_host.cpp -- the accumulation's hot-loop forms of csrc/f29.h driven on the host
// (test harness only; the pattern of f29_host.cpp).
//
// Built by tests/test_f29_acc_host_cpu.py with hipcc for the host side only, once plainly and
// once with the address and undefined-behaviour sanitisers.  Reads one operation per line
// from stdin, "op limbs...", every F29 value as 9 decimal 32-bit limbs (a point: X Y ZZ ZZZ,
// 36 limbs), and prints the result's limbs on one line:
//   madda  p qx qy   -> status, then p after xyzz29_madd_acc (37 numbers)
//   chain  n p (qx qy) x n -> status of the last step, then p after n hot-loop steps; a step
//                      whose status is not 0 starts the next one afresh, as the kernel does
//   subn64 / subn32  a b -> subn29<Fq, 64 / 32>(a, b)
//   mula a b, sqra a, mulx2a a b c d -> the carry-chained products
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "f29.h"

using namespace h2g;

static bool rd(std::istringstream& in, F29& v) {
  for (int i = 0; i < 9; i++)
    if (!(in >> v.l[i])) return false;
  return true;
}
static bool rdp(std::istringstream& in, G1xyzz29& p) { return rd(in, p.X) && rd(in, p.Y) && rd(in, p.ZZ) && rd(in, p.ZZZ); }
static void wr(const F29& v) {
  for (int i = 0; i < 9; i++) printf("%s%u", i ? " " : "", v.l[i]);
}
static void wrp(const G1xyzz29& p) {
  wr(p.X), printf(" "), wr(p.Y), printf(" "), wr(p.ZZ), printf(" "), wr(p.ZZZ);
}

static bool run(const std::string& op, std::istringstream& in) {
  F29 a, b, c, d;
  G1xyzz29 p;
  if (op == "madda") {
    if (!rdp(in, p) || !rd(in, a) || !rd(in, b)) return false;
    const int st = xyzz29_madd_acc(p, a, b);
    printf("%d ", st);
    wrp(p);
  } else if (op == "chain") {
    int n;
    if (!(in >> n) || !rdp(in, p)) return false;
    int st = 0;
    bool fresh = false;
    for (int i = 0; i < n; i++) {
      if (!rd(in, a) || !rd(in, b)) return false;
      if (fresh) {
        p.X = a, p.Y = b, p.ZZ = one29v<FqParams>(), p.ZZZ = p.ZZ;
        st = 0;
      } else {
        st = xyzz29_madd_acc(p, a, b);
      }
      fresh = st != 0;
    }
    printf("%d ", st);
    wrp(p);
  } else if (op == "subn64" || op == "subn32") {
    if (!rd(in, a) || !rd(in, b)) return false;
    wr(op == "subn64" ? subn29<FqParams, 64>(a, b) : subn29<FqParams, 32>(a, b));
  } else if (op == "mula") {
    if (!rd(in, a) || !rd(in, b)) return false;
    wr(mul29_acc<FqParams>(a, b));
  } else if (op == "sqra") {
    if (!rd(in, a)) return false;
    wr(sqr29_acc<FqParams>(a));
  } else if (op == "mulx2a") {
    if (!rd(in, a) || !rd(in, b) || !rd(in, c) || !rd(in, d)) return false;
    wr(mul29x2_acc<FqParams>(a, b, c, d));
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
