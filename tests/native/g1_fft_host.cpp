// g1_fft_host.cpp -- the G1 group FFT of csrc/g1_fft.h driven on the host (test harness only;
// the pattern of f29_acc_host.cpp).
//
// Built by tests/test_g1_fft_host_cpu.py with hipcc for the host side only, once plainly and
// once with the address and undefined-behaviour sanitisers.  Reads one transform per line from
// stdin,
//   fft k  omega_inv (4 u64, Montgomery)  n_inv (4 u64, canonical)  2^k points (8 u64 each)
// and prints the 2^k output points on one line.  The transform is the kernels': the twiddle
// table omega^-x (canonical), the bit-reversal swaps, then stage by stage every butterfly t in
// launch order through g1fft_stage_one -- with the twiddle of its wave's first butterfly
// where g1fft_stage_uniform says the wave shares one -- and the scaling by n^-1.
//   map k s t -> twiddle index, lo index, hi index of butterfly t of stage s
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "g1_fft.h"

using namespace h2g;

template <class F>
static bool rd(std::istringstream& in, F& v) {
  for (int i = 0; i < 4; i++) {
    uint64_t x;
    if (!(in >> x)) return false;
    v.l[2 * i] = (uint32_t)x;
    v.l[2 * i + 1] = (uint32_t)(x >> 32);
  }
  return true;
}
static void wr(const Fq& v) {
  for (int i = 0; i < 4; i++) printf("%llu ", (unsigned long long)((uint64_t)v.l[2 * i] | (uint64_t)v.l[2 * i + 1] << 32));
}

static bool fft(std::istringstream& in) {
  uint32_t k;
  Fr omega_inv, ninv;
  if (!(in >> k) || k < 1 || k > 12 || !rd(in, omega_inv) || !rd(in, ninv)) return false;
  const uint64_t n = 1ull << k;
  std::vector<G1Affine> p(n);
  for (auto& q : p)
    if (!rd(in, q.x) || !rd(in, q.y)) return false;
  std::vector<Fr> tw(n / 2);
  Fr w = Fr::one();
  for (uint64_t x = 0; x < n / 2; x++) {
    tw[x] = to_canonical(w);
    w = w * omega_inv;
  }
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t r = g1fft_bitrev(i, k);
    if (r >= n) return false;
    if (i < r) std::swap(p[i], p[r]);
  }
  for (uint32_t s = 1; s <= k; s++)
    for (uint64_t t = 0; t < n / 2; t++) {
      const uint64_t t_tw = g1fft_stage_uniform(k, s) ? t - t % G1FFT_WAVE : t;
      // what the kernel would touch, checked before it is touched
      const uint64_t lo = g1fft_lo_index(t, k, s), hi = lo + g1fft_half(s);
      if (hi >= n || g1fft_twiddle_index(t_tw, k, s) >= n / 2) return false;
      g1fft_stage_one(p.data(), tw.data(), k, s, t_tw, t);
    }
  for (auto& q : p) q = g1fft_scale(q, ninv);
  for (const auto& q : p) wr(q.x), wr(q.y);
  return true;
}

static bool map(std::istringstream& in) {
  uint32_t k, s;
  uint64_t t;
  if (!(in >> k >> s >> t) || s < 1 || s > k || k > G1FFT_MAX_K || t >= (1ull << k) / 2) return false;
  const uint64_t lo = g1fft_lo_index(t, k, s);
  printf("%llu %llu %llu %d", (unsigned long long)g1fft_twiddle_index(t, k, s), (unsigned long long)lo,
         (unsigned long long)(lo + g1fft_half(s)), (int)g1fft_stage_uniform(k, s));
  return true;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    const bool ok = op == "fft" ? fft(in) : (op == "map" ? map(in) : false);
    if (!ok) printf("ERR %s", op.c_str());
    printf("\n");
  }
  return 0;
}
