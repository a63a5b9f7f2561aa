// verifier.cpp -- verify_proof and the batch verifier (h2g_verify_proof / h2g_verify_batch),
// the verifying-key handles and ParamsVerifierKZG.
//
// A C++ restatement of
//   verify_proof                     halo2_backend/src/plonk/verifier.rs:58-512
//   vanishing verifier               plonk/vanishing/verifier.rs:40-137
//   permutation verifier             plonk/permutation/verifier.rs:33-253
//   lookup / shuffle verifiers       plonk/lookup/verifier.rs, plonk/shuffle/verifier.rs
//   VerifierSHPLONK / VerifierGWC    poly/kzg/multiopen/** -- multiopen.cpp (multiopen_verify_terms), shared
//                                    with h2g_multiopen_verify below
//   l_i_range                        poly/domain.rs:425-450
//   DualMSM::check                   poly/kzg/msm.rs:188-206
// The device pairing (pairing_dev.hip) serves h2g_pairing_check_batch and, when
// h2g_verify_set_isolation(1) is set, gives a failing batch's proofs their verdicts in one launch.
// (oracle/py/verifier.py restates the same sources in Python and is what the tests compare
// verdicts with).
//
// Split of the work.  The proof's layout is fixed by the key, the circuit count and the
// multi-open scheme, so every 32-byte point encoding of every proof is found without hashing:
// all of them are decompressed by one g1_decompress launch into the tail of one base array
// whose head holds g1 and the key's commitments.  The host then runs each proof's transcript
// and scalar arithmetic (a few thousand field operations) and emits the DualMSM's two sums as
// (base index, scalar) terms; one segmented MSM (msm_seg.hip) evaluates them all; the host
// pairing (pairing.h) decides.  A point is referred to by its index, never copied.
#include <sys/random.h>

#include "msm_seg.h"
#include "multiopen.h"
#include "pairing.h"
#include "pairing_dev.h"
#include "vanishing.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace h2g {
namespace prv {
std::map<uint64_t, std::unique_ptr<VerifyingKey>> g_vks;
}
}  // namespace h2g

namespace {
constexpr uint32_t KEY_H = 0xFFFFFFFFu;  // the query key of the h(X) MSM (no single base)

double g_verify_ms[4] = {0, 0, 0, 0};  // host, decompression, MSM, pairing of the last call
int g_isolation = 0;                   // h2g_verify_set_isolation

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct DevMem {
  void* p = nullptr;
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
};

bool fr_below(const Fr& a) {
  unsigned br = 0;
  for (int i = 0; i < 8; i++) (void)__builtin_subc(a.l[i], FrParams::M[i], br, &br);
  return br != 0;
}
bool fq_below_m(const Fq& a) {
  unsigned br = 0;
  for (int i = 0; i < 8; i++) (void)__builtin_subc(a.l[i], FqParams::M[i], br, &br);
  return br != 0;
}


// ------------------------------------------------------------------ what the key fixes
struct Shape {
  const VerifyingKey* vk;
  int NC, multiopen, transcript;
  size_t n;
  int qpd;  // quotient_poly_degree: the number of h pieces
  Fr omega, omega_inv, bary;
  size_t head_pts, scalars, tail_pts;  // the proof: head points, evaluations, multi-open points
  std::vector<int> rots;               // distinct rotations (mod n) of the queries, first appearance
  size_t proof_len() const { return 32 * (head_pts + scalars + tail_pts); }
  size_t pts() const { return head_pts + tail_pts; }
  int rot_id(int rot) const {
    const int r = (int)(((int64_t)rot % (int64_t)n + (int64_t)n) % (int64_t)n);
    for (size_t i = 0; i < rots.size(); i++)
      if (rots[i] == r) return (int)i;
    return -1;
  }
  uint32_t base_fixed(int i) const { return 1 + (uint32_t)i; }
  uint32_t base_perm(int i) const { return 1 + (uint32_t)vk->cs.F + (uint32_t)i; }
};

// the rotations of the queries in verify_proof's order (verifier.rs:395-470)
void shape_rotations(Shape& s) {
  const CsHost& cs = s.vk->cs;
  auto add = [&](int rot) {
    const int r = (int)(((int64_t)rot % (int64_t)s.n + (int64_t)s.n) % (int64_t)s.n);
    if (std::find(s.rots.begin(), s.rots.end(), r) == s.rots.end()) s.rots.push_back(r);
  };
  for (const auto& q : cs.adv_q) add(q.rot);
  if (cs.nsets) {
    add(0);
    add(1);
    if (cs.nsets > 1) add(-(cs.bf + 1));
  }
  if (cs.NL) {
    add(0);
    add(-1);
    add(1);
  }
  if (cs.NS) {
    add(0);
    add(1);
  }
  for (const auto& q : cs.fix_q) add(q.rot);
  add(0);  // sigma, h and the random polynomial
}

int shape_init(Shape& s, const VerifyingKey& vk, int NC, int multiopen, int transcript) {
  const CsHost& cs = vk.cs;
  s.vk = &vk;
  s.NC = NC;
  s.multiopen = multiopen;
  s.transcript = transcript;
  s.n = (size_t)1 << cs.k;
  s.qpd = cs.degree - 1;
  Fr o = root_of_unity();
  for (uint32_t i = cs.k; i < FR_S; i++) o = sqr(o);
  s.omega = o;
  s.omega_inv = inv(o);
  s.bary = inv(from_u64<FrParams>(s.n));
  const size_t nc = (size_t)NC;
  s.head_pts = nc * cs.A + nc * cs.NL * 2 + nc * cs.nsets + nc * cs.NL + nc * cs.NS + 1 + (size_t)s.qpd;
  s.scalars = nc * cs.adv_q.size() + cs.fix_q.size() + 1 + (size_t)cs.P +
              nc * (cs.nsets ? 3 * (size_t)cs.nsets - 1 : 0) + nc * cs.NL * 5 + nc * cs.NS * 2;
  shape_rotations(s);
  s.tail_pts = multiopen == MULTIOPEN_GWC ? s.rots.size() : 2;
  return H2G_OK;
}

// ------------------------------------------------------------------ one proof on the host
struct ProofReader {
  const Shape& sh;
  const uint8_t* proof;
  const G1Affine* pts;  // this proof's decompressed points, head then tail
  uint32_t base0;       // base index of pts[0]
  Transcript T;
  size_t pi = 0, si = 0;
  bool ok = true;
  ProofReader(const Shape& s, const uint8_t* p, const G1Affine* q, uint32_t b0)
      : sh(s), proof(p), pts(q), base0(b0), T(nullptr, s.transcript) {}
  // TranscriptRead::read_point: the decoded point (an identity here is a failed decoding or
  // the point at infinity, which common_point refuses); returns its base index
  uint32_t read_point() {
    if (pi >= sh.pts()) return ok = false, 0;
    const G1Affine& p = pts[pi];
    if (!T.common_point(p)) ok = false;
    return base0 + (uint32_t)pi++;
  }
  Fr read_scalar() {  // from_repr refuses values >= r
    if (si >= sh.scalars) return ok = false, Fr::zero();
    Fr c;
    std::memcpy(c.l, proof + 32 * (sh.head_pts + si), 32);
    si++;
    if (!fr_below(c)) return ok = false, Fr::zero();
    const Fr v = from_canonical(c);
    T.common_scalar(v);
    return v;
  }
};

// fills left / right with the DualMSM's terms; false: the proof is malformed
bool proof_terms(const Shape& sh, const h2g_verify_item& it, const G1Affine* pts, uint32_t base0, Msm* left_out,
                 Msm* right_out) {
  const CsHost& cs = sh.vk->cs;
  const int NC = sh.NC, nsets = cs.nsets, NL = cs.NL, NS = cs.NS;
  const size_t n = sh.n;
  ProofReader R(sh, it.proof, pts, base0);
  Transcript& T = R.T;
  // instances (verifier.rs:70-102)
  if (cs.I && (!it.instance || !it.instance_lens)) return false;
  std::vector<std::vector<std::vector<Fr>>> inst(NC, std::vector<std::vector<Fr>>(cs.I));
  for (int c = 0; c < NC && cs.I; c++) {
    if (!it.instance_lens[c]) return false;
    const uint64_t* v = it.instance[c];
    for (int i = 0; i < cs.I; i++) {
      const size_t len = it.instance_lens[c][i];
      if (len + (size_t)cs.bf + 1 > n) return false;  // InstanceTooLarge
      if (len && !v) return false;
      inst[c][i].resize(len);
      for (size_t j = 0; j < len; j++, v += 4) {
        inst[c][i][j] = fr_from_limbs(v);
        if (!fr_below(inst[c][i][j])) return false;
      }
    }
  }
  T.common_scalar(cs.transcript_repr);
  for (int c = 0; c < NC; c++)
    for (int i = 0; i < cs.I; i++)
      for (const Fr& v : inst[c][i]) T.common_scalar(v);
  // advice commitments per phase, circuit by circuit, each phase followed by its challenges
  std::vector<std::vector<uint32_t>> adv_cm(NC, std::vector<uint32_t>(cs.A, 0));
  std::vector<Fr> chal(cs.ch_phase.size(), Fr::zero());
  for (int ph = 0; ph <= cs.max_phase; ph++) {
    for (int c = 0; c < NC; c++)
      for (int col = 0; col < cs.A; col++)
        if (cs.adv_phase[col] == ph) adv_cm[c][col] = R.read_point();
    for (size_t i = 0; i < chal.size(); i++)
      if (cs.ch_phase[i] == ph) chal[i] = T.squeeze();
  }
  const Fr theta = T.squeeze();
  std::vector<std::vector<uint32_t>> lk_a(NC, std::vector<uint32_t>(NL)), lk_s = lk_a, lk_z = lk_a;
  for (int c = 0; c < NC; c++)
    for (int l = 0; l < NL; l++) {
      lk_a[c][l] = R.read_point();
      lk_s[c][l] = R.read_point();
    }
  const Fr beta = T.squeeze();
  const Fr gamma = T.squeeze();
  std::vector<std::vector<uint32_t>> perm_cm(NC, std::vector<uint32_t>(nsets)), sh_z(NC, std::vector<uint32_t>(NS));
  for (int c = 0; c < NC; c++)
    for (int i = 0; i < nsets; i++) perm_cm[c][i] = R.read_point();
  for (int c = 0; c < NC; c++)
    for (int l = 0; l < NL; l++) lk_z[c][l] = R.read_point();
  for (int c = 0; c < NC; c++)
    for (int l = 0; l < NS; l++) sh_z[c][l] = R.read_point();
  const uint32_t random_cm = R.read_point();
  const Fr y = T.squeeze();
  std::vector<uint32_t> h_cm(sh.qpd);
  for (auto& h : h_cm) h = R.read_point();
  const Fr x = T.squeeze();
  if (!R.ok) return false;
  const Fr xn = pow_u64(x, n);
  // the proof's values at x (vanishing.h): instance evaluations (QUERY_INSTANCE = false), then
  // the evaluations the proof carries
  const EvalDomain dom{n, sh.omega, sh.omega_inv, sh.bary};
  VanishingEvals E;
  E.chal = chal;
  E.theta = theta, E.beta = beta, E.gamma = gamma, E.y = y, E.x = x;
  E.ins_ev = instance_evals(cs, dom, x, xn, inst);
  E.adv_ev.assign(NC, std::vector<Fr>(cs.adv_q.size()));
  for (int c = 0; c < NC; c++)
    for (auto& e : E.adv_ev[c]) e = R.read_scalar();
  E.fix_ev.resize(cs.fix_q.size());
  for (auto& e : E.fix_ev) e = R.read_scalar();
  const Fr random_ev = R.read_scalar();
  E.perm_ev.resize(cs.P);
  for (auto& e : E.perm_ev) e = R.read_scalar();
  E.sets.assign(NC, std::vector<VanishingEvals::SetEv>(nsets));
  for (int c = 0; c < NC; c++)
    for (int i = 0; i < nsets; i++) {
      E.sets[c][i].e0 = R.read_scalar();
      E.sets[c][i].e1 = R.read_scalar();
      E.sets[c][i].e2 = i + 1 < nsets ? R.read_scalar() : Fr::zero();
    }
  E.lk_ev.assign(NC, std::vector<VanishingEvals::LkEv>(NL));
  E.sh_ev.assign(NC, std::vector<VanishingEvals::ShEv>(NS));
  for (int c = 0; c < NC; c++)
    for (auto& e : E.lk_ev[c]) {
      e.z = R.read_scalar();
      e.zn = R.read_scalar();
      e.ap = R.read_scalar();
      e.api = R.read_scalar();
      e.sp = R.read_scalar();
    }
  for (int c = 0; c < NC; c++)
    for (auto& e : E.sh_ev[c]) {
      e.z = R.read_scalar();
      e.zn = R.read_scalar();
    }
  if (!R.ok || R.si != sh.scalars) return false;

  // the vanishing argument: every circuit's expressions at x, one Horner chain in y
  const Fr one = Fr::one();
  const Fr expected_h = vanishing_expected_h(cs, dom, E);
  Msm h_msm;  // sum_i xn^i h_i
  {
    Fr p = one;
    for (uint32_t h : h_cm) {
      h_msm.push_back({h, p});
      p = p * xn;
    }
  }

  // queries, circuit by circuit, then the common ones (verifier.rs:395-470)
  const int r0 = sh.rot_id(0), r_next = sh.rot_id(1), r_prev = sh.rot_id(-1), r_last = sh.rot_id(-(cs.bf + 1));
  std::vector<VerifierQ> queries;  // key: the commitment's base index, or KEY_H; pt: index into Shape::rots
  for (int c = 0; c < NC; c++) {
    for (size_t qi = 0; qi < cs.adv_q.size(); qi++)
      queries.push_back({adv_cm[c][cs.adv_q[qi].index], sh.rot_id(cs.adv_q[qi].rot), E.adv_ev[c][qi]});
    for (int i = 0; i < nsets; i++) {
      queries.push_back({perm_cm[c][i], r0, E.sets[c][i].e0});
      queries.push_back({perm_cm[c][i], r_next, E.sets[c][i].e1});
    }
    for (int i = nsets - 2; i >= 0; i--) queries.push_back({perm_cm[c][i], r_last, E.sets[c][i].e2});
    for (int l = 0; l < NL; l++) {
      const VanishingEvals::LkEv& e = E.lk_ev[c][l];
      queries.push_back({lk_z[c][l], r0, e.z});
      queries.push_back({lk_a[c][l], r0, e.ap});
      queries.push_back({lk_s[c][l], r0, e.sp});
      queries.push_back({lk_a[c][l], r_prev, e.api});
      queries.push_back({lk_z[c][l], r_next, e.zn});
    }
    for (int l = 0; l < NS; l++) {
      queries.push_back({sh_z[c][l], r0, E.sh_ev[c][l].z});
      queries.push_back({sh_z[c][l], r_next, E.sh_ev[c][l].zn});
    }
  }
  for (size_t qi = 0; qi < cs.fix_q.size(); qi++)
    queries.push_back({sh.base_fixed(cs.fix_q[qi].index), sh.rot_id(cs.fix_q[qi].rot), E.fix_ev[qi]});
  for (int i = 0; i < cs.P; i++) queries.push_back({sh.base_perm(i), r0, E.perm_ev[i]});
  queries.push_back({KEY_H, r0, expected_h});
  queries.push_back({random_cm, r0, random_ev});
  for (const auto& q : queries)
    if (q.pt < 0) return false;  // unreachable: shape_rotations lists every rotation used here
  // the multi-open verifier's scalars (multiopen.cpp), reading this proof's tail points
  MultiopenVerifyIo io;
  io.T = &T;
  io.point.resize(sh.rots.size());
  for (size_t i = 0; i < io.point.size(); i++) io.point[i] = x * pow_u64(sh.omega, (uint64_t)sh.rots[i]);
  io.read_point = [&R] { return R.read_point(); };
  io.ok = [&R] { return R.ok; };
  io.add_obj = [&h_msm](Msm& m, uint32_t key, const Fr& f) {  // f * (the commitment or the h MSM)
    if (key == KEY_H)
      for (const auto& t : h_msm) m.push_back({t.base, t.s * f});
    else m.push_back({key, f});
  };
  io.expect_groups = (long)sh.tail_pts;  // GWC: one witness point per distinct rotation
  Msm left, right;
  if (!multiopen_verify_terms(sh.multiopen, queries, io, &left, &right)) return false;
  if (R.pi != sh.pts()) return false;
  msm_merge(left);
  msm_merge(right);
  *left_out = std::move(left);
  *right_out = std::move(right);
  return true;
}

// ------------------------------------------------------------------ the r_i
bool draw_nonzero(const h2g_rng* rng, Fr* out) {
  for (int tries = 0; tries < 64; tries++) {
    Fr r;
    if (rng && rng->random_fr) {
      uint64_t v[4] = {0, 0, 0, 0};
      if (rng->random_fr(rng->ctx, v) != 0) return false;
      r = fr_from_limbs(v);
      if (!fr_below(r)) return false;
    } else {
      uint32_t w[16];
      if (rng) {
        if (!rng->fill_bytes || rng->fill_bytes(rng->ctx, reinterpret_cast<uint8_t*>(w), 64) != 0) return false;
      } else {
        size_t got = 0;
        while (got < 64) {
          const ssize_t k = getrandom(reinterpret_cast<uint8_t*>(w) + got, 64 - got, 0);
          if (k <= 0) return false;
          got += (size_t)k;
        }
      }
      r = fr_from_u512(w);
    }
    if (!r.is_zero()) {
      *out = r;
      return true;
    }
  }
  return false;
}

struct VerifierPoints {
  G1Affine g1;
  G2Affine g2, s_g2;
};
int load_vp(const h2g_verifier_params* vp, VerifierPoints* out) {
  if (!vp) return fail(H2G_ERR_ARG, "verify: null verifier params");
  std::memcpy(&out->g1, vp->g1, sizeof(G1Affine));
  std::memcpy(&out->g2, vp->g2, sizeof(G2Affine));
  std::memcpy(&out->s_g2, vp->s_g2, sizeof(G2Affine));
  const G1Affine& g = out->g1;
  if (!fq_below_m(g.x) || !fq_below_m(g.y) || g.is_identity() || sqr(g.y) != sqr(g.x) * g.x + from_u64<FqParams>(3))
    return fail(H2G_ERR_ARG, "verify: g1 is not a point of the curve");
  if (!g2_valid(out->g2) || !g2_valid(out->s_g2) || out->g2.is_identity() || out->s_g2.is_identity())
    return fail(H2G_ERR_ARG, "verify: invalid G2 point in the verifier params");
  return H2G_OK;
}

// e(l, s_g2) == e(r, g2)  (DualMSM::check)
bool dual_check(const VerifierPoints& vp, const G1Affine& l, const G1Affine& r) {
  std::vector<PairingPair> pairs(2);
  pairs[0] = {l, vp.s_g2};
  pairs[1] = {affine_neg(r), vp.g2};
  return pairing_check(pairs);
}

// The device pairing's tables for these params: built on the host and uploaded when (g2, s_g2)
// differ from the last call's.  The device state owns them (runtime.h Device::pair_tab).
int pairing_tables(Device* d, const VerifierPoints& vp, const PairingTable** out) {
  uint64_t key[32];
  std::memcpy(key, &vp.g2, sizeof(G2Affine));
  std::memcpy(key + 16, &vp.s_g2, sizeof(G2Affine));
  if (!d->pair_valid || std::memcmp(key, d->pair_key, sizeof(key)) != 0) {
    auto tab = std::make_unique<PairingTable>();
    if (!pairing_table_build(vp.g2, vp.s_g2, tab.get()))
      return fail(H2G_ERR_ARG, "pairing: a G2 point of the verifier params is outside the r-torsion");
    d->pair_valid = false;
    HIPCHK(d->pair_tab.ensure(sizeof(PairingTable)));
    HIPCHK(hipDeviceSynchronize());  // a launch on a caller's stream may still read the old table
    HIPCHK(hipMemcpy(d->pair_tab.p, tab.get(), sizeof(PairingTable), hipMemcpyHostToDevice));
    std::memcpy(d->pair_key, key, sizeof(key));
    d->pair_valid = true;
  }
  *out = d->pair_tab.as<const PairingTable>();
  return H2G_OK;
}

// h2g_pairing_check_batch and h2g_debug_pairing_values: validate, copy in, one launch, copy out
int pairing_host_impl(Device* d, const h2g_verifier_params* vpp, const uint64_t* lr, size_t count, int32_t* ok,
                      uint64_t* miller, uint64_t* gt) {
  VerifierPoints vp;
  RCCHK(load_vp(vpp, &vp));
  if (count == 0) return H2G_OK;
  if (!lr) return fail(H2G_ERR_ARG, "pairing_check: null argument");
  if (count > (1u << 24)) return fail(H2G_ERR_ARG, "pairing_check: too many checks");
  const Fq three = from_u64<FqParams>(3);
  for (size_t i = 0; i < 2 * count; i++) {
    G1Affine c;
    std::memcpy(&c, lr + 8 * i, sizeof(G1Affine));
    if (!fq_below_m(c.x) || !fq_below_m(c.y) || (!c.is_identity() && sqr(c.y) != sqr(c.x) * c.x + three))
      return fail(H2G_ERR_ARG, std::string("pairing_check: the ") + (i & 1 ? "right" : "left") + " point of check " +
                                   std::to_string(i / 2) + " is not a point of the curve");
  }
  const PairingTable* tab = nullptr;
  RCCHK(pairing_tables(d, vp, &tab));
  hipStream_t st = d->stream;
  DevMem d_lr, d_ok, d_ml, d_gt;
  StreamSyncGuard guard{st};
  HIPCHK(hipMalloc(&d_lr.p, 2 * count * sizeof(G1Affine)));
  HIPCHK(hipMalloc(&d_ok.p, count * 4));
  if (miller) HIPCHK(hipMalloc(&d_ml.p, count * 6 * sizeof(Fq2)));
  if (gt) HIPCHK(hipMalloc(&d_gt.p, count * 6 * sizeof(Fq2)));
  std::vector<int32_t> okv(count);
  HIPCHK(hipMemcpyAsync(d_lr.p, lr, 2 * count * sizeof(G1Affine), hipMemcpyHostToDevice, st));
  HIPCHK(pairing_check_launch(tab, (const G1Affine*)d_lr.p, count, (int32_t*)d_ok.p, (Fq2*)d_ml.p, (Fq2*)d_gt.p, st));
  HIPCHK(hipMemcpyAsync(okv.data(), d_ok.p, count * 4, hipMemcpyDeviceToHost, st));
  if (miller) HIPCHK(hipMemcpyAsync(miller, d_ml.p, count * 6 * sizeof(Fq2), hipMemcpyDeviceToHost, st));
  if (gt) HIPCHK(hipMemcpyAsync(gt, d_gt.p, count * 6 * sizeof(Fq2), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (ok) std::memcpy(ok, okv.data(), count * 4);
  return H2G_OK;
}

int verify_impl(Device* d, uint64_t vk_h, const h2g_verifier_params* vpp, int multiopen, int transcript,
                const h2g_verify_item* items, size_t count, const h2g_rng* rng, bool combine, int32_t* verdicts,
                uint64_t stats[4]) {
  VerifyingKey* it = find_vk(vk_h);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown verifying key");
  if (multiopen != MULTIOPEN_SHPLONK && multiopen != MULTIOPEN_GWC)
    return fail(H2G_ERR_ARG, "verify: multiopen must be 0 (SHPLONK) or 1 (GWC)");
  if (transcript != TRANSCRIPT_BLAKE2B && transcript != TRANSCRIPT_KECCAK256)
    return fail(H2G_ERR_ARG, "verify: transcript must be 0 (Blake2b) or 1 (Keccak256)");
  if (!verdicts || (count && !items)) return fail(H2G_ERR_ARG, "verify: null argument");
  // an installed shard or SPMD transport takes no part: nothing here goes through commit()
  VerifierPoints vp;
  RCCHK(load_vp(vpp, &vp));
  const VerifyingKey& vk = *it;
  hipStream_t st = d->stream;
  double t_host = 0, t_dec = 0, t_msm = 0, t_pair = 0;
  uint64_t n_checks = 0, n_terms = 0, n_points = 0;
  double t0 = now_ms();

  // 1. layouts: a proof of the wrong length is malformed here
  std::map<uint32_t, Shape> shapes;  // by circuit count
  std::vector<const Shape*> shape_of(count, nullptr);
  std::vector<size_t> pt_off(count, 0);
  size_t total_pts = 0;
  for (size_t i = 0; i < count; i++) {
    verdicts[i] = H2G_VERIFY_MALFORMED;
    const h2g_verify_item& item = items[i];
    if (!item.proof || item.num_circuits < 1 || item.num_circuits > (1u << 16)) continue;
    auto sit = shapes.find(item.num_circuits);
    if (sit == shapes.end()) {
      Shape s;
      RCCHK(shape_init(s, vk, (int)item.num_circuits, multiopen, transcript));
      sit = shapes.emplace(item.num_circuits, std::move(s)).first;
    }
    if (item.proof_len != sit->second.proof_len()) continue;
    shape_of[i] = &sit->second;
    pt_off[i] = total_pts;
    total_pts += sit->second.pts();
  }
  const uint32_t key_bases = 1 + (uint32_t)vk.fixed.size() + (uint32_t)vk.perm.size();
  if ((uint64_t)key_bases + total_pts >= (1ull << 32)) return fail(H2G_ERR_ARG, "verify: too many points in one batch");

  // 2. every encoding of every proof, one decompression launch; the points stay on the device
  // behind g1 and the key's commitments
  std::vector<uint8_t> enc(32 * total_pts);
  for (size_t i = 0; i < count; i++) {
    const Shape* s = shape_of[i];
    if (!s) continue;
    uint8_t* dst = enc.data() + 32 * pt_off[i];
    std::memcpy(dst, items[i].proof, 32 * s->head_pts);
    std::memcpy(dst + 32 * s->head_pts, items[i].proof + 32 * (s->head_pts + s->scalars), 32 * s->tail_pts);
  }
  std::vector<G1Affine> key_pts;
  key_pts.push_back(vp.g1);
  key_pts.insert(key_pts.end(), vk.fixed.begin(), vk.fixed.end());
  key_pts.insert(key_pts.end(), vk.perm.begin(), vk.perm.end());
  const size_t nbases = key_bases + total_pts;
  std::vector<G1Affine> pts(total_pts);
  DevMem d_bases, d_enc, d_bad;
  t_host += now_ms() - t0;
  t0 = now_ms();
  HIPCHK(hipMalloc(&d_bases.p, nbases * sizeof(G1Affine)));
  HIPCHK(hipMemcpyAsync(d_bases.p, key_pts.data(), key_bases * sizeof(G1Affine), hipMemcpyHostToDevice, st));
  StreamSyncGuard guard{st};
  if (total_pts) {
    HIPCHK(hipMalloc(&d_enc.p, enc.size()));
    HIPCHK(hipMalloc(&d_bad.p, 4));
    HIPCHK(hipMemsetAsync(d_bad.p, 0, 4, st));
    HIPCHK(hipMemcpyAsync(d_enc.p, enc.data(), enc.size(), hipMemcpyHostToDevice, st));
    G1Affine* tail = (G1Affine*)d_bases.p + key_bases;
    HIPCHK(g1_decompress((const uint8_t*)d_enc.p, total_pts, tail, (uint32_t*)d_bad.p, st));
    HIPCHK(hipMemcpyAsync(pts.data(), tail, total_pts * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  n_points = total_pts;
  t_dec += now_ms() - t0;
  t0 = now_ms();

  // 3. per proof: transcript, challenges, expressions, queries, multi-open scalars
  std::vector<size_t> well;  // the well-formed proofs, in order
  std::vector<Fr> scalars;
  std::vector<uint32_t> index, seg_off(1, 0);
  for (size_t i = 0; i < count; i++) {
    const Shape* s = shape_of[i];
    if (!s) continue;
    Msm left, right;
    if (!proof_terms(*s, items[i], pts.data() + pt_off[i], key_bases + (uint32_t)pt_off[i], &left, &right)) continue;
    well.push_back(i);
    for (const Msm* m : {&left, &right}) {
      for (const auto& t : *m) {
        index.push_back(t.base);
        scalars.push_back(t.s);
      }
      seg_off.push_back((uint32_t)index.size());
    }
  }
  n_terms = index.size();
  const size_t W = well.size();
  t_host += now_ms() - t0;
  if (W == 0) {
    if (stats) stats[0] = 0, stats[1] = 0, stats[2] = n_points, stats[3] = (uint64_t)(t_host + 0.5);
    g_verify_ms[0] = t_host, g_verify_ms[1] = t_dec, g_verify_ms[2] = 0, g_verify_ms[3] = 0;
    return H2G_OK;
  }
  for (uint32_t b : index)
    if (b >= nbases) return fail(H2G_ERR_STATE, "verify: internal base index out of range");

  // 4. one segmented MSM: (L_i, R_i) per well-formed proof
  t0 = now_ms();
  DevMem d_sc, d_ix, d_off, d_lr, d_comb;
  HIPCHK(hipMalloc(&d_sc.p, std::max<size_t>(scalars.size(), 2 * W) * sizeof(Fr)));
  HIPCHK(hipMalloc(&d_ix.p, std::max<size_t>(index.size(), 2 * W) * 4));
  HIPCHK(hipMalloc(&d_off.p, seg_off.size() * 4));
  HIPCHK(hipMalloc(&d_lr.p, 2 * W * sizeof(G1Affine)));
  HIPCHK(hipMalloc(&d_comb.p, 2 * sizeof(G1Affine)));
  HIPCHK(hipMemcpyAsync(d_sc.p, scalars.data(), scalars.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ix.p, index.data(), index.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_off.p, seg_off.data(), seg_off.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(msm_segmented((const G1Affine*)d_bases.p, nbases, (const Fr*)d_sc.p, (const uint32_t*)d_ix.p,
                       (const uint32_t*)d_off.p, 2 * W, (G1Affine*)d_lr.p, st));
  HIPCHK(hipStreamSynchronize(st));
  t_msm += now_ms() - t0;

  if (!combine) {  // SingleStrategy: each proof its own check, no random factor
    std::vector<G1Affine> lr(2 * W);
    HIPCHK(hipMemcpy(lr.data(), d_lr.p, lr.size() * sizeof(G1Affine), hipMemcpyDeviceToHost));
    t0 = now_ms();
    for (size_t j = 0; j < W; j++) {
      verdicts[well[j]] = dual_check(vp, lr[2 * j], lr[2 * j + 1]) ? H2G_VERIFY_OK : H2G_VERIFY_REJECTED;
      n_checks++;
    }
    t_pair += now_ms() - t0;
  } else {
    // 5. one nonzero r_i per proof
    t0 = now_ms();
    std::vector<Fr> r(W);
    for (auto& v : r)
      if (!draw_nonzero(rng, &v)) return fail(H2G_ERR_STATE, "verify_batch: the random source failed");
    t_host += now_ms() - t0;
    // 6. e(sum r_i L_i, s_g2) == e(sum r_i R_i, g2) over a set of proofs: two segments of the
    // same kernel over the (L_i, R_i) array
    int rc = H2G_OK;
    auto test = [&](size_t lo, size_t hi) -> bool {
      const size_t m = hi - lo;
      std::vector<Fr> sc(2 * m);
      std::vector<uint32_t> ix(2 * m);
      for (size_t j = 0; j < m; j++) {
        sc[j] = sc[m + j] = r[lo + j];
        ix[j] = (uint32_t)(2 * (lo + j));
        ix[m + j] = (uint32_t)(2 * (lo + j) + 1);
      }
      const uint32_t off[3] = {0, (uint32_t)m, (uint32_t)(2 * m)};
      G1Affine comb[2];
      double ta = now_ms();
      hipError_t e = hipMemcpyAsync(d_sc.p, sc.data(), sc.size() * sizeof(Fr), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(d_ix.p, ix.data(), ix.size() * 4, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, off, sizeof(off), hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = msm_segmented((const G1Affine*)d_lr.p, 2 * W, (const Fr*)d_sc.p, (const uint32_t*)d_ix.p,
                          (const uint32_t*)d_off.p, 2, (G1Affine*)d_comb.p, st);
      if (e == hipSuccess) e = hipMemcpyAsync(comb, d_comb.p, sizeof(comb), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      t_msm += now_ms() - ta;
      if (e != hipSuccess) {
        rc = hip_fail(e, "verify_batch: combination MSM");
        return false;
      }
      ta = now_ms();
      const bool ok = dual_check(vp, comb[0], comb[1]);
      t_pair += now_ms() - ta;
      n_checks++;
      return ok;
    };
    auto mark = [&](size_t lo, size_t hi, int32_t v) {
      for (size_t j = lo; j < hi; j++) verdicts[well[j]] = v;
    };
    // a failing set is halved; when its first half holds, the second is known to fail and is
    // halved without a check of its own
    std::function<void(size_t, size_t)> resolve = [&](size_t lo, size_t hi) {
      if (rc) return;
      if (hi - lo == 1) return mark(lo, hi, H2G_VERIFY_REJECTED);
      const size_t mid = lo + (hi - lo + 1) / 2;
      if (test(lo, mid)) {
        mark(lo, mid, H2G_VERIFY_OK);
        return resolve(mid, hi);
      }
      if (rc) return;
      resolve(lo, mid);
      if (rc) return;
      if (test(mid, hi)) mark(mid, hi, H2G_VERIFY_OK);
      else if (!rc) resolve(mid, hi);
    };
    if (test(0, W)) {
      mark(0, W, H2G_VERIFY_OK);
    } else if (!rc && g_isolation == 1) {
      // one launch over the resident (L_i, R_i): each proof's own check, no random factor
      const double ta = now_ms();
      const PairingTable* tab = nullptr;
      RCCHK(pairing_tables(d, vp, &tab));
      DevMem d_ok;
      std::vector<int32_t> okv(W);
      HIPCHK(hipMalloc(&d_ok.p, W * 4));
      HIPCHK(pairing_check_launch(tab, (const G1Affine*)d_lr.p, W, (int32_t*)d_ok.p, nullptr, nullptr, st));
      HIPCHK(hipMemcpyAsync(okv.data(), d_ok.p, W * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (size_t j = 0; j < W; j++) verdicts[well[j]] = okv[j] ? H2G_VERIFY_OK : H2G_VERIFY_REJECTED;
      t_pair += now_ms() - ta;
      n_checks += W;
    } else if (!rc) {
      resolve(0, W);
    }
    if (rc) return rc;
  }
  if (stats) {
    stats[0] = n_checks;
    stats[1] = n_terms;
    stats[2] = n_points;
    stats[3] = (uint64_t)(t_host + t_pair + 0.5);
  }
  g_verify_ms[0] = t_host, g_verify_ms[1] = t_dec, g_verify_ms[2] = t_msm, g_verify_ms[3] = t_pair;
  return H2G_OK;
}
}  // namespace

extern "C" {

int h2g_vk_from_pk(uint64_t pk_h, uint64_t* vk) {
  NEED_DEV_P();
  if (!vk) return fail(H2G_ERR_ARG, "vk_from_pk: null argument");
  ProvingKey* it = find_pk(pk_h);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  RCCHK(h2g_pk_vk_commitments(pk_h, nullptr, nullptr));  // commit_lagrange, once per key
  auto key = std::make_unique<VerifyingKey>();
  key->cs = it->cs;
  key->fixed = it->vk_fixed;
  key->perm = it->vk_perm;
  *vk = g_next_handle++;
  g_vks[*vk] = std::move(key);
  return H2G_OK;
}

int h2g_vk_free(uint64_t vk) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!g_vks.erase(vk)) return fail(H2G_ERR_HANDLE, "unknown verifying key");
  return H2G_OK;
}

int h2g_params_verifier(uint64_t params, h2g_verifier_params* out) {
  NEED_DEV_P();
  Params* it = find_params(params);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown params");
  if (!out) return fail(H2G_ERR_ARG, "params_verifier: null argument");
  const Params& p = *it;
  if (!p.has_g2) return fail(H2G_ERR_STATE, "params_verifier: the params have no G2 points (h2g_params_set_g2)");
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(out->g1, p.g, sizeof(G1Affine), hipMemcpyDeviceToHost));
  std::memcpy(out->g2, &p.g2, sizeof(G2Affine));
  std::memcpy(out->s_g2, &p.s_g2, sizeof(G2Affine));
  return H2G_OK;
}

int h2g_verify_proof(uint64_t vk, const h2g_verifier_params* vp, int multiopen, int transcript,
                     const h2g_verify_item* item, int32_t* verdict) {
  NEED_DEV_P();
  if (!item || !verdict) return fail(H2G_ERR_ARG, "verify_proof: null argument");
  return verify_impl(d, vk, vp, multiopen, transcript, item, 1, nullptr, false, verdict, nullptr);
}

int h2g_verify_batch(uint64_t vk, const h2g_verifier_params* vp, int multiopen, int transcript,
                     const h2g_verify_item* items, size_t count, const h2g_rng* rng, int32_t* verdicts,
                     uint64_t stats[4]) {
  NEED_DEV_P();
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (count == 0) return H2G_OK;
  return verify_impl(d, vk, vp, multiopen, transcript, items, count, rng, true, verdicts, stats);
}

// Verifier::verify_proof (poly/commitment.rs:171-193) on its own: the caller's commitments and
// queries, the argument's points read from a read-mode transcript object (decoded on the
// host, a handful), the scalars of multiopen.cpp, one segmented MSM for (left, right).
int h2g_multiopen_verify(const h2g_verifier_params* vpp, int scheme, uint64_t transcript, const uint64_t* commitments,
                         size_t ncommitments, const h2g_verify_query* queries, size_t nqueries, int32_t* verdict,
                         uint64_t lr[16]) {
  NEED_DEV_P();
  if (!verdict) return fail(H2G_ERR_ARG, "multiopen_verify: null argument");
  *verdict = H2G_VERIFY_MALFORMED;
  TranscriptObj* ti = find_transcript(transcript);
  if (!ti) return fail(H2G_ERR_HANDLE, "unknown transcript");
  TranscriptObj& T = *ti;
  if (scheme != MULTIOPEN_SHPLONK && scheme != MULTIOPEN_GWC)
    return fail(H2G_ERR_ARG, "multiopen_verify: scheme must be 0 (SHPLONK) or 1 (GWC)");
  if (!T.read) return fail(H2G_ERR_ARG, "multiopen_verify: a write-mode transcript");
  if (!commitments || !queries || ncommitments == 0 || nqueries == 0)
    return fail(H2G_ERR_ARG, "multiopen_verify: no commitments or no queries");
  if (ncommitments > (1u << 24) || nqueries > (1u << 24)) return fail(H2G_ERR_ARG, "multiopen_verify: too many queries");
  VerifierPoints vp;
  RCCHK(load_vp(vpp, &vp));
  std::vector<G1Affine> bases(1 + ncommitments);
  bases[BASE_G1] = vp.g1;
  for (size_t i = 0; i < ncommitments; i++) {
    G1Affine& c = bases[1 + i];
    std::memcpy(&c, commitments + 8 * i, sizeof(G1Affine));
    if (!fq_below_m(c.x) || !fq_below_m(c.y) ||
        (!c.is_identity() && sqr(c.y) != sqr(c.x) * c.x + from_u64<FqParams>(3)))
      return fail(H2G_ERR_ARG, "multiopen_verify: commitment " + std::to_string(i) + " is not a point of the curve");
  }
  MultiopenVerifyIo io;
  std::vector<VerifierQ> qs(nqueries);
  for (size_t i = 0; i < nqueries; i++) {
    const h2g_verify_query& q = queries[i];
    if (q.commitment >= ncommitments)
      return fail(H2G_ERR_ARG, "multiopen_verify: query " + std::to_string(i) + " names an unknown commitment");
    const Fr pt = fr_from_limbs(q.point), ev = fr_from_limbs(q.eval);
    if (!fr_below(pt) || !fr_below(ev))
      return fail(H2G_ERR_ARG, "multiopen_verify: query " + std::to_string(i) + ": value not below r");
    size_t p = 0;
    while (p < io.point.size() && !(io.point[p] == pt)) p++;
    if (p == io.point.size()) io.point.push_back(pt);
    qs[i] = {1 + q.commitment, (int)p, ev};
  }
  bool ok = true;
  io.T = &T.tr;
  io.read_point = [&]() -> uint32_t {
    G1Affine p;
    if (!ok || !T.read_point(&p)) return ok = false, 0;
    bases.push_back(p);
    return (uint32_t)bases.size() - 1;
  };
  io.ok = [&ok] { return ok; };
  io.add_obj = [](Msm& m, uint32_t key, const Fr& f) { m.push_back({key, f}); };
  Msm left, right;
  if (!multiopen_verify_terms(scheme, qs, io, &left, &right)) return H2G_OK;  // MALFORMED
  msm_merge(left);
  msm_merge(right);
  std::vector<Fr> scalars;
  std::vector<uint32_t> index, seg_off(1, 0);
  for (const Msm* m : {&left, &right}) {
    for (const auto& t : *m) {
      index.push_back(t.base);
      scalars.push_back(t.s);
    }
    seg_off.push_back((uint32_t)index.size());
  }
  hipStream_t st = d->stream;
  DevMem d_bases, d_sc, d_ix, d_off, d_lr;
  StreamSyncGuard guard{st};
  HIPCHK(hipMalloc(&d_bases.p, bases.size() * sizeof(G1Affine)));
  HIPCHK(hipMalloc(&d_sc.p, scalars.size() * sizeof(Fr)));
  HIPCHK(hipMalloc(&d_ix.p, index.size() * 4));
  HIPCHK(hipMalloc(&d_off.p, seg_off.size() * 4));
  HIPCHK(hipMalloc(&d_lr.p, 2 * sizeof(G1Affine)));
  HIPCHK(hipMemcpyAsync(d_bases.p, bases.data(), bases.size() * sizeof(G1Affine), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_sc.p, scalars.data(), scalars.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ix.p, index.data(), index.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_off.p, seg_off.data(), seg_off.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(msm_segmented((const G1Affine*)d_bases.p, bases.size(), (const Fr*)d_sc.p, (const uint32_t*)d_ix.p,
                       (const uint32_t*)d_off.p, 2, (G1Affine*)d_lr.p, st));
  G1Affine out[2];
  HIPCHK(hipMemcpyAsync(out, d_lr.p, sizeof(out), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (lr) std::memcpy(lr, out, sizeof(out));
  *verdict = dual_check(vp, out[0], out[1]) ? H2G_VERIFY_OK : H2G_VERIFY_REJECTED;
  return H2G_OK;
}

int h2g_pairing_check_batch(const h2g_verifier_params* vp, const uint64_t* lr, size_t count, int32_t* ok) {
  NEED_DEV_P();
  if (count && !ok) return fail(H2G_ERR_ARG, "pairing_check: null argument");
  return pairing_host_impl(d, vp, lr, count, ok, nullptr, nullptr);
}

int h2g_pairing_check_batch_dev(const h2g_verifier_params* vpp, const void* d_lr, size_t count, void* d_ok,
                                void* stream) {
  NEED_DEV_P();
  VerifierPoints vp;
  RCCHK(load_vp(vpp, &vp));
  if (count == 0) return H2G_OK;
  if (!d_lr || !d_ok) return fail(H2G_ERR_ARG, "pairing_check_dev: null argument");
  if (((uintptr_t)d_lr | (uintptr_t)d_ok) & 15) return fail(H2G_ERR_ARG, "pairing_check_dev: misaligned pointer");
  if (count > (1u << 24)) return fail(H2G_ERR_ARG, "pairing_check_dev: too many checks");
  const PairingTable* tab = nullptr;
  RCCHK(pairing_tables(d, vp, &tab));
  HIPCHK(pairing_check_launch(tab, (const G1Affine*)d_lr, count, (int32_t*)d_ok, nullptr, nullptr,
                              pick_stream(d, stream)));
  return H2G_OK;
}

int h2g_verify_set_isolation(int mode) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (mode != 0 && mode != 1) return fail(H2G_ERR_ARG, "verify_set_isolation: mode must be 0 (bisection) or 1 (device checks)");
  g_isolation = mode;
  return H2G_OK;
}

int h2g_debug_pairing_values(const h2g_verifier_params* vp, const uint64_t* lr, size_t count, uint64_t* miller,
                             uint64_t* gt) {
  NEED_DEV_P();
  return pairing_host_impl(d, vp, lr, count, nullptr, miller, gt);
}

/* wall milliseconds of the last h2g_verify_proof / h2g_verify_batch: [0] host (transcripts,
 * scalar assembly, the r_i), [1] decompression (upload, kernel, copy back), [2] the segmented
 * MSMs (uploads, kernels, results), [3] pairing checks */
int h2g_verify_stages(double ms[4]) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!ms) return fail(H2G_ERR_ARG, "verify_stages: null argument");
  for (int i = 0; i < 4; i++) ms[i] = g_verify_ms[i];
  return H2G_OK;
}

}  // extern "C"
