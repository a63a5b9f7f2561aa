// pk_serde.cpp -- reading and writing params and proving keys in the three SerdeFormats.
#include "prover_state.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

// ------------------------------------------------------------------ serialisation
// SerdeFormat (halo2_backend/src/helpers.rs:8-21): 0 Processed, 1 RawBytes,
// 2 RawBytesUnchecked.  RawBytes writes points uncompressed and field elements as their
// Montgomery limbs -- the device layout, so arrays move with one copy -- and on read
// checks that every element is below its modulus and every point is on its curve (on
// the device for the n-sized arrays).  Processed (compressed points, canonical field
// elements) is refused: halo2curves' compressed-point flag bits cannot be pinned here.

namespace {
enum { SERDE_PROCESSED = 0, SERDE_RAW = 1, SERDE_RAW_UNCHECKED = 2 };
constexpr uint8_t PK_VERSION = 0x04;  // plonk.rs:58

struct DevScratch {
  void* p = nullptr;
  ~DevScratch() {
    if (p) (void)hipFree(p);
  }
};
// GroupEncoding::to_bytes / from_bytes of one G1 point on the host (the VK's commitments);
// the device form for whole arrays is g1_compress / g1_decompress (serde.hip)
void g1_compress_host(const G1Affine& a, uint8_t c[32]) {
  Fq x = Fq::zero();
  if (!a.is_identity()) {
    x = to_canonical(a.x);
    x.l[7] |= (to_canonical(a.y).l[0] & 1u) << 31;
  }
  std::memcpy(c, x.l, 32);
}
bool g1_decompress_host(const uint8_t c[32], G1Affine* out) {
  static constexpr uint32_t SQRT_EXP[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u,
                                           0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};  // (p+1)/4
  Fq x;
  std::memcpy(x.l, c, 32);
  const uint32_t ysign = x.l[7] >> 31;
  x.l[7] &= 0x7fffffffu;
  unsigned br = 0;
  for (int i = 0; i < 8; i++) (void)__builtin_subc(x.l[i], FqParams::M[i], br, &br);
  if (!br) return false;  // x >= p
  out->x = out->y = Fq::zero();
  if (x.is_zero() && !ysign) return true;  // identity
  const Fq xm = from_canonical(x);
  const Fq y2 = sqr(xm) * xm + from_u64<FqParams>(3);
  Fq y = pow_limbs(y2, SQRT_EXP);
  if (sqr(y) != y2) return false;
  if ((to_canonical(y).l[0] & 1u) != ysign) y = neg(y);
  out->x = xm;
  out->y = y;
  return true;
}

struct ByteWriter {  // out == NULL: count only
  uint8_t* out;
  size_t cap;
  // the library stream the arrays were produced on: copies and conversions queue behind
  // its work (it is non-blocking, so the NULL stream would not order with it)
  hipStream_t st;
  size_t len = 0;
  bool fits(size_t k) const { return out && len + k <= cap; }
  void put(const void* p, size_t k) {
    if (fits(k)) std::memcpy(out + len, p, k);
    len += k;
  }
  void u8(uint8_t v) { put(&v, 1); }
  void u32le(uint32_t v) { put(&v, 4); }
  void u32be(uint32_t v) {
    const uint8_t b[4] = {(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v};
    put(b, 4);
  }
  bool proc = false;  // SerdeFormat::Processed: compressed points, canonical field elements
  int dev(const void* d, size_t k) {  // device bytes
    if (fits(k)) {
      HIPCHK(hipMemcpyAsync(out + len, d, k, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    len += k;
    return H2G_OK;
  }
  // `cnt` elements converted on the device into a scratch array of `k` bytes, then copied
  template <class Conv>
  int dev_conv(size_t k, Conv conv) {
    if (fits(k)) {
      DevScratch t;
      HIPCHK(hipMalloc(&t.p, k));
      HIPCHK(conv(t.p));
      HIPCHK(hipMemcpyAsync(out + len, t.p, k, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    len += k;
    return H2G_OK;
  }
  int g1s(const G1Affine* d, size_t cnt) {  // SerdeCurveAffine::write of cnt device points
    if (!proc) return dev(d, cnt * sizeof(G1Affine));
    return dev_conv(cnt * 32, [&](void* t) { return g1_compress(d, cnt, (uint8_t*)t, st); });
  }
  void g1(const G1Affine& a) {
    if (!proc) return put(&a, sizeof(G1Affine));
    uint8_t c[32];
    g1_compress_host(a, c);
    put(c, 32);
  }
  void g2(const G2Affine& a) {
    if (!proc) return put(&a, sizeof(G2Affine));
    uint8_t c[64];
    g2_compress(a, c);
    put(c, 64);
  }
  int poly(const Fr* d, size_t cnt) {  // Polynomial::write (poly.rs:187-197)
    u32be((uint32_t)cnt);
    if (!proc) return dev(d, cnt * sizeof(Fr));
    return dev_conv(cnt * sizeof(Fr), [&](void* t) { return fr_to_repr(d, cnt, (Fr*)t, st); });
  }
  int polys(const std::vector<Fr*>& v, size_t cnt) {  // write_polynomial_slice (helpers.rs:119-129)
    u32be((uint32_t)v.size());
    for (const Fr* p : v) RCCHK(poly(p, cnt));
    return H2G_OK;
  }
};

struct ByteReader {
  const uint8_t* p;
  size_t len, pos = 0;
  bool ok = true;
  const uint8_t* take(size_t k) {
    if (!ok || pos + k > len) {
      ok = false;
      return nullptr;
    }
    const uint8_t* r = p + pos;
    pos += k;
    return r;
  }
  uint8_t u8() {
    const uint8_t* b = take(1);
    return b ? b[0] : 0;
  }
  uint32_t u32le() {
    const uint8_t* b = take(4);
    return b ? (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24 : 0;
  }
  uint32_t u32be() {
    const uint8_t* b = take(4);
    return b ? (uint32_t)b[3] | (uint32_t)b[2] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[0] << 24 : 0;
  }
  // one polynomial of exactly `cnt` elements (read_polynomial_vec / Polynomial::read)
  const uint8_t* poly(size_t cnt) {
    if (u32be() != cnt) ok = false;
    return take(cnt * sizeof(Fr));
  }
  bool polys(std::vector<const uint8_t*>& v, size_t count, size_t cnt) {
    if (u32be() != count) return ok = false;
    v.resize(count);
    for (auto& q : v) q = poly(cnt);
    return ok;
  }
};

bool fq_below(const Fq& a) {
  unsigned br = 0;
  for (int i = 0; i < 8; i++) (void)__builtin_subc(a.l[i], FqParams::M[i], br, &br);
  return br != 0;
}
}  // namespace

namespace h2g {
namespace prv {
bool g2_valid(const G2Affine& a) {
  return fq_below(a.x.c0) && fq_below(a.x.c1) && fq_below(a.y.c0) && fq_below(a.y.c1) && g2_on_curve(a);
}
bool g1_from_bytes_host(const uint8_t c[32], G1Affine* out) { return g1_decompress_host(c, out); }
}  // namespace prv
}  // namespace h2g

namespace {
bool g1_valid_host(const G1Affine& a) {
  if (!fq_below(a.x) || !fq_below(a.y)) return false;
  return a.is_identity() || sqr(a.y) == sqr(a.x) * a.x + from_u64<FqParams>(3);
}

// device RawBytes checks of uploaded arrays: number of bad elements
int count_bad_fr(const std::vector<std::pair<const Fr*, size_t>>& arrays, hipStream_t st, uint32_t* bad_out) {
  uint32_t* bad;
  HIPCHK(hipMalloc(&bad, 4));
  HIPCHK(hipMemsetAsync(bad, 0, 4, st));
  for (const auto& a : arrays) HIPCHK(fr_count_unreduced(a.first, a.second, bad, st));
  HIPCHK(hipMemcpyAsync(bad_out, bad, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  (void)hipFree(bad);
  return H2G_OK;
}

// VerifyingKey::write (plonk.rs:73-86): version, k, the fixed column count, the fixed
// commitments, then permutation::VerifyingKey::write -- the head of a written ProvingKey and
// all of a written VerifyingKey (h2g_vk_write)
void vk_write_prefix(ByteWriter& w, uint32_t k, const std::vector<G1Affine>& fixed, const std::vector<G1Affine>& perm) {
  w.u8(PK_VERSION);
  w.u8((uint8_t)k);
  w.u32le((uint32_t)fixed.size());
  for (const auto& c : fixed) w.g1(c);
  for (const auto& c : perm) w.g1(c);
}
// VerifyingKey::read (plonk.rs:88-129) up to the commitments; the constraint system is the caller's
int vk_read_prefix(ByteReader& r, int format, const h2g_circuit* circuit, const char* who, std::vector<G1Affine>* vf,
                   std::vector<G1Affine>* vp) {
  const std::string w = who;
  const bool proc = format == SERDE_PROCESSED;
  if (r.u8() != PK_VERSION) return fail(H2G_ERR_ARG, w + ": unexpected version byte");
  const uint32_t k = r.u8();
  if (!r.ok || k != circuit->k) return fail(H2G_ERR_ARG, w + ": k does not match");
  const uint32_t F = r.u32le();
  if (!r.ok || F != circuit->num_fixed) return fail(H2G_ERR_ARG, w + ": fixed column count does not match");
  vf->assign(F, G1Affine{Fq::zero(), Fq::zero()});
  vp->assign(circuit->num_perm_columns, G1Affine{Fq::zero(), Fq::zero()});
  bool enc_ok = true;
  for (auto* v : {vf, vp})
    for (auto& c : *v) {
      if (proc) {
        if (const uint8_t* b = r.take(32)) enc_ok = g1_decompress_host(b, &c) && enc_ok;
      } else if (const uint8_t* b = r.take(sizeof(G1Affine))) {
        std::memcpy(&c, b, sizeof(G1Affine));
      }
    }
  if (!r.ok) return fail(H2G_ERR_ARG, w + ": truncated verifying key");
  if (!enc_ok) return fail(H2G_ERR_ARG, w + ": invalid point encoding in the verifying key");
  if (format == SERDE_RAW) {
    for (const auto& c : *vf)
      if (!g1_valid_host(c)) return fail(H2G_ERR_ARG, w + ": invalid fixed commitment");
    for (const auto& c : *vp)
      if (!g1_valid_host(c)) return fail(H2G_ERR_ARG, w + ": invalid permutation commitment");
  }
  return H2G_OK;
}
}  // namespace

extern "C" {

/* VerifyingKey::write / read (plonk.rs:73-129): the prefix of h2g_pk_write's bytes */
int h2g_vk_write(uint64_t vk, int format, uint8_t* out, size_t cap, size_t* len) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  VerifyingKey* it = find_vk(vk);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown verifying key");
  if (!len) return fail(H2G_ERR_ARG, "vk_write: null length");
  if (format != SERDE_RAW && format != SERDE_RAW_UNCHECKED && format != SERDE_PROCESSED)
    return fail(H2G_ERR_ARG, "vk_write: unknown SerdeFormat");
  ByteWriter w{out, out ? cap : 0, nullptr};
  w.proc = format == SERDE_PROCESSED;
  vk_write_prefix(w, it->cs.k, it->fixed, it->perm);
  *len = w.len;
  if (out && w.len > cap) return fail(H2G_ERR_ARG, "vk_write: buffer too small");
  return H2G_OK;
}

int h2g_vk_read(const h2g_circuit* circuit, const uint8_t* buf, size_t len, int format, uint64_t* vk) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!circuit || !buf || !vk) return fail(H2G_ERR_ARG, "vk_read: null argument");
  if (format != SERDE_RAW && format != SERDE_RAW_UNCHECKED && format != SERDE_PROCESSED)
    return fail(H2G_ERR_ARG, "vk_read: unknown SerdeFormat");
  auto key = std::make_unique<VerifyingKey>();
  RCCHK(cs_host_build(circuit, &key->cs));
  ByteReader r{buf, len};
  RCCHK(vk_read_prefix(r, format, circuit, "vk_read", &key->fixed, &key->perm));
  if (r.pos != len) return fail(H2G_ERR_ARG, "vk_read: trailing bytes");
  *vk = g_next_handle++;
  g_vks[*vk] = std::move(key);
  return H2G_OK;
}

/* ParamsKZG::write_custom (kzg/commitment.rs:166-181): k (u32 LE), g, g_lagrange, g2, s_g2 */
int h2g_params_write(uint64_t params, int format, uint8_t* out, size_t cap, size_t* len) {
  NEED_DEV_P();
  Params* it = find_params(params);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown params");
  if (!len) return fail(H2G_ERR_ARG, "params_write: null length");
  if (format != SERDE_RAW && format != SERDE_RAW_UNCHECKED && format != SERDE_PROCESSED)
    return fail(H2G_ERR_ARG, "params_write: unknown SerdeFormat");
  const Params& p = *it;
  if (!p.has_g2) return fail(H2G_ERR_STATE, "params_write: the params have no G2 points (h2g_params_set_g2)");
  ByteWriter w{out, out ? cap : 0, d->stream};
  w.proc = format == SERDE_PROCESSED;
  w.u32le(p.k);
  RCCHK(w.g1s(p.g, p.n));
  RCCHK(w.g1s(p.gl, p.n));
  w.g2(p.g2);
  w.g2(p.s_g2);
  *len = w.len;
  if (out && w.len > cap) return fail(H2G_ERR_ARG, "params_write: buffer too small");
  return H2G_OK;
}

/* ParamsKZG::read_custom (kzg/commitment.rs:183-267) */
int h2g_params_read(const uint8_t* buf, size_t len, int format, uint64_t* handle) {
  NEED_DEV_P();
  if (!buf || !handle) return fail(H2G_ERR_ARG, "params_read: null argument");
  if (format != SERDE_RAW && format != SERDE_RAW_UNCHECKED && format != SERDE_PROCESSED)
    return fail(H2G_ERR_ARG, "params_read: unknown SerdeFormat");
  const bool proc = format == SERDE_PROCESSED;
  const size_t g1b = proc ? 32 : sizeof(G1Affine), g2b = proc ? 64 : sizeof(G2Affine);
  ByteReader r{buf, len};
  const uint32_t k = r.u32le();
  if (!r.ok || k > 27) return fail(H2G_ERR_ARG, "params_read: bad k");
  const size_t n = (size_t)1 << k;
  const uint8_t* g = r.take(n * g1b);
  const uint8_t* gl = r.take(n * g1b);
  const uint8_t* g2 = r.take(g2b);
  const uint8_t* sg2 = r.take(g2b);
  if (!r.ok) return fail(H2G_ERR_ARG, "params_read: truncated input");
  hipStream_t st = d->stream;
  auto p = std::make_unique<Params>();
  p->device = d->id;
  p->k = k;
  p->n = n;
  PALLOC(p->pool, p->g, n);
  PALLOC(p->pool, p->gl, n);
  if (proc) {  // load_points_from_file_parallelly (kzg/commitment.rs:195-213), on the device
    DevScratch t, bad;
    uint32_t nbad = 0;
    HIPCHK(hipMalloc(&t.p, 2 * n * 32));
    HIPCHK(hipMalloc(&bad.p, 4));
    HIPCHK(hipMemsetAsync(bad.p, 0, 4, st));
    HIPCHK(hipMemcpyAsync(t.p, g, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync((uint8_t*)t.p + n * 32, gl, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(g1_decompress((const uint8_t*)t.p, n, p->g, (uint32_t*)bad.p, st));
    HIPCHK(g1_decompress((const uint8_t*)t.p + n * 32, n, p->gl, (uint32_t*)bad.p, st));
    HIPCHK(hipMemcpyAsync(&nbad, bad.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nbad) return fail(H2G_ERR_ARG, "params_read: " + std::to_string(nbad) + " invalid point encodings");
    if (!g2_decompress(g2, &p->g2) || !g2_decompress(sg2, &p->s_g2))
      return fail(H2G_ERR_ARG, "params_read: invalid G2 point encoding");
  } else {
    HIPCHK(hipMemcpyAsync(p->g, g, n * sizeof(G1Affine), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(p->gl, gl, n * sizeof(G1Affine), hipMemcpyHostToDevice, st));
    std::memcpy(&p->g2, g2, sizeof(G2Affine));
    std::memcpy(&p->s_g2, sg2, sizeof(G2Affine));
  }
  p->has_g2 = true;
  if (format == SERDE_RAW) {
    uint32_t* bad;
    uint32_t nbad = 0;
    HIPCHK(hipMalloc(&bad, 4));
    HIPCHK(hipMemsetAsync(bad, 0, 4, st));
    HIPCHK(g1_count_invalid(p->g, n, bad, st));
    HIPCHK(g1_count_invalid(p->gl, n, bad, st));
    HIPCHK(hipMemcpyAsync(&nbad, bad, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    (void)hipFree(bad);
    if (nbad) return fail(H2G_ERR_ARG, "params_read: " + std::to_string(nbad) + " G1 points off the curve or unreduced");
    if (!g2_valid(p->g2) || !g2_valid(p->s_g2)) return fail(H2G_ERR_ARG, "params_read: invalid G2 point");
  }
  RCCHK(params_finish(*p, st));
  *handle = g_next_handle++;
  g_params[*handle] = std::move(p);
  return H2G_OK;
}

/* ProvingKey::write (plonk.rs:311-321) with VerifyingKey::write (plonk.rs:73-86) */
int h2g_pk_write(uint64_t pk_h, int format, uint8_t* out, size_t cap, size_t* len) {
  NEED_DEV_P();
  ProvingKey* it = find_pk(pk_h);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown proving key");
  if (!len) return fail(H2G_ERR_ARG, "pk_write: null length");
  if (format != SERDE_RAW && format != SERDE_RAW_UNCHECKED && format != SERDE_PROCESSED)
    return fail(H2G_ERR_ARG, "pk_write: unknown SerdeFormat");
  ProvingKey& pk = *it;
  Params* pit = find_params(pk.params);
  if (!pit) return fail(H2G_ERR_HANDLE, "pk_write: the key's params were freed");
  RCCHK(h2g_pk_vk_commitments(pk_h, nullptr, nullptr));  // commit_lagrange, once
  HIPCHK(hipStreamSynchronize(d->stream));
  ByteWriter w{out, out ? cap : 0, d->stream};
  w.proc = format == SERDE_PROCESSED;
  vk_write_prefix(w, pk.cs.k, pk.vk_fixed, pk.vk_perm);
  // The format holds the extended cosets.  A streamed key has none: each is produced from
  // its polynomial in the h(X) buffer (free between proofs) and written from there, one at a
  // time -- the same field elements a resident key holds, so the same bytes.
  auto coset = [&](const Fr* resident, const Fr* coeffs) -> int {
    if (!pk.cosets) return w.poly(resident, pk.ext);
    if (w.out) RCCHK(coeff_to_extended(d, pk.dom, coeffs, pk.h_ext, d->stream));
    return w.poly(pk.h_ext, pk.ext);
  };
  auto cosets = [&](const std::vector<Fr*>& resident, const std::vector<Fr*>& coeffs) -> int {
    w.u32be((uint32_t)resident.size());
    for (size_t i = 0; i < resident.size(); i++) RCCHK(coset(resident[i], coeffs[i]));
    return H2G_OK;
  };
  RCCHK(coset(pk.l0, pk.l0_poly));
  RCCHK(coset(pk.l_last, pk.l_last_poly));
  if (pk.cosets && w.out) {  // l_active = -((l_last + l_blind) - 1), in coefficient form (pk.mod)
    const Fr one = Fr::one();
    HIPCHK(poly_binop(POLY_ADD, pk.l_last_poly, pk.l_blind_poly, one, pk.mod, pk.n, d->stream));
    HIPCHK(poly_binop(POLY_SUB_CONST, pk.mod, nullptr, one, pk.mod, 1, d->stream));
    HIPCHK(poly_binop(POLY_SCALE, pk.mod, nullptr, fr_neg_one(), pk.mod, pk.n, d->stream));
  }
  RCCHK(coset(pk.l_active, pk.mod));
  RCCHK(w.polys(pk.fixed_lag, pk.n));
  RCCHK(w.polys(pk.fixed_poly, pk.n));
  RCCHK(cosets(pk.fixed_coset, pk.fixed_poly));
  RCCHK(w.polys(pk.sigma_lag, pk.n));  // permutation::ProvingKey::write (permutation.rs:82-91)
  RCCHK(w.polys(pk.sigma_poly, pk.n));
  RCCHK(cosets(pk.sigma_coset, pk.sigma_poly));
  *len = w.len;
  if (out && w.len > cap) return fail(H2G_ERR_ARG, "pk_write: buffer too small");
  return H2G_OK;
}

/* ProvingKey::read (plonk.rs:334-359): like the reference, the circuit (its constraint
 * system) comes from the caller; the key's arrays and commitments come from the bytes
 * (circuit->fixed_values and ->copies are not used and may be NULL). */
int h2g_pk_read(uint64_t params, const h2g_circuit* circuit, const uint8_t* buf, size_t len, int format,
                uint64_t* pk_out) {
  return h2g_pk_read_opts(params, circuit, buf, len, format, nullptr, pk_out);
}

/* The same with key options.  A streamed key takes the file's polynomials, runs every check
 * of the resident read on the file's cosets (in scratch, array by array) and drops them:
 * its proofs derive the sub-cosets from the polynomials. */
int h2g_pk_read_opts(uint64_t params, const h2g_circuit* circuit, const uint8_t* buf, size_t len, int format,
                     const h2g_key_options* opts, uint64_t* pk_out) {
  NEED_DEV_P();
  int cosets = H2G_COSETS_RESIDENT;
  RCCHK(key_options_mode(opts, "pk_read", &cosets));
  Params* it = find_params(params);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown params");
  if (!circuit || !buf || !pk_out) return fail(H2G_ERR_ARG, "pk_read: null argument");
  if (format != SERDE_RAW && format != SERDE_RAW_UNCHECKED && format != SERDE_PROCESSED)
    return fail(H2G_ERR_ARG, "pk_read: unknown SerdeFormat");
  const bool proc = format == SERDE_PROCESSED;
  ByteReader r{buf, len};
  const uint32_t k = circuit->k, F = circuit->num_fixed, P = circuit->num_perm_columns;
  if (k != it->k) return fail(H2G_ERR_ARG, "pk_read: k does not match");
  std::vector<G1Affine> vf, vp;
  RCCHK(vk_read_prefix(r, format, circuit, "pk_read", &vf, &vp));
  // the extended domain size follows from the constraint system (keygen::create_domain):
  // taken from the first polynomial here and checked against the keygen's below
  const size_t n = (size_t)1 << k;
  PkImage img;
  const uint8_t *l0, *ll, *la;
  const uint32_t ext_len = r.u32be();
  if (!r.ok || ext_len < n || (ext_len & (ext_len - 1))) return fail(H2G_ERR_ARG, "pk_read: bad l0 length");
  l0 = r.take((size_t)ext_len * sizeof(Fr));
  ll = r.poly(ext_len);
  la = r.poly(ext_len);
  img.l0 = l0;
  img.l_last = ll;
  img.l_active = la;
  r.polys(img.fixed_lag, F, n);
  r.polys(img.fixed_poly, F, n);
  r.polys(img.fixed_coset, F, ext_len);
  r.polys(img.sigma_lag, P, n);
  r.polys(img.sigma_poly, P, n);
  r.polys(img.sigma_coset, P, ext_len);
  if (!r.ok) return fail(H2G_ERR_ARG, "pk_read: truncated or mis-sized proving key");
  if (r.pos != len) return fail(H2G_ERR_ARG, "pk_read: trailing bytes");
  DevScratch bad;
  if (proc) {
    img.canonical = true;
    HIPCHK(hipMalloc(&bad.p, 4));
    HIPCHK(hipMemsetAsync(bad.p, 0, 4, d->stream));
    img.bad = (uint32_t*)bad.p;
  }
  DevScratch bad_raw;
  if (cosets && format == SERDE_RAW) {
    HIPCHK(hipMalloc(&bad_raw.p, 4));
    HIPCHK(hipMemsetAsync(bad_raw.p, 0, 4, d->stream));
    img.bad_raw = (uint32_t*)bad_raw.p;
  }
  auto pk = std::make_unique<ProvingKey>();
  pk->params = params;
  pk->cosets = cosets;
  int rc = keygen_impl(d, *it, circuit, *pk, &img);
  if (rc == H2G_OK && proc) {
    uint32_t nbad = 0;
    if (hipMemcpyAsync(&nbad, bad.p, 4, hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
        hipStreamSynchronize(d->stream) != hipSuccess)
      rc = fail(H2G_ERR_DEVICE, "pk_read: counter copy");
    else if (nbad) rc = fail(H2G_ERR_ARG, "pk_read: " + std::to_string(nbad) + " field elements not below the modulus");
  }
  if (rc == H2G_OK && pk->ext != ext_len) rc = fail(H2G_ERR_ARG, "pk_read: extended domain size does not match the circuit");
  if (rc == H2G_OK && format == SERDE_RAW) {
    // (a streamed key counted its cosets as they passed through scratch: img.bad_raw)
    std::vector<std::pair<const Fr*, size_t>> arrays;
    if (!cosets) arrays = {{pk->l0, pk->ext}, {pk->l_last, pk->ext}, {pk->l_active, pk->ext}};
    for (int i = 0; i < pk->cs.F; i++) {
      arrays.push_back({pk->fixed_lag[i], n});
      arrays.push_back({pk->fixed_poly[i], n});
      if (!cosets) arrays.push_back({pk->fixed_coset[i], pk->ext});
    }
    for (int i = 0; i < pk->cs.P; i++) {
      arrays.push_back({pk->sigma_lag[i], n});
      arrays.push_back({pk->sigma_poly[i], n});
      if (!cosets) arrays.push_back({pk->sigma_coset[i], pk->ext});
    }
    uint32_t nbad = 0, nbad_dropped = 0;
    rc = count_bad_fr(arrays, d->stream, &nbad);
    if (rc == H2G_OK && img.bad_raw) {
      if (hipMemcpy(&nbad_dropped, img.bad_raw, 4, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(H2G_ERR_DEVICE, "pk_read: counter copy");
      nbad += nbad_dropped;
    }
    if (rc == H2G_OK && nbad) rc = fail(H2G_ERR_ARG, "pk_read: " + std::to_string(nbad) + " field elements not below the modulus");
  }
  if (rc) return rc;
  pk->vk_fixed = vf;
  pk->vk_perm = vp;
  *pk_out = g_next_handle++;
  g_pks[*pk_out] = std::move(pk);
  return H2G_OK;
}

}  // extern "C"
