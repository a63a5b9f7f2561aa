// params.cpp -- the KZG params object: the SRS in both bases, their fixed-base windows,
// the lookup commitments' prefix basis, and the h2g_params_* entry points.
#include "g1_fft.h"
#include "prover_state.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace h2g {
namespace prv {
std::map<uint64_t, std::unique_ptr<Params>> g_params;
}  // namespace prv
}  // namespace h2g

namespace {
// The lookup commitments' basis.  A lookup's permuted columns A', S' are sorted into runs
// of equal values (permute_expression_pair), so with P_i = L_0 + ... + L_i,
//   sum_i a_i L_i = sum_i (a_i - a_{i+1}) P_i   (a_n = 0; the sum telescopes),
// the same commitment from scalars that are zero inside every run: the MSM's partition
// drops zero digits at the source, so its work follows the number of runs, not n.
// Windows of the prefix basis: for all n points (fgp; keygen builds them for keys with
// lookups, outside any proof) or for the rank's slab (sgp; built on the first set-2 MSM
// inside the slab, so a peer that only serves slabs never holds the full-size table).  Both
// need the prefix points of the whole basis (P_i sums every L_j below i), formed in scratch.
int params_prefix_build(Params& p, hipStream_t st, size_t lo, size_t hi, MsmFixedBase* out) {
  G1Affine* pre = nullptr;
  HIPCHK(hipMalloc(&pre, p.n * sizeof(G1Affine)));
  hipError_t e = msm_prefix_points(p.gl, p.n, pre, st);
  if (e == hipSuccess) e = msm_fixed_base_build(pre + lo, hi - lo, 0, out, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(pre);
  HIPCHK(e);
  return H2G_OK;
}
}  // namespace

namespace h2g {
namespace prv {
// before set-2 MSMs over [off, off + n): the slab's windows serve it if they exist, else the
// full windows, built here if nothing built them earlier (a fallback; normally a no-op)
int params_prefix(Params& p, hipStream_t st, size_t off, size_t n) {
  if (p.slab_hi > p.slab_lo && off >= p.slab_lo && off + n <= p.slab_hi && n > 0) {
    // inside this rank's slab: the slab's windows, built on first use (not in
    // h2g_params_set_slab, so params used without lookups never pay for them)
    if (!p.sgp.table) RCCHK(params_prefix_build(p, st, p.slab_lo, p.slab_hi, &p.sgp));
    return H2G_OK;
  }
  if (p.fgp.table) return H2G_OK;
  return params_prefix_build(p, st, 0, p.n, &p.fgp);
}

int params_finish(Params& p, hipStream_t st) {
  HIPCHK(msm_fixed_base_build(p.g, p.n, 0, &p.fg, st));
  HIPCHK(msm_fixed_base_build(p.gl, p.n, 0, &p.fgl, st));
  HIPCHK(hipStreamSynchronize(st));
  return H2G_OK;
}
}  // namespace prv
}  // namespace h2g

extern "C" {

int h2g_params_create(uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, uint64_t* handle) {
  NEED_DEV_P();
  if (!g || !g_lagrange || !handle || k > 27) return fail(H2G_ERR_ARG, "params_create: bad arguments");
  auto p = std::make_unique<Params>();
  p->device = d->id;
  p->k = k;
  p->n = (size_t)1 << k;
  PALLOC(p->pool, p->g, p->n);
  PALLOC(p->pool, p->gl, p->n);
  HIPCHK(hipMemcpy(p->g, g, p->n * sizeof(G1Affine), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p->gl, g_lagrange, p->n * sizeof(G1Affine), hipMemcpyHostToDevice));
  RCCHK(params_finish(*p, d->stream));
  *handle = g_next_handle++;
  g_params[*handle] = std::move(p);
  return H2G_OK;
}

int h2g_params_setup(uint32_t k, const uint64_t s_limbs[4], uint64_t* handle) {
  NEED_DEV_P();
  if (!s_limbs || !handle || k > 27) return fail(H2G_ERR_ARG, "params_setup: bad arguments");
  hipStream_t st = d->stream;
  auto p = std::make_unique<Params>();
  p->device = d->id;
  p->k = k;
  p->n = (size_t)1 << k;
  const size_t n = p->n;
  PALLOC(p->pool, p->g, n);
  PALLOC(p->pool, p->gl, n);
  const Fr s = fr_from_limbs(s_limbs);
  HIPCHK(srs_setup(s, n, p->g, st));
  Fr omega = root_of_unity();
  for (uint32_t i = k; i < FR_S; i++) omega = sqr(omega);
  Pool tmp;
  PowTable om;
  RCCHK(build_pow_table(tmp, omega, (int)k, &om, st));
  Fr *sc, *scr;
  HIPCHK(tmp.get((void**)&sc, n * sizeof(Fr)));
  HIPCHK(tmp.get((void**)&scr, n * sizeof(Fr)));
  const Fr mult = (pow_u64(s, n) - Fr::one()) * inv(from_u64<FrParams>(n));
  HIPCHK(srs_lagrange_scalars(sc, n, s, mult, om, scr, st));
  HIPCHK(g1_generator_mul(sc, n, p->gl, st));
  HIPCHK(hipStreamSynchronize(st));
  RCCHK(params_finish(*p, st));
  // g2 = generator, s_g2 = [s] g2 (kzg/commitment.rs:122-123)
  p->g2 = g2_generator();
  const Fr s_can = to_canonical(s);
  p->s_g2 = g2_mul(p->g2, s_can.l);
  p->has_g2 = true;
  *handle = g_next_handle++;
  g_params[*handle] = std::move(p);
  return H2G_OK;
}

/* ParamsKZG::from_parts (kzg/commitment.rs:135-154); g_lagrange == NULL: g_to_lagrange on the device */
int h2g_params_from_parts(uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint64_t g2[16],
                          const uint64_t s_g2[16], uint64_t* handle) {
  NEED_DEV_P();
  if (!g || !handle || k > G1FFT_MAX_K) return fail(H2G_ERR_ARG, "params_from_parts: bad arguments");
  if (!g2 != !s_g2) return fail(H2G_ERR_ARG, "params_from_parts: g2 and s_g2 go together (both or neither)");
  G2Affine a, b;
  if (g2) {
    std::memcpy(&a, g2, sizeof(G2Affine));
    std::memcpy(&b, s_g2, sizeof(G2Affine));
    if (!g2_valid(a) || !g2_valid(b)) return fail(H2G_ERR_ARG, "params_from_parts: invalid G2 point");
  }
  auto p = std::make_unique<Params>();
  p->device = d->id;
  p->k = k;
  p->n = (size_t)1 << k;
  PALLOC(p->pool, p->g, p->n);
  PALLOC(p->pool, p->gl, p->n);
  HIPCHK(hipMemcpy(p->g, g, p->n * sizeof(G1Affine), hipMemcpyHostToDevice));
  if (g_lagrange)
    HIPCHK(hipMemcpy(p->gl, g_lagrange, p->n * sizeof(G1Affine), hipMemcpyHostToDevice));
  else
    RCCHK(g1_to_lagrange(p->g, k, p->gl, d->stream));
  if (g2) {
    p->g2 = a;
    p->s_g2 = b;
    p->has_g2 = true;
  }
  RCCHK(params_finish(*p, d->stream));
  *handle = g_next_handle++;
  g_params[*handle] = std::move(p);
  return H2G_OK;
}

/* ParamsKZG::downsize (kzg/commitment.rs:291-299) into a new object; the source is only read */
int h2g_params_downsize(uint64_t params, uint32_t k, uint64_t* handle) {
  NEED_DEV_P();
  if (!handle) return fail(H2G_ERR_ARG, "params_downsize: null handle output");
  Params* it = find_params(params);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown params");
  const Params& src = *it;
  if (src.device != d->id) return fail(H2G_ERR_ARG, "params_downsize: params live on another device");
  if (k > src.k || k > G1FFT_MAX_K)
    return fail(H2G_ERR_ARG, "params_downsize: k = " + std::to_string(k) + " above the params' " + std::to_string(src.k));
  hipStream_t st = d->stream;
  auto p = std::make_unique<Params>();
  p->device = d->id;
  p->k = k;
  p->n = (size_t)1 << k;
  PALLOC(p->pool, p->g, p->n);
  PALLOC(p->pool, p->gl, p->n);
  HIPCHK(hipMemcpyAsync(p->g, src.g, p->n * sizeof(G1Affine), hipMemcpyDeviceToDevice, st));
  RCCHK(g1_to_lagrange(p->g, k, p->gl, st));
  p->has_g2 = src.has_g2;
  p->g2 = src.g2;
  p->s_g2 = src.s_g2;
  RCCHK(params_finish(*p, st));
  *handle = g_next_handle++;
  g_params[*handle] = std::move(p);
  return H2G_OK;
}

int h2g_params_export(uint64_t params, uint64_t* g, uint64_t* g_lagrange) {
  NEED_DEV_P();
  Params* it = find_params(params);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown params");
  if (g) HIPCHK(hipMemcpy(g, it->g, it->n * sizeof(G1Affine), hipMemcpyDeviceToHost));
  if (g_lagrange) HIPCHK(hipMemcpy(g_lagrange, it->gl, it->n * sizeof(G1Affine), hipMemcpyDeviceToHost));
  return H2G_OK;
}

int h2g_params_free(uint64_t params) {
  NEED_DEV_P();
  if (!g_params.erase(params)) return fail(H2G_ERR_HANDLE, "unknown params");
  return H2G_OK;
}

/* the G2 points of the params: 16 u64 each (x.c0, x.c1, y.c0, y.c1, Montgomery) */
int h2g_params_g2(uint64_t params, uint64_t g2[16], uint64_t s_g2[16]) {
  NEED_DEV_P();
  Params* it = find_params(params);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown params");
  if (!it->has_g2) return fail(H2G_ERR_STATE, "params have no G2 points");
  if (g2) std::memcpy(g2, &it->g2, sizeof(G2Affine));
  if (s_g2) std::memcpy(s_g2, &it->s_g2, sizeof(G2Affine));
  return H2G_OK;
}
int h2g_params_set_g2(uint64_t params, const uint64_t g2[16], const uint64_t s_g2[16]) {
  NEED_DEV_P();
  Params* it = find_params(params);
  if (!it) return fail(H2G_ERR_HANDLE, "unknown params");
  if (!g2 || !s_g2) return fail(H2G_ERR_ARG, "params_set_g2: null argument");
  G2Affine a, b;
  std::memcpy(&a, g2, sizeof(G2Affine));
  std::memcpy(&b, s_g2, sizeof(G2Affine));
  if (!g2_valid(a) || !g2_valid(b)) return fail(H2G_ERR_ARG, "params_set_g2: invalid G2 point");
  it->g2 = a;
  it->s_g2 = b;
  it->has_g2 = true;
  return H2G_OK;
}

int h2g_params_set_slab(uint64_t params, uint64_t lo, uint64_t hi) {
  NEED_DEV_P();
  Params* ip = find_params(params);
  if (!ip) return fail(H2G_ERR_HANDLE, "unknown params");
  Params& prm = *ip;
  if (prm.device != d->id) return fail(H2G_ERR_ARG, "params_set_slab: params live on another device");
  if (lo > hi || hi > prm.n) return fail(H2G_ERR_ARG, "params_set_slab: bad range");
  msm_fixed_base_free(&prm.sg);
  msm_fixed_base_free(&prm.sgl);
  msm_fixed_base_free(&prm.sgp);
  prm.slab_lo = prm.slab_hi = 0;
  if (hi == lo || (lo == 0 && hi == prm.n)) return H2G_OK;  // none / the full tables
  HIPCHK(msm_fixed_base_build(prm.g + lo, hi - lo, 0, &prm.sg, d->stream));
  HIPCHK(msm_fixed_base_build(prm.gl + lo, hi - lo, 0, &prm.sgl, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  // the lookup basis's windows for the slab (sgp) are built on the first set-2 MSM inside
  // the slab (params_prefix), so a peer serving set-2 slabs never builds the full-size table
  prm.slab_lo = lo;
  prm.slab_hi = hi;
  return H2G_OK;
}

int h2g_params_table_bytes(uint64_t params, uint64_t out[4]) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Params* ip = find_params(params);
  if (!ip) return fail(H2G_ERR_HANDLE, "unknown params");
  if (!out) return fail(H2G_ERR_ARG, "params_table_bytes: null output");
  const Params& p = *ip;
  auto bytes = [](const MsmFixedBase& t) -> uint64_t {
    return t.table ? (uint64_t)t.W * (uint64_t)t.n * sizeof(G1Affine) : 0;
  };
  out[0] = bytes(p.fg) + bytes(p.fgl);
  out[1] = bytes(p.sg) + bytes(p.sgl);
  out[2] = bytes(p.fgp);
  out[3] = bytes(p.sgp);
  return H2G_OK;
}

int h2g_params_msm_dev(uint64_t params, int32_t base_set, uint64_t offset, uint64_t n, const void* d_scalars,
                       uint64_t out_affine[8], int32_t* out_is_identity) {
  NEED_DEV_P();
  Params* ip = find_params(params);
  if (!ip) return fail(H2G_ERR_HANDLE, "unknown params");
  Params& prm = *ip;
  if (prm.device != d->id) return fail(H2G_ERR_ARG, "params_msm_dev: params live on another device");
  if (base_set < SRS_G || base_set > SRS_LAGRANGE_PREFIX || offset > prm.n || n > prm.n - offset || !out_affine ||
      (n && !d_scalars))
    return fail(H2G_ERR_ARG, "params_msm_dev: bad arguments");
  if (base_set == SRS_LAGRANGE_PREFIX) RCCHK(params_prefix(prm, d->stream, offset, n));
  int id = 0;
  size_t toff = 0;
  const MsmFixedBase& tb = prm.tables(base_set, offset, n, &toff);
  RCCHK(msm_fixed_host_impl(d, d_scalars, tb, toff, n, out_affine, &id, d->stream));
  if (out_is_identity) *out_is_identity = id;
  return H2G_OK;
}

}  // extern "C"
