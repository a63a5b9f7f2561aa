// kzg.cpp -- the polynomial-commitment layer of the C ABI on its own: transcript objects,
// ParamsKZG::commit / commit_lagrange, eval_polynomial, kate_division and the multi-open
// prover (h2g_multiopen_prove).  The multi-open argument itself is multiopen.cpp, shared with
// create_proof; h2g_multiopen_verify stands beside the plonk verifier (verifier.cpp).
//   Blake2bWrite/Read, Keccak256Write/Read   halo2_backend/src/transcript.rs:291-463
//   ParamsKZG::commit / commit_lagrange      poly/kzg/commitment.rs:305-317,354-366
//   eval_polynomial, kate_division           arithmetic.rs:57-82,101-120
//   Prover::create_proof                     poly/commitment.rs:141-168
#include "multiopen.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace h2g {
namespace prv {
std::map<uint64_t, std::unique_ptr<TranscriptObj>> g_transcripts;

bool TranscriptObj::read_point(G1Affine* out) {
  if (!read || bytes.size() - pos < 32) return false;
  G1Affine p;
  if (!g1_from_bytes_host(bytes.data() + pos, &p) || p.is_identity()) return false;
  if (!tr.common_point(p)) return false;
  pos += 32;
  *out = p;
  return true;
}
bool TranscriptObj::read_scalar(Fr* out) {
  if (!read || bytes.size() - pos < 32) return false;
  Fr c;
  std::memcpy(c.l, bytes.data() + pos, 32);
  unsigned br = 0;
  for (int i = 0; i < 8; i++) (void)__builtin_subc(c.l[i], FrParams::M[i], br, &br);
  if (!br) return false;  // from_repr refuses values >= r
  const Fr v = from_canonical(c);
  tr.common_scalar(v);
  pos += 32;
  *out = v;
  return true;
}
}  // namespace prv
}  // namespace h2g

namespace {
bool fr_reduced(const Fr& a) {
  unsigned br = 0;
  for (int i = 0; i < 8; i++) (void)__builtin_subc(a.l[i], FrParams::M[i], br, &br);
  return br != 0;
}
bool fq_reduced(const Fq& a) {
  unsigned br = 0;
  for (int i = 0; i < 8; i++) (void)__builtin_subc(a.l[i], FqParams::M[i], br, &br);
  return br != 0;
}
// a caller's G1Affine as a transcript takes it: coordinates below p, on the curve, not the identity
bool point_arg(const uint64_t p[8], G1Affine* out) {
  std::memcpy(out, p, sizeof(G1Affine));
  if (!fq_reduced(out->x) || !fq_reduced(out->y) || out->is_identity()) return false;
  return sqr(out->y) == sqr(out->x) * out->x + from_u64<FqParams>(3);
}
#define NEED_TRANSCRIPT(t)                                  \
  std::lock_guard<std::recursive_mutex> _lk(g_mu);          \
  TranscriptObj* T = find_transcript(t);                    \
  if (!T) return fail(H2G_ERR_HANDLE, "unknown transcript");

// h2g_multiopen_prove's device scratch, kept with the params (grow-only; freed with them)
struct MultiopenWs {
  Pool pool;
  Fr *nx = nullptr, *hx = nullptr, *lx = nullptr, *q1 = nullptr, *scr = nullptr;
  DevArr<Fr> small;
  std::vector<Fr*> gwc_q;
};

int commit_impl(Device* d, Params& prm, int set, const Fr* d_scalars, size_t len, uint64_t out[8], int* is_identity,
                hipStream_t st) {
  int id = 1;
  if (len == 0) {
    std::memset(out, 0, 64);
  } else {
    size_t toff = 0;
    const MsmFixedBase& tb = prm.tables(set, 0, len, &toff);
    RCCHK(msm_fixed_host_impl(d, d_scalars, tb, toff, len, out, &id, st));
  }
  if (is_identity) *is_identity = id;
  return H2G_OK;
}
int commit_entry(uint64_t params, int set, const void* scalars, bool on_device, size_t len, uint64_t out[8],
                 int* is_identity, void* stream) {
  NEED_DEV_P();
  Params* ip = find_params(params);
  if (!ip) return fail(H2G_ERR_HANDLE, "unknown params");
  Params& prm = *ip;
  if (prm.device != d->id) return fail(H2G_ERR_ARG, "commit: params live on another device");
  if (!out || (len && !scalars)) return fail(H2G_ERR_ARG, "commit: null argument");
  if (len > prm.n) return fail(H2G_ERR_ARG, "commit: more coefficients than the params have points");
  if (on_device) {
    if ((uintptr_t)scalars % 16) return fail(H2G_ERR_ARG, "commit: device scalars must be 16-byte aligned");
    return commit_impl(d, prm, set, (const Fr*)scalars, len, out, is_identity, pick_stream(d, stream));
  }
  HIPCHK(d->a.ensure(len * sizeof(Fr) + 32));
  HIPCHK(hipMemcpyAsync(d->a.p, scalars, len * sizeof(Fr), hipMemcpyHostToDevice, d->stream));
  return commit_impl(d, prm, set, d->a.as<Fr>(), len, out, is_identity, d->stream);
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------- transcript objects
int h2g_transcript_new_write(int kind, uint64_t* t) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!t) return fail(H2G_ERR_ARG, "transcript_new_write: null argument");
  if (kind != TRANSCRIPT_BLAKE2B && kind != TRANSCRIPT_KECCAK256)
    return fail(H2G_ERR_ARG, "transcript: kind must be 0 (Blake2b) or 1 (Keccak256)");
  *t = g_next_handle++;
  g_transcripts[*t] = std::make_unique<TranscriptObj>(false, kind);
  return H2G_OK;
}
int h2g_transcript_new_read(int kind, const uint8_t* proof, size_t len, uint64_t* t) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!t || (len && !proof)) return fail(H2G_ERR_ARG, "transcript_new_read: null argument");
  if (kind != TRANSCRIPT_BLAKE2B && kind != TRANSCRIPT_KECCAK256)
    return fail(H2G_ERR_ARG, "transcript: kind must be 0 (Blake2b) or 1 (Keccak256)");
  auto obj = std::make_unique<TranscriptObj>(true, kind);
  if (len) obj->bytes.assign(proof, proof + len);
  *t = g_next_handle++;
  g_transcripts[*t] = std::move(obj);
  return H2G_OK;
}
int h2g_transcript_free(uint64_t t) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!g_transcripts.erase(t)) return fail(H2G_ERR_HANDLE, "unknown transcript");
  return H2G_OK;
}
int h2g_transcript_common_point(uint64_t t, const uint64_t p[8]) {
  NEED_TRANSCRIPT(t);
  G1Affine a;
  if (!p || !point_arg(p, &a)) return fail(H2G_ERR_ARG, "transcript: not a point of the curve, or the identity");
  T->tr.common_point(a);
  return H2G_OK;
}
int h2g_transcript_common_scalar(uint64_t t, const uint64_t s[4]) {
  NEED_TRANSCRIPT(t);
  if (!s || !fr_reduced(fr_from_limbs(s))) return fail(H2G_ERR_ARG, "transcript: scalar not below r");
  T->tr.common_scalar(fr_from_limbs(s));
  return H2G_OK;
}
int h2g_transcript_write_point(uint64_t t, const uint64_t p[8]) {
  NEED_TRANSCRIPT(t);
  if (T->read) return fail(H2G_ERR_ARG, "transcript_write_point: a read-mode transcript");
  G1Affine a;
  if (!p || !point_arg(p, &a))
    return fail(H2G_ERR_ARG, "cannot write points at infinity (or off the curve) to the transcript");
  T->tr.write_point(a);
  return H2G_OK;
}
int h2g_transcript_write_scalar(uint64_t t, const uint64_t s[4]) {
  NEED_TRANSCRIPT(t);
  if (T->read) return fail(H2G_ERR_ARG, "transcript_write_scalar: a read-mode transcript");
  if (!s || !fr_reduced(fr_from_limbs(s))) return fail(H2G_ERR_ARG, "transcript: scalar not below r");
  T->tr.write_scalar(fr_from_limbs(s));
  return H2G_OK;
}
int h2g_transcript_read_point(uint64_t t, uint64_t p[8]) {
  NEED_TRANSCRIPT(t);
  if (!T->read) return fail(H2G_ERR_ARG, "transcript_read_point: a write-mode transcript");
  G1Affine a;
  if (!p || !T->read_point(&a))
    return fail(H2G_ERR_ARG, "transcript_read_point: the bytes end, or no valid encoding of a point other than the identity");
  std::memcpy(p, &a, sizeof(G1Affine));
  return H2G_OK;
}
int h2g_transcript_read_scalar(uint64_t t, uint64_t s[4]) {
  NEED_TRANSCRIPT(t);
  if (!T->read) return fail(H2G_ERR_ARG, "transcript_read_scalar: a write-mode transcript");
  Fr v;
  if (!s || !T->read_scalar(&v)) return fail(H2G_ERR_ARG, "transcript_read_scalar: the bytes end, or a value >= r");
  fr_to_limbs(v, s);
  return H2G_OK;
}
int h2g_transcript_squeeze(uint64_t t, uint64_t c[4]) {
  NEED_TRANSCRIPT(t);
  if (!c) return fail(H2G_ERR_ARG, "transcript_squeeze: null argument");
  fr_to_limbs(T->tr.squeeze(), c);
  return H2G_OK;
}
int h2g_transcript_bytes(uint64_t t, uint8_t* out, size_t cap, size_t* len) {
  NEED_TRANSCRIPT(t);
  if (T->read) return fail(H2G_ERR_ARG, "transcript_bytes: a read-mode transcript");
  if (!len) return fail(H2G_ERR_ARG, "transcript_bytes: null argument");
  *len = T->bytes.size();
  if (!out) return H2G_OK;
  if (cap < T->bytes.size()) return fail(H2G_ERR_ARG, "transcript_bytes: buffer too small");
  if (!T->bytes.empty()) std::memcpy(out, T->bytes.data(), T->bytes.size());
  return H2G_OK;
}
int h2g_transcript_remaining(uint64_t t, size_t* bytes) {
  NEED_TRANSCRIPT(t);
  if (!T->read) return fail(H2G_ERR_ARG, "transcript_remaining: a write-mode transcript");
  if (!bytes) return fail(H2G_ERR_ARG, "transcript_remaining: null argument");
  *bytes = T->bytes.size() - T->pos;
  return H2G_OK;
}

// ---------------------------------------------------------------- commitments
int h2g_params_commit(uint64_t params, const uint64_t* coeffs, size_t len, uint64_t out[8], int* is_identity) {
  return commit_entry(params, SRS_G, coeffs, false, len, out, is_identity, nullptr);
}
int h2g_params_commit_lagrange(uint64_t params, const uint64_t* evals, size_t len, uint64_t out[8], int* is_identity) {
  return commit_entry(params, SRS_LAGRANGE, evals, false, len, out, is_identity, nullptr);
}
int h2g_params_commit_dev(uint64_t params, const void* d_coeffs, size_t len, uint64_t out[8], int* is_identity,
                          void* stream) {
  return commit_entry(params, SRS_G, d_coeffs, true, len, out, is_identity, stream);
}
int h2g_params_commit_lagrange_dev(uint64_t params, const void* d_evals, size_t len, uint64_t out[8],
                                   int* is_identity, void* stream) {
  return commit_entry(params, SRS_LAGRANGE, d_evals, true, len, out, is_identity, stream);
}

// ---------------------------------------------------------------- eval_polynomial, kate_division
int h2g_fr_eval_dev(const void* d_poly, size_t len, const uint64_t x[4], uint64_t out[4], void* stream) {
  NEED_DEV_P();
  if (!x || !out || (len && !d_poly)) return fail(H2G_ERR_ARG, "fr_eval: null argument");
  if ((uintptr_t)d_poly % 16) return fail(H2G_ERR_ARG, "fr_eval: the polynomial must be 16-byte aligned");
  if (len == 0) {
    fr_to_limbs(Fr::zero(), out);
    return H2G_OK;
  }
  hipStream_t st = pick_stream(d, stream);
  // work: the request (64 B), the result (64 B), the kernel's partial sums
  const size_t scr = poly_eval_scratch_len(1, len);
  HIPCHK(d->work.ensure(128 + scr * sizeof(Fr)));
  uint8_t* w = d->work.as<uint8_t>();
  const EvalReq rq{(const Fr*)d_poly, (uint64_t)len, fr_from_limbs(x)};
  Fr r;
  HIPCHK(hipMemcpyAsync(w, &rq, sizeof(rq), hipMemcpyHostToDevice, st));
  HIPCHK(poly_eval_batch((const EvalReq*)w, 1, len, (Fr*)(w + 64), (Fr*)(w + 128), st));
  HIPCHK(hipMemcpyAsync(&r, w + 64, sizeof(Fr), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  fr_to_limbs(r, out);
  return H2G_OK;
}
int h2g_fr_eval(const uint64_t* poly, size_t len, const uint64_t x[4], uint64_t out[4]) {
  NEED_DEV_P();
  if (len && !poly) return fail(H2G_ERR_ARG, "fr_eval: null argument");
  HIPCHK(d->a.ensure(len * sizeof(Fr) + 32));
  HIPCHK(hipMemcpyAsync(d->a.p, poly, len * sizeof(Fr), hipMemcpyHostToDevice, d->stream));
  return h2g_fr_eval_dev(d->a.p, len, x, out, nullptr);
}
int h2g_kate_division_dev(const void* d_a, size_t len, const uint64_t b[4], void* d_q, void* stream) {
  NEED_DEV_P();
  if (len == 0) return fail(H2G_ERR_ARG, "kate_division: an empty polynomial");
  if (!d_a || !b || (len > 1 && !d_q)) return fail(H2G_ERR_ARG, "kate_division: null argument");
  if ((uintptr_t)d_a % 16 || (uintptr_t)d_q % 16)
    return fail(H2G_ERR_ARG, "kate_division: device arrays must be 16-byte aligned");
  if (len == 1) return H2G_OK;
  HIPCHK(d->work.ensure(kate_scratch_len(len) * sizeof(Fr) + 32));
  HIPCHK(kate_division((const Fr*)d_a, len, fr_from_limbs(b), (Fr*)d_q, d->work.as<Fr>(), pick_stream(d, stream)));
  return H2G_OK;
}
int h2g_debug_kate_division_dev(const void* d_a, size_t len, const uint64_t b[4], void* d_q, int accumulate,
                                int tile_s, void* stream) {
  NEED_DEV_P();
  if (len == 0) return fail(H2G_ERR_ARG, "kate_division: an empty polynomial");
  if (!d_a || !b || (len > 1 && !d_q)) return fail(H2G_ERR_ARG, "kate_division: null argument");
  if ((uintptr_t)d_a % 16 || (uintptr_t)d_q % 16)
    return fail(H2G_ERR_ARG, "kate_division: device arrays must be 16-byte aligned");
  if (tile_s != 0 && tile_s != 8 && tile_s != 16 && tile_s != 32 && tile_s != 64)
    return fail(H2G_ERR_ARG, "debug_kate_division: tile_s must be 0, 8, 16, 32 or 64");
  if (len == 1) return H2G_OK;
  HIPCHK(d->work.ensure(kate_scratch_len(len) * sizeof(Fr) + 32));
  HIPCHK(kate_division((const Fr*)d_a, len, fr_from_limbs(b), (Fr*)d_q, d->work.as<Fr>(), pick_stream(d, stream),
                       accumulate != 0, tile_s));
  return H2G_OK;
}
int h2g_debug_kate_tile_s(size_t len, int* tile_s) {
  if (len == 0) return fail(H2G_ERR_ARG, "kate_division: an empty polynomial");
  if (!tile_s) return fail(H2G_ERR_ARG, "debug_kate_tile_s: null argument");
  *tile_s = kate_tile_s((uint64_t)len - 1);
  return H2G_OK;
}
int h2g_kate_division(const uint64_t* a, size_t len, const uint64_t b[4], uint64_t* q) {
  NEED_DEV_P();
  if (len == 0) return fail(H2G_ERR_ARG, "kate_division: an empty polynomial");
  if (!a || !b || (len > 1 && !q)) return fail(H2G_ERR_ARG, "kate_division: null argument");
  if (len == 1) return H2G_OK;
  HIPCHK(d->a.ensure(len * sizeof(Fr) + 32));
  HIPCHK(d->b.ensure(len * sizeof(Fr) + 32));
  HIPCHK(hipMemcpyAsync(d->a.p, a, len * sizeof(Fr), hipMemcpyHostToDevice, d->stream));
  RCCHK(h2g_kate_division_dev(d->a.p, len, b, d->b.p, nullptr));
  HIPCHK(hipMemcpyAsync(q, d->b.p, (len - 1) * sizeof(Fr), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  return H2G_OK;
}

// ---------------------------------------------------------------- Prover::create_proof
int h2g_multiopen_prove(uint64_t params, int scheme, uint64_t transcript, const h2g_poly_ref* polys, size_t npolys,
                        const h2g_open_query* queries, size_t nqueries) {
  NEED_DEV_P();
  Params* ip = find_params(params);
  if (!ip) return fail(H2G_ERR_HANDLE, "unknown params");
  TranscriptObj* T = find_transcript(transcript);
  if (!T) return fail(H2G_ERR_HANDLE, "unknown transcript");
  Params& prm = *ip;
  if (prm.device != d->id) return fail(H2G_ERR_ARG, "multiopen_prove: params live on another device");
  if (scheme != MULTIOPEN_SHPLONK && scheme != MULTIOPEN_GWC)
    return fail(H2G_ERR_ARG, "multiopen_prove: scheme must be 0 (SHPLONK) or 1 (GWC)");
  if (T->read) return fail(H2G_ERR_ARG, "multiopen_prove: a read-mode transcript");
  if (!polys || !queries || npolys == 0 || nqueries == 0)
    return fail(H2G_ERR_ARG, "multiopen_prove: no polynomials or no queries");
  if (npolys > (1u << 24) || nqueries > (1u << 24)) return fail(H2G_ERR_ARG, "multiopen_prove: too many queries");
  const size_t n = prm.n;
  if (n < 2) return fail(H2G_ERR_ARG, "multiopen_prove: params of a single point");
  // the commitments' MSMs would be cut into the transport's slabs (commit_launch): the
  // standalone argument is single-device
  if (g_spmd.world > 1 || g_shard.world > 1)
    return fail(H2G_ERR_STATE, "multiopen_prove: a shard or SPMD transport is installed");
  for (size_t i = 0; i < npolys; i++) {
    const h2g_poly_ref& p = polys[i];
    if (!p.coeffs || p.len == 0) return fail(H2G_ERR_ARG, "multiopen_prove: polynomial " + std::to_string(i) + " is empty");
    if (p.len > n)
      return fail(H2G_ERR_ARG, "multiopen_prove: polynomial " + std::to_string(i) + " is longer than the params' n");
    if (p.on_device && (uintptr_t)p.coeffs % 16)
      return fail(H2G_ERR_ARG, "multiopen_prove: device polynomial " + std::to_string(i) + " is not 16-byte aligned");
  }
  std::vector<OpenQ> qs(nqueries);
  for (size_t i = 0; i < nqueries; i++) {
    if (queries[i].poly >= npolys)
      return fail(H2G_ERR_ARG, "multiopen_prove: query " + std::to_string(i) + " names an unknown polynomial");
    qs[i] = {(int)queries[i].poly, fr_from_limbs(queries[i].point)};
    if (!fr_reduced(qs[i].pt)) return fail(H2G_ERR_ARG, "multiopen_prove: query " + std::to_string(i) + ": point not below r");
  }
  hipStream_t st = d->stream;
  if (!prm.kzg_ws) prm.kzg_ws = std::make_shared<MultiopenWs>();
  MultiopenWs& ws = *static_cast<MultiopenWs*>(prm.kzg_ws.get());
  if (!ws.nx) {
    PALLOC(ws.pool, ws.nx, n);
    PALLOC(ws.pool, ws.hx, n);
    PALLOC(ws.pool, ws.lx, n);
    PALLOC(ws.pool, ws.q1, n);
    PALLOC(ws.pool, ws.scr, kate_scratch_len(n));
  }
  HIPCHK(ws.small.ensure(nqueries + 1));
  // this call's own allocations: host polynomials brought to the device, the evaluations
  Pool call;
  MsmRingGuard ring_guard{d};
  StreamSyncGuard guard{st};  // nothing of `call` is freed, no host staging dropped, under a running kernel
  std::vector<PolyRef> prs(npolys);
  for (size_t i = 0; i < npolys; i++) {
    const h2g_poly_ref& p = polys[i];
    if (p.on_device) {
      prs[i] = {(const Fr*)p.coeffs, (uint64_t)p.len};
      continue;
    }
    Fr* dp;
    PALLOC(call, dp, p.len);
    HIPCHK(hipMemcpyAsync(dp, p.coeffs, p.len * sizeof(Fr), hipMemcpyHostToDevice, st));
    prs[i] = {dp, (uint64_t)p.len};
  }
  // the evaluations: every distinct (polynomial, point), one batched launch
  std::vector<OpenQ> keys;
  std::vector<std::vector<int>> of(npolys);
  auto index = [&](int poly, const Fr& pt) -> int {
    for (int i : of[poly])
      if (keys[i].pt == pt) return i;
    return -1;
  };
  for (const OpenQ& q : qs)
    if (index(q.poly, q.pt) < 0) {
      keys.push_back(q);
      of[q.poly].push_back((int)keys.size() - 1);
    }
  const int nreq = (int)keys.size();
  std::vector<Fr> evals(nreq);
  {
    uint64_t max_len = 1;
    std::vector<EvalReq> reqs(nreq);
    for (int i = 0; i < nreq; i++) {
      reqs[i] = EvalReq{prs[keys[i].poly].p, prs[keys[i].poly].len, keys[i].pt};
      max_len = std::max<uint64_t>(max_len, reqs[i].len);
    }
    EvalReq* d_reqs;
    Fr *d_out, *d_scr;
    PALLOC(call, d_reqs, nreq);
    PALLOC(call, d_out, nreq);
    PALLOC(call, d_scr, poly_eval_scratch_len(nreq, max_len));
    HIPCHK(hipMemcpyAsync(d_reqs, reqs.data(), nreq * sizeof(EvalReq), hipMemcpyHostToDevice, st));
    HIPCHK(poly_eval_batch(d_reqs, nreq, max_len, d_out, d_scr, st));
    HIPCHK(hipMemcpyAsync(evals.data(), d_out, nreq * sizeof(Fr), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  // the argument runs on a copy of the transcript: a failed call (an identity commitment)
  // leaves the caller's as it was
  TranscriptObj run = *T;
  MultiopenCtx c;
  c.d = d;
  c.prm = &prm;
  c.st = st;
  c.tr = &run.tr;
  c.n = n;
  c.polys = &prs;
  c.queries = &qs;
  c.ev = [&](int poly, const Fr& pt) { return evals[index(poly, pt)]; };
  c.nx = ws.nx, c.hx = ws.hx, c.lx = ws.lx, c.q1 = ws.q1, c.scr = ws.scr, c.small = ws.small.p;
  c.gwc_q = &ws.gwc_q;
  c.pool = &ws.pool;
  c.upload = [st](void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  };
  c.sl = Slab{0, n, n};
  RCCHK(scheme == MULTIOPEN_GWC ? multiopen_gwc(c) : multiopen_shplonk(c));
  HIPCHK(hipStreamSynchronize(st));
  *T = run;
  return H2G_OK;
}

}  // extern "C"
