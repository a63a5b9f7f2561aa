// check_witness.cpp -- h2g_check_witness: MockProver::verify on the device.
#include "prover_state.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace {
// ------------------------------------------------------------------ check_witness
// MockProver::verify for a complete witness (halo2_frontend/src/dev.rs:742-1166) on circuit
// 0's workspace: the advice comes in as create_proof brings it in, rows [u, n) are filled as
// the prover will fill them (zero / Fr::random), then gates (dev.rs:849-925), lookups
// (:957-1052), shuffles (:1054-1112) and copies (:1114-1142) append to one record buffer
// (check.hip).  Nothing a later proof depends on is kept: the workspace columns, the
// challenge slots of pk.consts and tmp_a / tmp_b are rewritten by every proof, and the
// lookups' sort hints (lk_hb) are not touched -- the check sorts with buffers of its own.
int check_ws_prepare(ProvingKey& pk, size_t rec_cap, size_t ncopies) {
  ProvingKey::CheckWs& cw = pk.ck;
  const size_t u = pk.n - (size_t)(pk.cs.bf + 1);
  if (!cw.ready) {
    PALLOC(pk.pool, cw.total, 16);
    PALLOC(pk.pool, cw.sh_flags, pk.cs.NS + 1);
    PALLOC(pk.pool, cw.seeds, 8);
    PALLOC(pk.pool, cw.offs, 1);
    PALLOC(pk.pool, cw.blind, (size_t)std::max(pk.cs.A, 1) * (pk.cs.bf + 1));
    PALLOC(pk.pool, cw.cols, pk.cs.A + pk.cs.F + pk.cs.I + 1);
    PALLOC(pk.pool, cw.segs, pk.cs.A + 1);
    cw.ready = true;
  }
  if (pk.cs.NL + pk.cs.NS > 0 && !cw.sort_ready) {
    PALLOC(pk.pool, cw.canon, u);
    PALLOC(pk.pool, cw.sorted_a, u);
    PALLOC(pk.pool, cw.sorted_b, u);
    for (int q = 0; q < 2; q++) {
      PALLOC(pk.pool, cw.key[q], u);
      PALLOC(pk.pool, cw.idx[q], u);
    }
    HIPCHK(pk.pool.get(&cw.scr, radix_sort_scratch_bytes(u)));
    cw.sort_ready = true;
  }
  HIPCHK(cw.rec.ensure(rec_cap));
  HIPCHK(cw.copies.ensure(6 * ncopies));
  return H2G_OK;
}

int check_impl(Device* d, ProvingKey& pk, const h2g_check_inputs* in, h2g_check_failure* out, size_t cap,
               uint64_t* total) {
  hipStream_t st = d->stream;
  const size_t n = pk.n;
  const int bf = pk.cs.bf;
  const size_t u = n - (size_t)(bf + 1);
  const int NCH = (int)pk.cs.ch_phase.size();
  // ---- arguments, before anything on the device changes
  if (pk.cs.A && !in->advice) return fail(H2G_ERR_ARG, "check_witness: null advice");
  if (pk.cs.I && !in->instance) return fail(H2G_ERR_ARG, "check_witness: null instance");
  if (NCH && !in->challenges) return fail(H2G_ERR_ARG, "check_witness: the key has challenges, none were given");
  if (in->advice_on_device && pk.cs.A && (reinterpret_cast<uintptr_t>(in->advice) & 15) != 0)
    return fail(H2G_ERR_ARG, "check_witness: device advice must be 16-byte aligned");
  const uint32_t ncp = in->copies ? in->num_copies : 0;
  for (uint32_t i = 0; i < ncp; i++) {
    const int32_t* cp = in->copies + 6 * (size_t)i;
    for (int s = 0; s < 2; s++) {
      const int t = cp[3 * s], ix = cp[3 * s + 1], row = cp[3 * s + 2];
      const int lim = t == COL_ADVICE ? pk.cs.A : t == COL_FIXED ? pk.cs.F : t == COL_INSTANCE ? pk.cs.I : 0;
      if (ix < 0 || ix >= lim) return fail(H2G_ERR_ARG, "check_witness: copy " + std::to_string(i) + " names a column out of range");
      if (row < 0 || (size_t)row >= n) return fail(H2G_ERR_ARG, "check_witness: copy " + std::to_string(i) + " names a row out of range");
    }
  }
  const int G = (int)pk.seg_gate.size();
  // no more records than there can be failures
  const size_t most = (size_t)G * n + (size_t)pk.cs.NL * u + (size_t)ncp;
  const size_t rec_cap = out ? std::min(cap, most) : 0;
  xp_drain(pk);  // a failed proof's overlapped exchanges
  HIPCHK(hipStreamSynchronize(st));
  if (pk.cws.empty()) RCCHK(circuit_ws_add(pk));
  RCCHK(check_ws_prepare(pk, rec_cap, ncp));
  ProvingKey::CheckWs& cw = pk.ck;
  CircuitWs& w = *pk.cws[0];

  // ---- theta and the blinding rows' ChaCha20 key from the seed
  static const uint8_t kDefaultSeed[32] = {'h', '2', 'g', '-', 'c', 'h', 'e', 'c', 'k', '-', 'w', 'i', 't', 'n', 'e', 's', 's'};
  ChaChaRng rng(in->seed ? in->seed : kDefaultSeed);
  const Fr theta = rng.random_fr();
  uint32_t blind_key[8];
  rng.fill(reinterpret_cast<uint8_t*>(blind_key), sizeof(blind_key));
  const uint64_t blind_off = 0;
  std::vector<CopySeg> segs;
  StreamSyncGuard guard{st};  // the host staging above is read by asynchronous copies

  // ---- instances, advice (create_proof's upload / copy path), challenges
  for (int i = 0; i < pk.cs.I; i++)
    HIPCHK(hipMemcpyAsync(w.inst_val[i], in->instance + 4 * n * i, n * sizeof(Fr), hipMemcpyHostToDevice, st));
  if (in->advice_on_device) {
    ColCopy cc{};
    int ncc = 0;
    for (int c = 0; c < pk.cs.A; c++) {
      cc.src[ncc] = reinterpret_cast<const Fr*>(in->advice + 4 * n * c);
      cc.dst[ncc] = w.adv[c];
      cc.sum[ncc++] = nullptr;
      if (ncc == COPY_COLS_MAX || c + 1 == pk.cs.A) {
        HIPCHK(copy_columns(cc, ncc, n, false, st));
        ncc = 0;
      }
    }
  } else {
    for (int c = 0; c < pk.cs.A; c++)
      HIPCHK(hipMemcpyAsync(w.adv[c], in->advice + 4 * n * c, n * sizeof(Fr), hipMemcpyHostToDevice, st));
  }
  if (NCH) HIPCHK(hipMemcpyAsync(pk.consts + pk.num_consts, in->challenges, NCH * sizeof(Fr), hipMemcpyHostToDevice, st));
  // rows [u, n): zero for unblinded columns, Fr::random for the others (prover.rs:417-437)
  for (int c = 0; c < pk.cs.A; c++) {
    if (pk.unblinded[c]) HIPCHK(hipMemsetAsync(w.adv[c] + u, 0, (size_t)(bf + 1) * sizeof(Fr), st));
    else segs.push_back(CopySeg{cw.blind + (size_t)c * (bf + 1), w.adv[c] + u, (uint64_t)(bf + 1)});
  }
  if (!segs.empty()) {
    HIPCHK(hipMemcpyAsync(cw.seeds, blind_key, sizeof(blind_key), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cw.offs, &blind_off, sizeof(blind_off), hipMemcpyHostToDevice, st));
    HIPCHK(chacha_random_poly(cw.blind, (size_t)pk.cs.A * (bf + 1), cw.seeds, cw.offs, 1, st));
    HIPCHK(hipMemcpyAsync(cw.segs, segs.data(), segs.size() * sizeof(CopySeg), hipMemcpyHostToDevice, st));
    HIPCHK(copy_segments(cw.segs, (int)segs.size(), (uint64_t)(bf + 1), st));
  }
  HIPCHK(hipMemsetAsync(cw.total, 0, 16 * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(cw.sh_flags, 0, (size_t)(pk.cs.NS + 1) * sizeof(uint32_t), st));
  CheckSink sink;
  sink.rec = cw.rec.p;
  sink.total = cw.total;
  sink.cap = rec_cap;

  // ---- gates
  {
    GateCheckArgs ga;
    ga.prog = pk.prog;
    ga.segs = pk.d_seg_gate;
    ga.ngates = G;
    ga.n_slots = pk.n_slots;
    ga.consts = pk.consts;
    ga.load_col = w.d_load_col_lag;
    ga.load_rot = pk.d_load_rot;
    ga.n = n;
    ga.u = u;
    ga.sink = sink;
    HIPCHK(check_gates(ga, st));
  }
  // ---- lookups and shuffles through the theta-compression and the full canonical sort
  auto compress = [&](int2 seg, Fr* dst) -> int {
    CompressArgs ca;
    ca.prog = pk.prog;
    ca.seg = seg;
    ca.n_slots = pk.n_slots;
    ca.consts = pk.consts;
    ca.load_col = w.d_load_col_lag;
    ca.load_rot = pk.d_load_rot;
    ca.n = n;
    ca.theta = theta;
    ca.out = dst;
    HIPCHK(compress_lagrange(ca, st));
    return H2G_OK;
  };
  // rows [0, u) of src by Ord on Fr (permute_expression_pair's full sort: four stable
  // 64-bit limb sorts of the canonical values, least significant first)
  auto sort_canon = [&](const Fr* src, CanonKey* dst) -> int {
    HIPCHK(lookup_keys(src, u, 0, cw.canon, nullptr, nullptr, cw.total + 1, st));
    HIPCHK(iota_u32(cw.idx[0], u, st));
    for (int limb = 0; limb < 4; limb++) {  // 8 passes each: the result is back in the first pair
      HIPCHK(canon_limb_keys(cw.canon, cw.idx[0], u, limb, cw.key[0], st));
      bool alt = false;
      HIPCHK(radix_sort_pairs(cw.key[0], cw.idx[0], cw.key[1], cw.idx[1], u, 0, 64, cw.scr, st, &alt));
      if (alt) return fail(H2G_ERR_STATE, "check_witness: unexpected sort pass parity");
    }
    HIPCHK(lookup_gather(cw.canon, cw.idx[0], u, dst, cw.total + 5, st));
    return H2G_OK;
  };
  int sorted_tab = -1;  // the lookup whose table cw.sorted_b holds (equal tables are sorted once)
  for (int l = 0; l < pk.cs.NL; l++) {
    const int rep = (size_t)l < pk.lk_trep.size() ? pk.lk_trep[l] : l;
    if (rep != sorted_tab) {
      RCCHK(compress(pk.seg_lk_tab[rep], pk.tmp_b));
      RCCHK(sort_canon(pk.tmp_b, cw.sorted_b));
      sorted_tab = rep;
    }
    RCCHK(compress(pk.seg_lk_in[l], pk.tmp_a));
    HIPCHK(check_lookup_members(pk.tmp_a, cw.sorted_b, u, (uint32_t)l, sink, st));
  }
  for (int s = 0; s < pk.cs.NS; s++) {
    RCCHK(compress(pk.seg_sh_in[s], pk.tmp_a));
    RCCHK(compress(pk.seg_sh_sh[s], pk.tmp_b));
    RCCHK(sort_canon(pk.tmp_a, cw.sorted_a));
    RCCHK(sort_canon(pk.tmp_b, cw.sorted_b));
    HIPCHK(check_sorted_equal(cw.sorted_a, cw.sorted_b, u, cw.sh_flags + s, st));
  }
  // ---- copies
  if (ncp) {
    std::vector<const Fr*> cols((size_t)pk.cs.A + pk.cs.F + pk.cs.I + 1, nullptr);
    for (int c = 0; c < pk.cs.A; c++) cols[c] = w.adv[c];
    for (int c = 0; c < pk.cs.F; c++) cols[pk.cs.A + c] = pk.fixed_lag[c];
    for (int c = 0; c < pk.cs.I; c++) cols[pk.cs.A + pk.cs.F + c] = w.inst_val[c];
    HIPCHK(hipMemcpyAsync(cw.cols, cols.data(), cols.size() * sizeof(Fr*), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cw.copies.p, in->copies, (size_t)ncp * 6 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(check_copies(cw.cols, pk.cs.A, pk.cs.A + pk.cs.F, cw.copies.p, ncp, sink, st));
    HIPCHK(hipStreamSynchronize(st));  // `cols` is read by its upload
  }
  // ---- results
  unsigned long long dev_total = 0;
  std::vector<uint32_t> shf(pk.cs.NS + 1, 0);
  HIPCHK(hipMemcpyAsync(&dev_total, cw.total, sizeof(dev_total), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(shf.data(), cw.sh_flags, shf.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<h2g_check_failure> recs((size_t)std::min<unsigned long long>(dev_total, rec_cap));
  if (!recs.empty())
    HIPCHK(hipMemcpy(recs.data(), cw.rec.p, recs.size() * sizeof(h2g_check_failure), hipMemcpyDeviceToHost));
  uint64_t all = dev_total;
  for (int s = 0; s < pk.cs.NS; s++)
    if (shf[s]) {
      all++;
      recs.push_back(h2g_check_failure{H2G_CHECK_SHUFFLE, (uint32_t)s, H2G_CHECK_NO_ROW, 0});
    }
  std::sort(recs.begin(), recs.end(), [](const h2g_check_failure& a, const h2g_check_failure& b) {
    if (a.kind != b.kind) return a.kind < b.kind;
    if (a.index != b.index) return a.index < b.index;
    return a.row < b.row;
  });
  *total = all;
  if (out)
    for (size_t i = 0; i < recs.size() && i < cap; i++) out[i] = recs[i];
  return H2G_OK;
}
}  // namespace

extern "C" {

int h2g_check_witness(uint64_t pk, const h2g_check_inputs* in, h2g_check_failure* out, size_t cap, uint64_t* total) {
  NEED_DEV_P();
  ProvingKey* ik = find_pk(pk);
  if (!ik) return fail(H2G_ERR_HANDLE, "unknown proving key");
  if (!in || !total) return fail(H2G_ERR_ARG, "check_witness: null argument");
  ProvingKey& K = *ik;
  if (K.device != d->id) return fail(H2G_ERR_ARG, "check_witness: pk lives on another device");
  const int rc = check_impl(d, K, in, cap ? out : nullptr, cap, total);
  if (rc) (void)hipStreamSynchronize(d->stream);
  return rc;
}

}  // extern "C"
