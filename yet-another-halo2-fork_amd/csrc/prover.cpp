// prover.cpp -- keygen (keygen.cpp) and create_proof on the device (BN254 / KZG / SHPLONK).
//
// Host orchestration of halo2_backend's prover, all polynomial data resident in HBM:
//   keygen_vk / keygen_pk          plonk/keygen.rs:43-190, circuit.rs:95-180,292-320
//   permutation Assembly/build_pk  plonk/permutation/keygen.rs:16-213
//   Prover::new_with_engine        plonk/prover.rs:174-305 (instances)
//   commit_phase                   plonk/prover.rs:309-494 (every advice phase, challenges after each)
//   create_proof                   plonk/prover.rs:512-899
//   permutation_commit/evaluate    plonk/permutation/prover.rs:50-333
//   vanishing commit/construct     plonk/vanishing/prover.rs:40-205
//   evaluate_h                     plonk/evaluation.rs:317-483
//   SHPLONK / GWC                  poly/kzg/multiopen/** -- multiopen.cpp, run over ProofRun::multiopen_ctx()
// Host work is the transcript, the prover RNG's few hundred draws, query bookkeeping
// and O(#queries^2) interpolation; every length-n or extended-length operation is a
// kernel (MSM, NTT, prover_kernels.hip, poly.hip).  MSM results come back to the host
// (they enter the transcript), which is the only per-step synchronisation.
// ProofRun (proof_run.h) is the proof in flight; its stages are defined here, the lookup
// argument's permutation (LookupPermute) in prover_lookup.cpp.
#include "proof_run.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace {
std::vector<Fr> g_last_challenges;  // the challenges of the last proof (h2g_last_challenges)

// ------------------------------------------------------------------ host field helpers
Fr rotate_omega(const Domain& d, const Fr& x, int rot) {
  return x * pow_u64(rot >= 0 ? d.omega : d.omega_inv, (uint64_t)(rot >= 0 ? rot : -rot));
}

// the proof's upload staging (ProvingKey::up_h): armed behind a sync of the prover's
// stream, so no copy of the previous proof still reads it
int pk_upload_arm(ProvingKey& pk, hipStream_t st) {
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(pk.up_h.ensure(4u << 20));
  pk.up_off = 0;
  return H2G_OK;
}
}  // namespace

namespace h2g {
namespace prv {
std::vector<std::pair<const char*, double>> g_stages;
bool g_stage_sync = false;
// dst <- src (host, any) on st through the staging; past its end, the pageable copy
hipError_t pk_upload(ProvingKey& pk, void* dst, const void* src, size_t bytes, hipStream_t st) {
  const size_t a = (pk.up_off + 63) & ~(size_t)63;
  if (a + bytes <= pk.up_h.len) {
    std::memcpy(pk.up_h.p + a, src, bytes);
    pk.up_off = a + bytes;
    return hipMemcpyAsync(dst, pk.up_h.p + a, bytes, hipMemcpyHostToDevice, st);
  }
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
}
int copy_list_run(ProvingKey& pk, const std::vector<CopySeg>& segs, hipStream_t st) {
  if (segs.empty()) return H2G_OK;
  HIPCHK(pk.d_segs.ensure(segs.size()));
  uint64_t mx = 0;
  for (const CopySeg& g : segs) mx = std::max<uint64_t>(mx, g.len);
  HIPCHK(pk_upload(pk, pk.d_segs.p, segs.data(), segs.size() * sizeof(CopySeg), st));
  HIPCHK(copy_segments(pk.d_segs.p, (int)segs.size(), mx, st));
  return H2G_OK;
}
}  // namespace prv
}  // namespace h2g

// ------------------------------------------------------------------ create_proof
// h2g_create_proof_assigned: circuit ci's phase-ph numerators (w.wit_pin) and its Rational
// cells go up to the key's scratch and are evaluated there in place on the prover's stream
// (assigned.hip); the phase then reads the scratch as device advice
int ProofRun::assigned_convert(int ci, int ph, const std::vector<int>& cols, CircuitWs& w,
                               const h2g_assigned_dens& dn) {
  const size_t cells = (size_t)pk.cs.A * n;
  const std::string at = "circuit " + std::to_string(ci) + " phase " + std::to_string(ph);
  if (dn.count && (!dn.index || !dn.den))
    return fail(H2G_ERR_ARG, "create_proof_assigned: null denominator list at " + at);
  bool inside = true;  // every entry in one of this phase's columns (the usual case: no copy)
  for (size_t j = 0; j < dn.count; j++) {
    const uint64_t c = dn.index[j];
    if (c >= cells)
      return fail(H2G_ERR_ARG, "create_proof_assigned: index[" + std::to_string(j) + "] = " + std::to_string(c) +
                                   " is not below num_advice * n at " + at);
    if (j && c <= dn.index[j - 1])
      return fail(H2G_ERR_ARG, "create_proof_assigned: index[" + std::to_string(j) +
                                   "] does not exceed the entry before it (the list must be strictly increasing) at " + at);
    inside = inside && pk.cs.adv_phase[c >> pk.cs.k] == ph;  // n = 2^k
  }
  const uint64_t* idx = dn.index;
  const uint64_t* den = dn.den;
  size_t m = dn.count;
  if (!inside) {
    asg_idx_h.clear();
    asg_den_h.clear();
    for (size_t j = 0; j < dn.count; j++)
      if (pk.cs.adv_phase[dn.index[j] >> pk.cs.k] == ph) {
        asg_idx_h.push_back(dn.index[j]);
        asg_den_h.push_back(fr_from_limbs(dn.den + 4 * j));
      }
    idx = asg_idx_h.data();
    den = reinterpret_cast<const uint64_t*>(asg_den_h.data());
    m = asg_idx_h.size();
  }
  HIPCHK(pk.asg_num.ensure(cells));  // sizes first, then pointers (DevArr)
  HIPCHK(pk.asg_idx.ensure(m));
  HIPCHK(pk.asg_den.ensure(m));
  if (m) HIPCHK(d->work.ensure(m * sizeof(Fr) + 32));
  for (int c : cols)
    HIPCHK(hipMemcpyAsync(pk.asg_num.p + n * c, w.wit_pin + 4 * n * c, n * sizeof(Fr), hipMemcpyHostToDevice, st));
  if (m == 0) return H2G_OK;
  HIPCHK(hipMemcpyAsync(pk.asg_idx.p, idx, m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(pk.asg_den.p, den, m * sizeof(Fr), hipMemcpyHostToDevice, st));
  HIPCHK(pk.asg_ev.ensure());
  HIPCHK(hipEventRecord(pk.asg_ev, st));
  asg_pending = true;
  HIPCHK(assigned_to_fr(pk.asg_num.p, cells, pk.asg_idx.p, pk.asg_den.p, m, pk.asg_num.p, d->work.as<Fr>(), 0, st));
  return H2G_OK;
}

int ProofRun::launch_van_early() {
  // the vanishing argument's random polynomial does not depend on the witness: with the
  // seeded RNG its seeds are the keystream bytes at the position the last proof drew
  // them from, so it is generated and its commitment MSM launched early -- queued behind
  // phase 0's advice MSMs, it runs under the advice transforms and the lookup and
  // permutation products instead of between the product commitments and y; the
  // vanishing stage checks that the real draws equal these bytes (else it redoes both)
  van_seeds.assign(van_off.size() * 8, 0);
  rng.peek((uint64_t)pk.van_pos, reinterpret_cast<uint8_t*>(van_seeds.data()), van_seeds.size() * 4);
  HIPCHK(pk_upload(pk, pk.d_seeds.p, van_seeds.data(), van_seeds.size() * 4, st));
  HIPCHK(pk_upload(pk, pk.d_offsets.p, van_off.data(), van_off.size() * 8, st));
  HIPCHK(chacha_random_poly(pk.random_poly, n, pk.d_seeds.p, pk.d_offsets.p, (int)van_off.size(), st, sl.lo, sl.hi1));
  RCCHK(commit_launch(d, prm, pk.random_poly, n, SRS_G, st, &van_tk));
  van_early = true;
  return H2G_OK;
}

// ---- vk.hash_into + every circuit's instances (prover.rs:187-271; KZG: QUERY_INSTANCE = false)
int ProofRun::instances() {
  tr.common_scalar(pk.cs.transcript_repr);
  for (int ci = 0; ci < ncirc; ci++)
    for (int i = 0; i < pk.cs.I; i++) {
      const uint32_t len = in.inst_lens[ci][i];
      if ((size_t)len > n - (size_t)(bf + 1)) return fail(H2G_ERR_ARG, "create_proof: InstanceTooLarge");
      const uint64_t* col = in.instance[ci] + 4 * n * i;
      for (uint32_t r = 0; r < len; r++) tr.common_scalar(fr_from_limbs(col + 4 * r));
      HIPCHK(hipMemcpyAsync(W[ci]->inst_val[i], col, n * sizeof(Fr), hipMemcpyHostToDevice, st));
      if (!coef_recv) RCCHK(lagrange_to_coeff(d, D, W[ci]->inst_val[i], W[ci]->inst_poly[i], st));
    }
  return H2G_OK;
}

// ---- commit_phase per advice phase (prover.rs:309-494), circuit by circuit: the
// phase's blinding rows, its blinds, its commitments; then the phase's challenges
int ProofRun::advice_phases() {
  if (from_src)  // a witness source writes straight into pinned staging, one per circuit,
    for (CircuitWs* w : W) {  // allocated once (a pinned allocation costs more than the copies it speeds up)
      if (w->wit_pin) continue;
      const size_t bytes = (size_t)std::max(pk.cs.A, 1) * n * sizeof(Fr);
      if (hipHostMalloc((void**)&w->wit_pin, bytes, hipHostMallocDefault) == hipSuccess) {
        w->wit_pin_pinned = true;
      } else {  // pageable fallback: slower uploads, same bytes
        (void)hipGetLastError();
        w->wit_pin = static_cast<uint64_t*>(std::malloc(bytes));
        w->wit_pin_pinned = false;
        if (!w->wit_pin) return fail(H2G_ERR_NOMEM, "create_proof: witness staging allocation failed");
      }
    }
  HIPCHK(pk.d_seeds.ensure(van_off.size() * 8));
  HIPCHK(pk.d_offsets.ensure(van_off.size()));
  for (int ph = 0; ph <= pk.cs.max_phase; ph++) {
    if (ph == 0 && van_first) RCCHK(launch_van_early());
    std::vector<int> cols;
    for (int c = 0; c < pk.cs.A; c++)
      if (pk.cs.adv_phase[c] == ph) cols.push_back(c);
    if (from_src && ph > 0) HIPCHK(hipStreamSynchronize(st));  // the previous phase's uploads read the staging
    std::vector<MsmTicket> tk(cols.size() * ncirc);
    // a wide phase: column i (circuit-major) is rank i mod world's -- every rank uploads the
    // whole witness (the lookups and products read it), only the owner commits and
    // transforms the column
    const bool adv_wide = wide((int)(cols.size() * ncirc));
    const bool digest = g_spmd.world > 1 && !cols.empty();  // this phase's witness into the consistency digest
    if (digest) RCCHK(spmd_witness_prepare(pk, (int)(ncirc * cols.size()), st));
    for (int ci = 0; ci < ncirc; ci++) {
      CircuitWs& w = *W[ci];
      const uint64_t* from = in.advice ? in.advice[ci] : nullptr;
      bool from_dev = in.adv_dev;
      // copy_columns reads device advice in 16-byte chunks: refuse what it cannot
      if (from_dev && from && (reinterpret_cast<uintptr_t>(from) & 15) != 0)
        return fail(H2G_ERR_ARG, "create_proof: device advice must be 16-byte aligned");
      if (from_src) {
        // the staging outlives proofs: the unusable rows of unblinded columns start at zero
        // as the reference requires (prover.rs:417-421), whatever an earlier proof left there
        for (int c : cols)
          if (pk.unblinded[c]) std::memset(w.wit_pin + 4 * (n * c + unusable), 0, (n - unusable) * sizeof(Fr));
        const uint64_t* chp = reinterpret_cast<const uint64_t*>(challenges.data());
        h2g_assigned_dens dn = {nullptr, nullptr, 0};
        if (asg_pending) {  // the last list is the callback's again once its upload has been read
          HIPCHK(hipEventSynchronize(pk.asg_ev));
          asg_pending = false;
        }
        const int frc = in.asg   ? in.asg->fill(in.asg->ctx, (uint32_t)ci, (uint32_t)ph, chp, w.wit_pin, &dn)
                        : in.src ? in.src->fill(in.src->ctx, (uint32_t)ci, (uint32_t)ph, chp, w.wit_pin)
                                 : in.src1->fill(in.src1->ctx, (uint32_t)ph, chp, w.wit_pin);
        if (frc)
          return fail(H2G_ERR_ARG, "create_proof: witness source failed at " +
                                       (ncirc > 1 ? "circuit " + std::to_string(ci) + " " : std::string()) + "phase " +
                                       std::to_string(ph));
        from = w.wit_pin;
        from_dev = false;
        if (in.asg) {
          RCCHK(assigned_convert(ci, ph, cols, w, dn));
          from = reinterpret_cast<const uint64_t*>(pk.asg_num.p);
          from_dev = true;
        }
      }
      // column by column: upload, blinding rows, and (when the MSMs go one by one) the
      // commitment at once, so that a column's MSM overlaps the next column's upload
      // from host memory; the RNG draws keep the reference's order (every column's rows,
      // then every column's blind)
      const bool early = !adv_wide && commit_batch_chunk(prm, n, SRS_LAGRANGE) < 2;
      // device-resident columns come in through copy_columns (a streaming kernel, up to
      // COPY_COLS_MAX columns a launch; per-column DMA copies left the GPU idle for ~0.8 ms
      // of 32 columns at 2^18), host ones through the DMA upload; under SPMD either way
      // also takes each column's checksum before its blinding rows land (spmd_witness_fold)
      ColCopy cc{};
      int ncc = 0;
      auto flush = [&]() -> int {
        if (ncc) HIPCHK(copy_columns(cc, ncc, n, digest, st));
        ncc = 0;
        return H2G_OK;
      };
      Fr* const blind_rows = adv_blind.data() + (size_t)ci * pk.cs.A * (bf + 1);  // bf + 1 per column
      for (size_t k = 0; k < cols.size(); k++) {
        const int c = cols[k];
        const Fr* src = reinterpret_cast<const Fr*>(from + 4 * n * c);
        unsigned long long* sum = digest ? pk.wsum_d.p + (size_t)ci * cols.size() + k : nullptr;
        if (from_dev) {
          cc.src[ncc] = src;
          cc.dst[ncc] = w.adv[c];
          cc.sum[ncc++] = sum;
        } else {
          HIPCHK(hipMemcpyAsync(w.adv[c], src, n * sizeof(Fr), hipMemcpyHostToDevice, st));
          if (digest) {
            cc.src[ncc] = w.adv[c];
            cc.dst[ncc] = nullptr;
            cc.sum[ncc++] = sum;
          }
        }
        if (early || ncc == COPY_COLS_MAX || !from_dev) RCCHK(flush());
        if (early) {
          if (sc_mode) RCCHK(sc_unusable_rows(ci, {c}));
          if (!pk.unblinded[c]) {
            Fr* rows = blind_rows + (size_t)c * (bf + 1);
            draw_rows(rows, bf + 1);
            HIPCHK(pk_upload(pk, w.adv[c] + unusable, rows, (size_t)(bf + 1) * sizeof(Fr), st));
          }
          RCCHK(commit_launch(d, prm, w.adv[c], n, SRS_LAGRANGE, st, &tk[(size_t)ci * cols.size() + k]));
        }
      }
      RCCHK(flush());
      if (!early && sc_mode) RCCHK(sc_unusable_rows(ci, cols));
      if (!early) {  // every column's rows drawn in order, then one upload for the phase
        HIPCHK(pk.blind_d.ensure((size_t)pk.cs.A * (bf + 1)));
        std::vector<CopySeg> segs;
        for (int c : cols) {
          if (pk.unblinded[c]) continue;
          draw_rows(blind_rows + (size_t)c * (bf + 1), bf + 1);
          segs.push_back(CopySeg{pk.blind_d.p + (size_t)c * (bf + 1), w.adv[c] + unusable, (uint64_t)(bf + 1)});
        }
        RCCHK(upload_rows_batch(pk, blind_rows, (size_t)pk.cs.A * (bf + 1), segs, st));
      }
      for (int c : cols)
        if (!pk.unblinded[c]) (void)rng.random_fr();  // commitment blinds (unused by KZG)
      if (!cols.empty() && !early && !adv_wide) {
        Cols one;
        one.advice(w, cols);
        RCCHK(commit_stage(one.lag.data(), one.size(), nullptr, SRS_LAGRANGE, tk.data() + (size_t)ci * cols.size()));
      }
    }
    if (digest) RCCHK(spmd_witness_fold(pk, (int)(ncirc * cols.size()), st));
    // the phase's advice to coefficient form and its extended-domain cosets do not depend
    // on any challenge: queued behind the uploads, they run while the commitment MSMs
    // (their own streams) are in flight (lagrange_to_coeff, prover.rs:673-689; the
    // cosets of evaluation.rs:344-361)
    Cols adv;  // every circuit's columns of the phase
    for (CircuitWs* w : W) adv.advice(*w, cols);
    if (adv_wide) {
      std::vector<int> adv_owner(adv.size());
      for (int i = 0; i < adv.size(); i++) adv_owner[i] = i % Wsp;
      RCCHK(commit_stage(adv.lag.data(), adv.size(), &adv_owner, SRS_LAGRANGE, tk.data()));
      RCCHK(xform(adv, &adv_owner));
      for (int ci = 0; ci < ncirc; ci++)
        for (int c : cols) adv_shard[(size_t)ci * pk.cs.A + c] = 1;
    } else if (pieces && !cols.empty()) {  // one owner per column, every circuit's
      if (defer_adv) xform_later(adv);
      else RCCHK(xform(adv, nullptr));
    } else if (!cols.empty()) {  // a batch per circuit
      for (CircuitWs* w : W) {
        Cols one;
        one.advice(*w, cols);
        RCCHK(xform(one, nullptr));
      }
    }
    if (ph == 0 && early_van && !van_first) RCCHK(launch_van_early());
    if (ph == 0) clk.mark("upload+instances");
    RCCHK(collect_write({&tk}));  // circuit by circuit, column by column
    RCCHK(rng_ok());
    for (int i = 0; i < NCH; i++)
      if (pk.cs.ch_phase[i] == ph) challenges[i] = tr.squeeze();
  }
  if (NCH)
    HIPCHK(pk_upload(pk, pk.consts + pk.num_consts, challenges.data(), NCH * sizeof(Fr), st));
  g_last_challenges = challenges;
  clk.mark("advice commit");
  return H2G_OK;
}

// ---- lookup_commit_permuted, per circuit, per lookup (lookup/prover.rs:64-173): A'_l and
// S'_l of every lookup (LookupPermute), then the bf + 1 random rows of each (input first,
// then table), their commitments and transforms
int ProofRun::lookup_permuted() {
  ch.theta = tr.squeeze();
  const bool lk_wide = wide(NLT);
  LookupPermute lp(*this, lk_wide);
  RCCHK(lp.plan());
  RCCHK(lp.compress());
  std::vector<Fr> rows((size_t)NLT * 2 * (bf + 1));  // host staging: lives until the commitments are collected
  for (int j = 0; j < NLT; j++) {
    draw_rows(rows.data() + (size_t)2 * j * (bf + 1), 2 * (bf + 1));  // A'_j's rows, then S'_j's
    (void)rng.random_fr();  // permuted input blind
    (void)rng.random_fr();  // permuted table blind
  }
  RCCHK(lp.key_and_sort());
  RCCHK(lp.match_all());
  RCCHK(lp.check_and_redo());
  RCCHK(lp.rows_upload(rows));
  bool lk_ok = lp.matched();
  if (lk_wide) {  // every rank learns whether any owner's lookup failed (none may hang in a collective)
    std::vector<Fr> mine(1, lk_ok ? Fr::zero() : Fr::one()), all;
    RCCHK(spmd_allgather_fr(mine, &all));
    for (const Fr& f : all) lk_ok = lk_ok && f.is_zero();
  }
  if (!lk_ok) return fail(H2G_ERR_ARG, "create_proof: lookup input value not in the table (ConstraintSystemFailure)");
  RCCHK(sc_lookup_permuted());
  Cols perm;  // (A'_l, S'_l) in transcript order
  for (CircuitWs* w : W) perm.lookup_permuted(*w);
  std::vector<int> own2(2 * NLT);
  for (int j = 0; j < NLT; j++) own2[2 * j] = own2[2 * j + 1] = lk_wide ? lk_owner_all[j] : g_spmd.rank;
  // A', S' against the prefix-summed Lagrange basis (params_prefix): the same commitments
  std::vector<const Fr*> com_cols = perm.lag;
  RCCHK(params_prefix(prm, st));
  // scalars only for the columns this rank commits (all of them but in a wide stage,
  // where a column belongs to its owner and the others' are not read here)
  size_t owned = 0;
  for (int i = 0; i < 2 * NLT; i++) owned += own2[i] == g_spmd.rank;
  HIPCHK(pk.lk_diff.ensure(std::max<size_t>(owned, 1) * n));
  PrefixDiff pd{};
  int m = 0;
  size_t slot = 0;
  for (int i = 0; i < 2 * NLT; i++) {
    if (own2[i] != g_spmd.rank) continue;
    Fr* e = pk.lk_diff.p + (slot++) * n;
    com_cols[i] = e;
    pd.a[m] = perm.lag[i];
    pd.e[m] = e;
    if (++m == PREFIX_DIFF_MAX) {
      HIPCHK(prefix_diff(pd, m, n, st));
      m = 0;
    }
  }
  if (m) HIPCHK(prefix_diff(pd, m, n, st));
  // coefficient forms and cosets, batched transforms (they overlap the commitments)
  std::vector<MsmTicket> tk(2 * NLT);
  RCCHK(commit_stage(com_cols.data(), 2 * NLT, lk_wide ? &own2 : nullptr, SRS_LAGRANGE_PREFIX, tk.data()));
  RCCHK(xform(perm, lk_wide ? &own2 : nullptr));
  lk_shard = lk_wide;
  RCCHK(collect_write({&tk}));
  RCCHK(rng_ok());
  if (pk.cs.NL) clk.mark("lookup permuted");
  return H2G_OK;
}

// ---- permutation_commit per circuit (permutation/prover.rs:50-197); commitments are
// written after the loop (nothing is squeezed in between, so the transcript is unchanged)
int ProofRun::permutation_products() {
  ch.beta = tr.squeeze(), ch.gamma = tr.squeeze();
  dump("beta", &beta, 1, st, true);
  dump("gamma", &gamma, 1, st, true);
  // large MSMs start as soon as their set's z is ready; small ones wait and go as a batch
  const bool perm_batched = commit_batch_chunk(prm, n, SRS_LAGRANGE) > 1;
  for (CircuitWs* w : W) all_z.z(*w);
  // with row pieces the grand products go by slabs: each rank forms its MSM slab's rows of
  // every set (denominators, inversion, numerators, a slab-local running product), one host
  // all-gather of the slabs' products chains the slabs and the sets (z_0 of set s + 1 is
  // set s's last product row), the commitments take the slabs, and each set's transform
  // owner gathers the whole column.  Otherwise every rank forms the whole columns
  const bool perm_slab = pieces && NST > 0;
  const int me = g_spmd.rank;
  const size_t plo = perm_slab ? shard_lo(prm.n, n, Wsp, me) : 0, phi = perm_slab ? shard_lo(prm.n, n, Wsp, me + 1) : n;
  const size_t len = phi - plo;
  std::vector<Fr*> zlag, zl(NST), zs(NST);  // every set's z_lag; z_lag and z from row plo
  for (CircuitWs* w : W) zlag.insert(zlag.end(), w->z_lag.begin(), w->z_lag.end());
  for (int i = 0; i < NST; i++) {
    zl[i] = zlag[i] + plo;
    zs[i] = all_z.pol[i] + plo;
  }
  // every set's denominators (into z_lag), one batched inversion over all circuits' sets
  // (z as its scratch until the iNTT fills it)
  for (int i = 0; i < NST; i++) RCCHK(perm_set(i, false, zl[i], plo, len));
  if (NST) dump("den0", zl[0], len, st);
  if (len) HIPCHK(poly_batch_invert_multi(zl.data(), zs.data(), NST, len, st));
  if (NST) dump("inv0", zl[0], len, st);
  if (perm_slab) {
    for (int i = 0; i < NST; i++) RCCHK(perm_set(i, true, zl[i], plo, len));
    if (len)
      HIPCHK(poly_prefix_product_multi((const Fr* const*)zl.data(), zs.data(), NST, len, pk.scr, pk.scr_len, st));
    // the slab's product of the rows that feed z (factors below n - bf - 1)
    const size_t hc = std::min(phi, n - (size_t)bf - 1);
    std::vector<Fr> tp(NST, Fr::one());
    if (hc > plo)
      for (int i = 0; i < NST; i++)
        HIPCHK(hipMemcpyAsync(&tp[i], all_z.pol[i] + hc - 1, sizeof(Fr), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<Fr> allp;
    RCCHK(spmd_allgather_fr(tp, &allp));
    std::vector<Fr> lzp(NST);  // z at this slab's first row = z_0 * (the slabs below)
    for (int ci = 0; ci < ncirc; ci++) {
      Fr lz = Fr::one();
      for (int s = 0; s < pk.cs.nsets; s++) {
        const int i = ci * pk.cs.nsets + s;
        Fr below = Fr::one(), all = Fr::one();
        for (int r = 0; r < Wsp; r++) {
          if (r < me) below = below * allp[(size_t)r * NST + i];
          all = all * allp[(size_t)r * NST + i];
        }
        lzp[i] = lz * below;
        lz = lz * all;
      }
    }
    HIPCHK(pk.perm_lz.ensure(std::max(NST, 1)));
    HIPCHK(pk_upload(pk, pk.perm_lz.p, lzp.data(), NST * sizeof(Fr), st));
    for (int i = 0; i < NST; i++) {
      Fr* blind_rows = perm_blind.data() + (size_t)i * bf;
      draw_rows(blind_rows, bf);
      (void)rng.random_fr();  // blind
      HIPCHK(pk_upload(pk, pk.small, blind_rows, bf * sizeof(Fr), st));
      HIPCHK(perm_z_assemble(zlag[i], n, bf, all_z.pol[i], pk.perm_lz.p + i, pk.small, st, plo, phi));
    }
    HIPCHK(hipStreamSynchronize(st));  // lzp (host) was read
    RCCHK(commit_stage(all_z.lag.data(), NST, nullptr, SRS_LAGRANGE, perm_tk.data()));
    // each set's owner gathers its column, then transforms and distributes it
    const std::vector<int> own = next_owners(NST);
    RCCHK(gather_to_owners(pk, zlag, own, prm.n, st));
    RCCHK(xform(all_z, &own));
    RCCHK(run_deferred());  // the advice columns' transforms beside the products
  } else {
    // per set numerators, scan and z
    // (every set's numerators, then one batched scan of all sets: measured, rejected)
    for (int ci = 0; ci < ncirc; ci++) {
      CircuitWs& w = *W[ci];
      HIPCHK(hipMemcpyAsync(pk.last_z, pk.one, sizeof(Fr), hipMemcpyDeviceToDevice, st));  // z_0 starts at one
      for (int s = 0; s < pk.cs.nsets; s++) {
        const int i = ci * pk.cs.nsets + s;
        Fr* blind_rows = perm_blind.data() + (size_t)i * bf;
        Fr* prod = w.z_lag[s];
        RCCHK(perm_set(i, true, prod, 0, n));
        // z = last_z * running product, blinding rows from the rng
        if (ci == 0 && s == 0) dump("mod0", prod, n, st);
        HIPCHK(poly_prefix_product(prod, pk.pre, n, pk.scr, pk.scr_len, st));
        if (ci == 0 && s == 0) dump("pre0", pk.pre, n, st);
        draw_rows(blind_rows, bf);
        (void)rng.random_fr();  // blind
        HIPCHK(pk_upload(pk, pk.small, blind_rows, bf * sizeof(Fr), st));
        HIPCHK(perm_z_assemble(w.z_lag[s], n, bf, pk.pre, pk.last_z, pk.small, st));
        HIPCHK(hipMemcpyAsync(pk.last_z, w.z_lag[s] + (n - (size_t)(bf + 1)), sizeof(Fr), hipMemcpyDeviceToDevice,
                              st));
        RCCHK(sc_permutation(i));
        if (ci == 0 && s == 0) {
          dump("z0", w.z_lag[s], n, st);
          dump("sigma0", pk.sigma_lag[0], n, st);
          dump("v0", col_vals(w, 0), n, st);
        }
        if (!perm_batched)
          RCCHK(commit_launch(d, prm, w.z_lag[s], n, SRS_LAGRANGE, st, &perm_tk[i]));
      }
    }
    RCCHK(xform(all_z, nullptr));
    if (perm_batched) RCCHK(commit_stage(all_z.lag.data(), NST, nullptr, SRS_LAGRANGE, perm_tk.data()));
  }
  clk.mark("permutation products");
  return H2G_OK;
}

// ---- lookup products (lookup/prover.rs:182-325), every circuit's, then shuffle
// products (shuffle/prover.rs:97-206): z = [1, running product ...], bf random rows, blind
int ProofRun::lookup_shuffle_products() {
  // a wide lookup stage keeps its owners here: lookup j's product is rank j mod world's
  // (the permuted columns are already there); the others only make the RNG draws
  const bool lz_wide = lk_shard;
  auto mine = [&](int j) { return lk_owner_all[j] == g_spmd.rank; };
  // every product's random rows and blind, drawn up front in the products' order (no
  // other draws come between them) and uploaded once
  const size_t nprod = (size_t)NLT + (size_t)NSH;
  for (size_t z = 0; z < nprod; z++) {
    draw_rows(prod_blind.data() + z * (size_t)bf, bf);
    (void)rng.random_fr();  // product blind
  }
  if (nprod) {
    HIPCHK(pk.blind_d.ensure(nprod * (size_t)bf));
    HIPCHK(pk_upload(pk, pk.blind_d.p, prod_blind.data(), nprod * (size_t)bf * sizeof(Fr), st));
  }
  // the products this rank assembles here whose transforms are not their owners' (below):
  // prod: the running product's factors, or (scanned) already its prefix products
  Cols zc;
  size_t zrow = 0;
  auto finish_z = [&](const Fr* prod, Fr* z_lag, Fr* z_poly, Fr* z_coset, bool scanned, bool here,
                      bool listed) -> int {
    const Fr* rows_d = pk.blind_d.p + (zrow++) * (size_t)bf;
    if (!here) return H2G_OK;
    const Fr* pre = prod;
    if (!scanned) {
      HIPCHK(poly_prefix_product(prod, pk.pre, n, pk.scr, pk.scr_len, st));
      pre = pk.pre;
    }
    HIPCHK(perm_z_assemble(z_lag, n, bf, pre, pk.one, rows_d, st));
    if (listed) zc.add(z_lag, z_poly, z_coset);
    return H2G_OK;
  };
  // every lookup's denominators go through one batched inversion (the per-thread
  // inversion's latency is paid once); z_poly holds the product until its iNTT,
  // z_lag serves as the inversion's scratch until z is assembled into it
  std::vector<Fr*> dens, dens_scr;
  for (int ci = 0, j = 0; ci < ncirc; ci++)
    for (int l = 0; l < pk.cs.NL; l++, j++) {
      if (!mine(j)) continue;
      CircuitWs* w = W[ci];
      HIPCHK(lookup_prod_den(w->lk_ap[l], w->lk_sp[l], beta, gamma, w->lk_z_poly[l], n, st));
      dens.push_back(w->lk_z_poly[l]);
      dens_scr.push_back(w->lk_z[l]);
    }
  if (!dens.empty()) HIPCHK(poly_batch_invert_multi(dens.data(), dens_scr.data(), (int)dens.size(), n, st));
  // numerators, then every lookup's running product in one batched scan (in place)
  for (int ci = 0, j = 0; ci < ncirc; ci++)
    for (int l = 0; l < pk.cs.NL; l++, j++)
      if (mine(j)) HIPCHK(lookup_prod_num(W[ci]->lk_a[l], W[ci]->lk_s[l], beta, gamma, W[ci]->lk_z_poly[l], n, st));
  if (!dens.empty())
    HIPCHK(poly_prefix_product_multi((const Fr* const*)dens.data(), dens.data(), (int)dens.size(), n, pk.scr,
                                     pk.scr_len, st));
  for (int ci = 0, j = 0; ci < ncirc; ci++)
    for (int l = 0; l < pk.cs.NL; l++, j++) {
      CircuitWs* w = W[ci];
      RCCHK(finish_z(w->lk_z_poly[l], w->lk_z[l], w->lk_z_poly[l], w->lk_zc[l], true, mine(j), !lz_wide));
      RCCHK(sc_product(ci, (uint32_t)l, w->lk_z[l], w->lk_a[l], w->lk_s[l], w->lk_ap[l], w->lk_sp[l]));
    }
  for (int ci = 0; ci < ncirc; ci++)
    for (int s = 0; s < pk.cs.NS; s++) {
      CircuitWs* w = W[ci];
      RCCHK(compress(*w, pk.seg_sh_in[s], pk.tmp_a));
      RCCHK(compress(*w, pk.seg_sh_sh[s], pk.tmp_b));
      HIPCHK(shuffle_prod_den(pk.tmp_b, gamma, pk.mod, n, st));
      HIPCHK(poly_batch_invert(pk.mod, n, pk.scr, st));
      HIPCHK(shuffle_prod_num(pk.tmp_a, gamma, pk.mod, n, st));
      RCCHK(finish_z(pk.mod, w->sh_z[s], w->sh_z_poly[s], w->sh_zc[s], false, true, true));
      RCCHK(sc_product(ci, (uint32_t)(pk.cs.NL + s), w->sh_z[s], pk.tmp_a, nullptr, pk.tmp_b, nullptr));
    }
  RCCHK(xform(zc, nullptr));
  // product commitments: every circuit's lookups, then every circuit's shuffles
  std::vector<const Fr*> zs;
  for (CircuitWs* w : W) zs.insert(zs.end(), w->lk_z.begin(), w->lk_z.end());
  for (CircuitWs* w : W) zs.insert(zs.end(), w->sh_z.begin(), w->sh_z.end());
  std::vector<MsmTicket> zt(zs.size());
  if (lz_wide) {
    Cols lkz;
    for (CircuitWs* w : W) lkz.lookup_z(*w);
    RCCHK(commit_stage(zs.data(), NLT, &lk_owner_all, SRS_LAGRANGE, zt.data()));
    if (NSH) RCCHK(commit_stage(zs.data() + NLT, NSH, nullptr, SRS_LAGRANGE, zt.data() + NLT));
    RCCHK(xform(lkz, &lk_owner_all));
  } else if (!zs.empty()) {
    RCCHK(commit_stage(zs.data(), (int)zs.size(), nullptr, SRS_LAGRANGE, zt.data()));
  }
  for (int j = 0; j < NLT; j++) lkz_tk[j] = zt[j];
  for (int j = 0; j < NSH; j++) shz_tk[j] = zt[NLT + j];
  if (pk.cs.NL + pk.cs.NS) clk.mark("lookup/shuffle products");
  return H2G_OK;
}

// ---- vanishing commit (vanishing/prover.rs:40-98), through the y squeeze
int ProofRun::vanishing_commit() {
  {
    const uint64_t at = rng.position();
    std::vector<uint32_t> drawn(van_off.size() * 8, 0);
    for (size_t i = 0; i < van_off.size(); i++) rng.fill(reinterpret_cast<uint8_t*>(&drawn[8 * i]), 32);
    if (van_early && (at != (uint64_t)pk.van_pos || drawn != van_seeds)) {
      // the early draws were not the real ones: drop that commitment, redo it below
      G1Affine unused;
      RCCHK(commit_collect(d, &van_tk, &unused));
      van_early = false;
    }
    if (rng.seeded()) {
      pk.van_pos = (int64_t)at;
      pk.van_T = (uint32_t)van_off.size();
    }
    if (!van_early) {
      van_seeds = drawn;
      HIPCHK(pk_upload(pk, pk.d_seeds.p, van_seeds.data(), van_seeds.size() * 4, st));
      HIPCHK(pk_upload(pk, pk.d_offsets.p, van_off.data(), van_off.size() * 8, st));
      // a slab-mode rank draws only its coefficients (and the halo) of the random polynomial
      HIPCHK(chacha_random_poly(pk.random_poly, n, pk.d_seeds.p, pk.d_offsets.p, (int)van_off.size(), st, sl.lo,
                                sl.hi1));
    }
    (void)rng.random_fr();  // random_blind
    RCCHK(rng_ok());
    if (!van_early) RCCHK(commit_launch(d, prm, pk.random_poly, n, SRS_G, st, &van_tk));
  }
  // the instance columns' cosets do not depend on y: they overlap the permutation /
  // vanishing MSMs (the advice went to coefficients and cosets under its own MSMs)
  for (CircuitWs* w : W)
    RCCHK(ext_cosets(d, pk, (const Fr* const*)w->inst_poly.data(), w->inst_coset.data(), pk.cs.I, st));
  RCCHK(collect_write({&perm_tk, &lkz_tk, &shz_tk}, &van_tk));
  RCCHK(run_deferred());  // (no permutation stage ran them)
  RCCHK(xp_flush(pk, st));  // the overlapped exchanges' rows, before h(X) reads them
  clk.mark("perm+vanishing commits, cosets");
  HIPCHK(xjoin.join());  // the columns' cosets and coefficients (the transform stream)
  ch.y = tr.squeeze();
  return H2G_OK;
}

// ---- evaluate_h (evaluation.rs:317-620): one launch per circuit, each continuing the
// previous circuit's Horner chain in y; the last one divides by t(X)
int ProofRun::eval_h() {
  const bool subc = spmd_subcosets();
  if (pk.cosets) return eval_h_streamed();
  for (int ci = 0; ci < ncirc && !subc; ci++) {
    EvalHArgs a = eval_h_args(ci, W[ci]->whole(), pk.d_sigma, pk.l0, pk.l_last, pk.l_active);
    a.delta_start = beta * zeta();
    a.ext_omega = pk.eo;
    a.ext = ext;
    a.rot_scale = pk.rot_scale;
    a.t_evals = D.d_t.p;
    a.t_mask = D.t_evals.size() - 1;
    a.acc_in = ci > 0 ? pk.h_ext : nullptr;
    a.out = pk.h_ext;
    HIPCHK(evaluate_h(a, st));
  }
  if (subc) {  // rows of this rank's sub-cosets, then every sub-coset's h from its owner
    const int e = (int)(D.ek - D.k);
    for (CircuitWs* w : W) RCCHK(sub_ws_tables(pk, *w));
    for (size_t i = 0; i < pk.sub_ts.size(); i++) {
      const uint64_t t = pk.sub_ts[i];
      for (int ci = 0; ci < ncirc; ci++) {  // (with row pieces: this rank's rows of the sub-coset)
        const EvalHArgs a = eval_h_sub(ci, t, pk.h_gather + t * n, W[ci]->sub[i], pk.d_sigma_sub[i], pk.sub_l0 + i * n,
                                       pk.sub_ll + i * n, pk.sub_la + i * n, pieces);
        HIPCHK(evaluate_h(a, st));
      }
    }
    if (h_slabs) {
      if (pieces) RCCHK(h_gather_pieces(pk, st));
      RCCHK(h_by_slabs(d, pk, sl, st));
    } else {
      HIPCHK(hipStreamSynchronize(st));
      for (uint64_t t = 0; t < (1ull << e); t++)
        if (spmd_timed(3, n * sizeof(Fr), [&] {
              return g_spmd.bcast(g_spmd.ctx, pk.h_gather + t * n, n * sizeof(Fr), (int)(t % (uint64_t)g_spmd.world));
            }) != 0)
          return fail(H2G_ERR_STATE, "spmd transport: broadcast of sub-coset " + std::to_string(t) + " failed");
      HIPCHK(subcoset_scatter(pk.h_gather, pk.h_ext, n, e, st));
    }
  }
  if (!h_slabs) dump("h_ext", pk.h_ext, ext, st);
  clk.mark("evaluate_h");
  return H2G_OK;
}

// A streamed key (ProvingKey::cosets): the same evaluation sub-coset by sub-coset.  Row
// t + 2^e m of the extended coset is the point zeta w_ext^t w^m and rotations move rows by
// multiples of 2^e, so evaluate_h on sub-coset t reads sub-coset t of every column -- the
// arguments the SPMD split passes -- and every column array is one n-point slot, refilled for
// each t from its coefficient form: the key's columns once per t for all circuits, then
// circuit by circuit (the slots are shared, so a circuit's transforms follow the previous
// circuit's launch).  All on the prover's stream, one slot set: the transforms and the
// launches alternate, each filling the chip on its own (DESIGN, "Streamed cosets").
int ProofRun::eval_h_streamed() {
  const int e = (int)(D.ek - D.k);
  const Fr one = Fr::one();
  std::vector<const Fr*> ksrc;
  std::vector<Fr*> kdst;
  for (int i = 0; i < pk.cs.F; i++) ksrc.push_back(pk.fixed_poly[i]), kdst.push_back(pk.fixed_coset[i]);
  for (int i = 0; i < pk.cs.P; i++) ksrc.push_back(pk.sigma_poly[i]), kdst.push_back(pk.sigma_coset[i]);
  ksrc.push_back(pk.l0_poly), kdst.push_back(pk.l0);
  ksrc.push_back(pk.l_last_poly), kdst.push_back(pk.l_last);
  ksrc.push_back(pk.l_blind_poly), kdst.push_back(pk.l_active);  // l_blind, then 1 - l_last - l_blind in place
  std::vector<Cols> cc(ncirc);  // per circuit every column: pol -> its slot cst
  for (int ci = 0; ci < ncirc; ci++) {
    const CircuitWs& w = *W[ci];
    cc[ci].add(w.adv, w.adv_poly, w.adv_coset);
    cc[ci].add(w.inst_val, w.inst_poly, w.inst_coset);
    cc[ci].z(w);
    cc[ci].add(w.lk_ap, w.lk_ap_poly, w.lk_apc);
    cc[ci].add(w.lk_sp, w.lk_sp_poly, w.lk_spc);
    cc[ci].lookup_z(w);
    cc[ci].add(w.sh_z, w.sh_z_poly, w.sh_zc);
  }
  for (uint64_t t = 0; t < (1ull << e); t++) {
    RCCHK(coeff_to_subcoset_batch(d, D, ksrc.data(), kdst.data(), (int)ksrc.size(), t, st));
    HIPCHK(poly_binop(POLY_ADD, pk.l_last, pk.l_active, one, pk.l_active, n, st));
    HIPCHK(poly_binop(POLY_SUB_CONST, pk.l_active, nullptr, one, pk.l_active, n, st));
    HIPCHK(poly_binop(POLY_SCALE, pk.l_active, nullptr, fr_neg_one(), pk.l_active, n, st));
    for (int ci = 0; ci < ncirc; ci++) {
      RCCHK(coeff_to_subcoset_batch(d, D, (const Fr* const*)cc[ci].pol.data(), cc[ci].cst.data(), cc[ci].size(), t, st));
      // the tables of circuit_ws_add: their columns are the slots
      const EvalHArgs a = eval_h_sub(ci, t, pk.h_gather + t * n, W[ci]->whole(), pk.d_sigma, pk.l0, pk.l_last,
                                     pk.l_active, false);
      HIPCHK(evaluate_h(a, st));
    }
  }
  HIPCHK(subcoset_scatter(pk.h_gather, pk.h_ext, n, e, st));
  dump("h_ext", pk.h_ext, ext, st);
  clk.mark("evaluate_h");
  return H2G_OK;
}

// ---- vanishing construct (vanishing/prover.rs:102-155): h(X) pieces of size n (a rank
// that received h by slabs holds its slab of each piece already)
int ProofRun::h_commit() {
  if (!h_slabs) RCCHK(extended_to_coeff(d, D, pk.h_ext, pk.h_coeff, st));
  const int npieces = pk.cs.degree - 1;
  for (int p = 0; p < npieces; p++) (void)rng.random_fr();  // h blinds
  RCCHK(rng_ok());
  {
    std::vector<MsmTicket> tk(npieces);
    std::vector<const Fr*> h_pieces(npieces);
    for (int p = 0; p < npieces; p++) h_pieces[p] = pk.h_coeff + (size_t)p * n;
    RCCHK(commit_stage(h_pieces.data(), npieces, nullptr, SRS_G, tk.data()));
    RCCHK(collect_write({&tk}));
  }
  clk.mark("h commit");
  ch.x = tr.squeeze();
  const Fr xn = pow_u64(x, n);
  // h(X) = sum_p X^(n p) h_p(X)  (vanishing/prover.rs:166-170)
  {
    LinTerms t;
    Fr c = Fr::one();
    bool first = true;
    for (int p = 0; p < npieces; p++) {
      if (t.k == LIN_MAXT) {
        RCCHK(lincomb_range(pk.h_poly, sl.lo, sl.hi1, t, !first, st));  // a slab rank: its slab + halo
        first = false;
        t.k = 0;
      }
      t.p[t.k] = pk.h_coeff + (size_t)p * n;
      t.len[t.k] = n;
      t.coef[t.k] = c;
      t.k++;
      c = c * xn;
    }
    RCCHK(lincomb_range(pk.h_poly, sl.lo, sl.hi1, t, !first, st));
  }
  return H2G_OK;
}

// ---- the polynomial openings (prover.rs:840-889) and their evaluations
int ProofRun::openings_and_evals() {
  for (const CircuitWs* w : W) {
    for (int c = 0; c < pk.cs.A; c++) polys.push_back({w->adv_poly[c], n});
    for (int s = 0; s < pk.cs.nsets; s++) polys.push_back({w->z[s], n});
    for (int l = 0; l < pk.cs.NL; l++) {
      polys.push_back({w->lk_z_poly[l], n});
      polys.push_back({w->lk_ap_poly[l], n});
      polys.push_back({w->lk_sp_poly[l], n});
    }
    for (int s = 0; s < pk.cs.NS; s++) polys.push_back({w->sh_z_poly[s], n});
  }
  const int id_fix = (int)polys.size();
  if (coef_send || coef_recv) {  // the per-circuit coefficient columns' slabs, owners -> the others
    std::vector<Fr*> cols;     // (the columns of wide stages reached every rank from their owners)
    for (int ci = 0; ci < ncirc; ci++)
      for (int i = 0; i < per_c; i++) {
        if (i < pk.cs.A && adv_shard[(size_t)ci * pk.cs.A + i]) continue;
        if (lk_shard && i >= pk.cs.A + pk.cs.nsets && i < pk.cs.A + pk.cs.nsets + 3 * pk.cs.NL) continue;
        cols.push_back(const_cast<Fr*>(polys[(size_t)ci * per_c + i].p));
      }
    RCCHK(coef_exchange(pk, cols, st));
  }
  for (int c = 0; c < pk.cs.F; c++) polys.push_back({pk.fixed_poly[c], n});
  const int id_sig = (int)polys.size();
  for (int c = 0; c < pk.cs.P; c++) polys.push_back({pk.sigma_poly[c], n});
  const int id_h = (int)polys.size();
  polys.push_back({pk.h_poly, n});
  const int id_r = (int)polys.size();
  polys.push_back({pk.random_poly, n});
  const Fr x_next = rotate_omega(D, x, 1), x_last = rotate_omega(D, x, -(bf + 1));
  const Fr x_prev = rotate_omega(D, x, -1);
  for (int ci = 0; ci < ncirc; ci++) {  // per circuit: advice, permutation, lookups, shuffles
    for (auto& q : pk.cs.adv_q) queries.push_back({id_adv(ci) + q.index, rotate_omega(D, x, q.rot)});
    for (int s = 0; s < pk.cs.nsets; s++) {  // permutation/prover.rs:300-333
      queries.push_back({id_z(ci) + s, x});
      queries.push_back({id_z(ci) + s, x_next});
    }
    for (int s = pk.cs.nsets - 2; s >= 0; s--) queries.push_back({id_z(ci) + s, x_last});
    for (int l = 0; l < pk.cs.NL; l++) {  // lookup/prover.rs:364-405
      const int zi = id_lk(ci) + 3 * l;
      queries.push_back({zi, x});
      queries.push_back({zi + 1, x});
      queries.push_back({zi + 2, x});
      queries.push_back({zi + 1, x_prev});
      queries.push_back({zi, x_next});
    }
    for (int s = 0; s < pk.cs.NS; s++) {  // shuffle/prover.rs:234-254
      queries.push_back({id_sh(ci) + s, x});
      queries.push_back({id_sh(ci) + s, x_next});
    }
  }
  for (auto& q : pk.cs.fix_q) queries.push_back({id_fix + q.index, rotate_omega(D, x, q.rot)});
  for (int c = 0; c < pk.cs.P; c++) queries.push_back({id_sig + c, x});
  queries.push_back({id_h, x});
  queries.push_back({id_r, x});
  ev_of.resize(polys.size());
  for (auto& q : queries) ev_index(q.poly, q.pt);
  evals.resize(ev_keys.size());
  {
    const int nreq = (int)ev_keys.size();
    HIPCHK(pk.d_reqs.ensure(nreq));
    HIPCHK(pk.evals.ensure(nreq));
    HIPCHK(pk.eval_scr.ensure(poly_eval_scratch_len(nreq, n)));
    std::vector<EvalReq> reqs(nreq);
    for (int i = 0; i < nreq; i++) {  // a slab rank evaluates its coefficients [lo, hi) only
      const PolyRef& pr = polys[ev_keys[i].poly];
      const uint64_t len = pr.len > sl.lo ? std::min<uint64_t>(pr.len, sl.hi) - sl.lo : 0;
      reqs[i] = EvalReq{pr.p + (len ? sl.lo : 0), len, ev_keys[i].pt};
    }
    HIPCHK(pk_upload(pk, pk.d_reqs.p, reqs.data(), nreq * sizeof(EvalReq), st));
    HIPCHK(poly_eval_batch(pk.d_reqs.p, nreq, sl.hi - sl.lo, pk.evals.p, pk.eval_scr.p, st));
    HIPCHK(hipMemcpyAsync(evals.data(), pk.evals.p, nreq * sizeof(Fr), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (slabs) {  // p(x) = sum_r x^lo_r (slab r's partial evaluation), summed in rank order
      std::vector<std::pair<Fr, Fr>> shift;  // (point, point^lo): a few distinct points
      for (int i = 0; i < nreq; i++) {
        const Fr& pt = ev_keys[i].pt;
        size_t j = 0;
        while (j < shift.size() && !(shift[j].first == pt)) j++;
        if (j == shift.size()) shift.emplace_back(pt, pow_u64(pt, sl.lo));
        evals[i] = evals[i] * shift[j].second;
      }
      std::vector<Fr> all;
      RCCHK(spmd_allgather_fr(evals, &all));
      for (int i = 0; i < nreq; i++) {
        Fr acc = Fr::zero();
        for (int r = 0; r < g_spmd.world; r++) acc = acc + all[(size_t)r * nreq + i];
        evals[i] = acc;
      }
    }
  }
  for (int ci = 0; ci < ncirc; ci++)  // [TRANSCRIPT-17] every circuit's advice evaluations
    for (auto& q : pk.cs.adv_q) tr.write_scalar(ev(id_adv(ci) + q.index, rotate_omega(D, x, q.rot)));
  for (auto& q : pk.cs.fix_q) tr.write_scalar(ev(id_fix + q.index, rotate_omega(D, x, q.rot)));
  tr.write_scalar(ev(id_r, x));
  for (int c = 0; c < pk.cs.P; c++) tr.write_scalar(ev(id_sig + c, x));
  for (int ci = 0; ci < ncirc; ci++)
    for (int s = 0; s < pk.cs.nsets; s++) {
      tr.write_scalar(ev(id_z(ci) + s, x));
      tr.write_scalar(ev(id_z(ci) + s, x_next));
      if (s + 1 < pk.cs.nsets) tr.write_scalar(ev(id_z(ci) + s, x_last));
    }
  for (int ci = 0; ci < ncirc; ci++)
    for (int l = 0; l < pk.cs.NL; l++) {  // product, product_next, A', A'_inv, S' (lookup/prover.rs:330-361)
      const int zi = id_lk(ci) + 3 * l;
      tr.write_scalar(ev(zi, x));
      tr.write_scalar(ev(zi, x_next));
      tr.write_scalar(ev(zi + 1, x));
      tr.write_scalar(ev(zi + 1, x_prev));
      tr.write_scalar(ev(zi + 2, x));
    }
  for (int ci = 0; ci < ncirc; ci++)
    for (int s = 0; s < pk.cs.NS; s++) {
      tr.write_scalar(ev(id_sh(ci) + s, x));
      tr.write_scalar(ev(id_sh(ci) + s, x_next));
    }
  clk.mark("evaluations");
  return H2G_OK;
}

// ---- the multi-open argument (multiopen.cpp) over this proof's polynomials, queries and
// evaluations, with the proving key's scratch
MultiopenCtx ProofRun::multiopen_ctx() {
  MultiopenCtx c;
  c.d = d;
  c.prm = &prm;
  c.st = st;
  c.tr = &tr;
  c.n = n;
  c.polys = &polys;
  c.queries = &queries;
  c.ev = [this](int poly, const Fr& pt) { return ev(poly, pt); };
  c.nx = pk.nx, c.hx = pk.hx, c.lx = pk.lx, c.q1 = pk.q1, c.scr = pk.scr, c.small = pk.small;
  c.gwc_q = &pk.gwc_q;
  c.pool = &pk.pool;
  c.upload = [this](void* dst, const void* src, size_t bytes) { return pk_upload(pk, dst, src, bytes, st); };
  c.mark = [this](const char* name) { clk.mark(name); };
  c.slabs = slabs;
  c.sl = sl;
  c.slab_pk = &pk;
  return c;
}
int ProofRun::gwc() {
  MultiopenCtx c = multiopen_ctx();
  return multiopen_gwc(c);
}
int ProofRun::shplonk() {
  MultiopenCtx c = multiopen_ctx();
  return multiopen_shplonk(c);
}

namespace {

// row pieces: the advice transforms run in the permutation stage when every transform of
// the proof has a rank of its own (prove_impl; keeping them in the advice stage: measured,
// rejected)
// Single-GPU proofs: the columns' transforms (lagrange_to_coeff, the coset extension) on a
// stream of their own (Device::xstream), joined before evaluate_h, their first reader.
// On the prover's stream they held back every later stage's kernels -- the lookups'
// sorts and grand products are chains of small launches that leave most of the chip idle,
// and ran only after the 2^20-point transforms ahead of them on the stream (keccak-style
// k = 18: the same 33.1 ms with every stage drained as without; 31.8-32.4 vs 33.3-34.3 ms
// on their own stream, profiles/r06/xs/ab_ordered_streams.log).  Only for circuits with
// lookups or shuffles: C3 (no lookups; its stages are MSM-bound, the chip already full)
// measured 76.1-77.3 vs 73.1-73.8 ms with it.  The stream is created by the first proof
// that uses it, after the MSM streams (the hardware-queue order matters, abi.cpp).  Stream
// priorities (transforms low, or MSMs high) measured slower (profiles/r06/xs/).
int prove_impl(Device* d, Params& prm, ProvingKey& pk, const ProveIn& in, std::vector<uint8_t>* proof) {
  hipStream_t st = d->stream;
  if (pk.self_check && (g_spmd.world > 1 || g_shard.world > 1))
    return fail(H2G_ERR_STATE, "create_proof: the self-check (h2g_pk_set_self_check) does not run under a shard or "
                               "SPMD transport");
  if (pk.cosets && g_spmd.world > 1)
    return fail(H2G_ERR_STATE, "create_proof: a streamed-coset key does not prove under an SPMD transport of " +
                                   std::to_string(g_spmd.world) + " ranks (make the key with H2G_COSETS_RESIDENT)");
  xp_drain(pk);  // a failed proof's overlapped exchanges
  RCCHK(pk_upload_arm(pk, st));
  while ((int)pk.cws.size() < in.nc) RCCHK(circuit_ws_add(pk));  // workspaces grow once
  // with the slab exchange and world a multiple of 2^e above it, every rank takes a row
  // piece of one sub-coset (sub_prepare)
  const int E_sub = 1 << (pk.dom.ek - pk.dom.k);
  const bool pieces = spmd_subcosets() && g_spmd.allgather_host && g_spmd.exchange && pk.multiopen == 0 &&
                      g_spmd_colshard && g_spmd.world >= kColshardMinWorld && g_spmd.world > E_sub &&
                      g_spmd.world % E_sub == 0;
  if (spmd_subcosets()) RCCHK(sub_prepare(pk, st, pieces));  // this rank's sub-cosets of the key's cosets
  const bool xsplit = g_spmd.world <= 1 && !spmd_subcosets() && pk.cs.NL + pk.cs.NS > 0;
  if (xsplit && !d->xstream) {  // after the MSM streams (h2g_init): the hardware-queue order, abi.cpp
    HIPCHK(hipStreamCreateWithFlags(&d->xstream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&d->xev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&d->xev_done, hipEventDisableTiming));
  }
  ProofRun run(d, prm, pk, in, proof, E_sub, pieces, xsplit);
  RCCHK(run.self_check_begin());
  RCCHK(run.instances());
  RCCHK(run.advice_phases());
  RCCHK(run.lookup_permuted());
  RCCHK(run.permutation_products());
  RCCHK(run.lookup_shuffle_products());
  RCCHK(run.vanishing_commit());
  RCCHK(run.eval_h());
  RCCHK(run.h_commit());
  RCCHK(run.openings_and_evals());
  RCCHK(run.self_check());
  return pk.multiopen == 1 ? run.gwc() : run.shplonk();
}

// the checks and output handling every create_proof entry point shares
int create_proof_entry(Device* d, uint64_t params, uint64_t pk, ProveIn& in, uint8_t* proof, size_t proof_cap,
                       size_t* proof_len) {
  Params* ip = find_params(params);
  if (!ip) return fail(H2G_ERR_HANDLE, "unknown params");
  ProvingKey* ik = find_pk(pk);
  if (!ik) return fail(H2G_ERR_HANDLE, "unknown proving key");
  ProvingKey& K = *ik;
  if (K.params != params) return fail(H2G_ERR_ARG, "create_proof: pk was generated with other params");
  if (K.device != d->id) return fail(H2G_ERR_ARG, "create_proof: pk lives on another device");
  if (!proof_len || in.nc < 1 || in.nc > 1024) return fail(H2G_ERR_ARG, "create_proof: bad arguments");
  for (int c = 0; c < in.nc; c++) {
    if (K.cs.A && !in.src && !in.src1 && !in.asg && (!in.advice || !in.advice[c])) return fail(H2G_ERR_ARG, "create_proof: null advice");
    if (K.cs.I && (!in.instance || !in.inst_lens || !in.instance[c] || !in.inst_lens[c]))
      return fail(H2G_ERR_ARG, "create_proof: null instance");  // InvalidInstances
  }
  std::vector<uint8_t> out;
  out.reserve(32 * 256);
  int rc = prove_impl(d, *ip, K, in, &out);
  if (rc) {
    (void)hipStreamSynchronize(d->stream);
    if (rc == H2G_ERR_UNSATISFIED) *proof_len = 0;  // refused by the self-check: no proof
    return rc;
  }
  *proof_len = out.size();
  if (out.size() > proof_cap) return fail(H2G_ERR_ARG, "create_proof: proof buffer too small");
  if (proof) std::memcpy(proof, out.data(), out.size());
  return H2G_OK;
}

// h2g_prove_inputs (after the entry point's own checks): the caller's RNG or the seed's,
// and the fields every witness form fills alike
int prove_inputs(const h2g_prove_inputs* p, std::unique_ptr<ProverRng>* rng, ProveIn* in) {
  if (!p->rng && !p->rng_seed) return fail(H2G_ERR_ARG, "create_proof: neither an rng nor a seed");
  // fill_bytes is required: the vanishing argument's ChaCha seeds are fill_bytes draws
  // (vanishing/prover.rs:69-73) whatever F::random uses
  if (p->rng && !p->rng->fill_bytes) return fail(H2G_ERR_ARG, "create_proof: the caller's rng needs fill_bytes");
  *rng = p->rng ? std::make_unique<ProverRng>(p->rng->fill_bytes, p->rng->random_fr, p->rng->ctx)
                : std::make_unique<ProverRng>(p->rng_seed);
  in->nc = (int)std::min<uint32_t>(p->num_circuits, 1u << 20);
  in->instance = p->instance;
  in->inst_lens = p->instance_lens;
  in->rng = rng->get();
  in->vthreads = p->vanishing_threads;
  return H2G_OK;
}

}  // namespace

extern "C" {

int h2g_create_proof(uint64_t params, uint64_t pk, const uint64_t* advice, int advice_on_device,
                     const uint64_t* instance, const uint32_t* instance_lens, const uint8_t rng_seed[32],
                     uint32_t vanishing_threads, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  NEED_DEV_P();
  self_check_reset();  // h2g_last_self_check speaks of this call from here on
  if (!rng_seed) return fail(H2G_ERR_ARG, "create_proof: null rng seed");
  ProverRng rng(rng_seed);
  ProveIn in;
  in.advice = &advice;
  in.adv_dev = advice_on_device != 0;
  in.instance = &instance;
  in.inst_lens = &instance_lens;
  in.rng = &rng;
  in.vthreads = vanishing_threads;
  return create_proof_entry(d, params, pk, in, proof, proof_cap, proof_len);
}

int h2g_create_proof_phased(uint64_t params, uint64_t pk, const h2g_witness_source* witness,
                            const uint64_t* instance, const uint32_t* instance_lens, const uint8_t rng_seed[32],
                            uint32_t vanishing_threads, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  NEED_DEV_P();
  self_check_reset();  // h2g_last_self_check speaks of this call from here on
  if (!rng_seed || !witness || !witness->fill) return fail(H2G_ERR_ARG, "create_proof: null argument");
  ProverRng rng(rng_seed);
  ProveIn in;
  in.src1 = witness;
  in.instance = &instance;
  in.inst_lens = &instance_lens;
  in.rng = &rng;
  in.vthreads = vanishing_threads;
  return create_proof_entry(d, params, pk, in, proof, proof_cap, proof_len);
}

int h2g_create_proof_multi(uint64_t params, uint64_t pk, const h2g_prove_inputs* p, uint8_t* proof,
                           size_t proof_cap, size_t* proof_len) {
  NEED_DEV_P();
  self_check_reset();  // h2g_last_self_check speaks of this call from here on
  if (!p || p->num_circuits < 1) return fail(H2G_ERR_ARG, "create_proof: no circuits");
  if (p->witness && !p->witness->fill) return fail(H2G_ERR_ARG, "create_proof: null witness fill");
  std::unique_ptr<ProverRng> rng;
  ProveIn in;
  RCCHK(prove_inputs(p, &rng, &in));
  in.advice = p->advice;
  in.adv_dev = p->advice_on_device != 0;
  in.src = p->witness;
  return create_proof_entry(d, params, pk, in, proof, proof_cap, proof_len);
}

int h2g_create_proof_assigned(uint64_t params, uint64_t pk, const h2g_prove_inputs* p,
                              const h2g_assigned_source* source, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  NEED_DEV_P();
  self_check_reset();  // h2g_last_self_check speaks of this call from here on
  if (!p || p->num_circuits < 1) return fail(H2G_ERR_ARG, "create_proof: no circuits");
  if (!source || !source->fill) return fail(H2G_ERR_ARG, "create_proof_assigned: null source");
  if (p->advice || p->witness)
    return fail(H2G_ERR_ARG, "create_proof_assigned: the witness comes from `source`; advice and witness must be NULL");
  std::unique_ptr<ProverRng> rng;
  ProveIn in;
  RCCHK(prove_inputs(p, &rng, &in));
  in.asg = source;
  return create_proof_entry(d, params, pk, in, proof, proof_cap, proof_len);
}

// a ChaCha20Rng::from_seed (rand_chacha 0.3) behind the h2g_rng callbacks: the RngCore
// a Rust host passes to create_proof, here native -- the caller-RNG path of
// h2g_create_proof_multi (no early vanishing commitment) with the seeded path's bytes
std::map<uint64_t, std::unique_ptr<ChaChaRng>> g_rngs;
int rng_fill_cb(void* ctx, uint8_t* out, size_t len) {
  static_cast<ChaChaRng*>(ctx)->fill(out, len);
  return 0;
}
int h2g_rng_chacha20(const uint8_t seed[32], h2g_rng* out, uint64_t* handle) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!seed || !out || !handle) return fail(H2G_ERR_ARG, "rng_chacha20: null argument");
  auto r = std::make_unique<ChaChaRng>(seed);
  out->ctx = r.get();
  out->fill_bytes = rng_fill_cb;
  out->random_fr = nullptr;
  *handle = g_next_handle++;
  g_rngs[*handle] = std::move(r);
  return H2G_OK;
}
int h2g_rng_free(uint64_t handle) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!g_rngs.erase(handle)) return fail(H2G_ERR_HANDLE, "rng_free: unknown handle");
  return H2G_OK;
}

int h2g_last_challenges(uint64_t* out, int max, int* count) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!count) return fail(H2G_ERR_ARG, "last_challenges: null count");
  *count = (int)g_last_challenges.size();
  if (out)
    for (int i = 0; i < *count && i < max; i++) std::memcpy(out + 4 * i, &g_last_challenges[i], sizeof(Fr));
  return H2G_OK;
}

int h2g_prover_stage_sync(int on) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  g_stage_sync = on != 0;
  return H2G_OK;
}

int h2g_prover_stages(double* ms, int max, int* count) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  const int c = (int)g_stages.size();
  for (int i = 0; i < c && i < max; i++) ms[i] = g_stages[i].second;
  if (count) *count = c;
  return H2G_OK;
}

const char* h2g_prover_stage_name(int i) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (i < 0 || i >= (int)g_stages.size()) return "";
  return g_stages[i].first;
}

}  // extern "C"
