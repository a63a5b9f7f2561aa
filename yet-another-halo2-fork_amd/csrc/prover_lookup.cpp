// prover_lookup.cpp -- LookupPermute (proof_run.h): the device pipeline of the lookup
// argument's permute_expression_pair (lookup/prover.rs:410-494), all lookups of a proof at
// once.  ProofRun::lookup_permuted (prover.cpp) runs it between theta and the commitments.
#include "proof_run.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

int LookupPermute::plan() {
  // per-lookup host staging (match counters, value masks): no host synchronisation between
  // lookups, so their device pipelines queue back to back; the counters are checked once
  // all lookups are queued
  HIPCHK(pk.lk_cnt.ensure((size_t)NLT * LKC));
  HIPCHK(pk.lk_or_d.ensure((size_t)NLT * LKF));
  HIPCHK(pk.lk_or_h.ensure((size_t)NLT * LKF));
  if ((int)pk.lk_hb.size() < NLT) pk.lk_hb.resize(NLT, 64);
  if (NLT) HIPCHK(hipMemsetAsync(pk.lk_or_d.p, 0, (size_t)NLT * LKF * sizeof(unsigned long long), st));
  lq.assign(NLT, -1);
  for (int j = 0; j < NLT; j++) {
    if (wide) r.lk_owner_all[j] = j % r.Wsp;
    if (r.lk_owner_all[j] == g_spmd.rank) lq[j] = nown++;
  }
  tsrc.assign(NLT, 0), gi0.assign(NLT, -1), gi1.assign(NLT, -1), used.assign(NLT, 0);
  share = !wide && pk.lk_trep.size() == (size_t)NL && (int)pk.lk_hb.size() >= NLT;
  for (int j = 0; j < NLT && share; j++)
    if (lq[j] >= 0 && pk.lk_hb[j] == 0) share = false;
  int ntab = 0;
  for (int j = 0; j < NLT; j++) {
    tsrc[j] = j;
    if (lq[j] < 0) continue;
    used[j] = pk.lk_hb[j];
    if (share) {
      const int rep = (j / NL) * NL + pk.lk_trep[j % NL];
      if (lq[rep] >= 0) tsrc[j] = rep;
      gi0[j] = lq[j];
      if (tsrc[j] == j) gi1[j] = nown + ntab++;
      else gi1[j] = gi1[tsrc[j]];  // (rep < j: assigned already)
    } else {
      gi0[j] = 2 * lq[j];
      gi1[j] = 2 * lq[j] + 1;
    }
  }
  G = share ? nown + ntab : 2 * nown;
  while ((1 << gbits) < G) gbits++;
  if (NLT) {  // the batch buffers, sized before anything below takes an address in them
    const size_t m = (size_t)G * u;
    HIPCHK(pk.lkb_canon.ensure(m));
    for (int q = 0; q < 2; q++) {
      HIPCHK(pk.lkb_key[q].ensure(m));
      HIPCHK(pk.lkb_idx[q].ensure(m));
    }
    HIPCHK(pk.lkb_scr.ensure(std::max(std::max(radix_sort_scratch_bytes(m), radix_sort_scratch_bytes(r.n)),
                                      compact_scratch_bytes(r.n))));
  }
  // every lookup's counters and flags cleared at once (a redo clears its own again)
  HIPCHK(pk.lk_counters.ensure((size_t)NLT * LKC));
  HIPCHK(pk.lk_flags.ensure((size_t)NLT * u));
  if (NLT) {
    HIPCHK(hipMemsetAsync(pk.lk_counters.p, 0, (size_t)NLT * LKC * sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(pk.lk_flags.p, 1, (size_t)NLT * u, st));
  }
  return H2G_OK;
}

int LookupPermute::compress() {  // batched launches
  CompressBatch cb;
  cb.prog = pk.prog;
  cb.n_slots = pk.n_slots;
  cb.consts = pk.consts;
  cb.load_rot = pk.d_load_rot;
  cb.n = r.n;
  cb.theta = r.theta;
  for (int j = 0; j < NLT; j++) {
    if (lq[j] < 0) continue;
    const CircuitWs& w = ws(j);
    const int l = j % NL;
    const int2 seg[2] = {pk.seg_lk_in[l], pk.seg_lk_tab[l]};
    Fr* const out[2] = {w.lk_a[l], w.lk_s[l]};
    for (int side = 0; side < 2; side++) {
      if (cb.count == COMPRESS_BATCH_MAX) {
        HIPCHK(compress_lagrange_batch(cb, st));
        cb.count = 0;
      }
      cb.seg[cb.count] = seg[side];
      cb.load_col[cb.count] = w.d_load_col_lag;
      cb.out[cb.count++] = out[side];
    }
  }
  HIPCHK(compress_lagrange_batch(cb, st));
  return H2G_OK;
}

int LookupPermute::key_and_sort() {
  LookupKeysBatch kb;  // every column's keys, batched launches
  kb.n = u;
  kb.canon = pk.lkb_canon.p;
  kb.key = pk.lkb_key[0].p;
  kb.idx = pk.lkb_idx[0].p;
  kb.kbits = 48;
  kb.kmask = (1ull << 48) - 1;
  for (int j = 0; j < NLT; j++) {
    if (lq[j] < 0) continue;
    const int l = j % NL, shift = used[j] > 48 ? used[j] - 48 : 0;
    const Fr* srcs[2] = {ws(j).lk_a[l], ws(j).lk_s[l]};
    for (int side = 0; side < 2; side++) {  // every column keys (a full-sort lookup's are ignored)
      if (side == 1 && tsrc[j] != j) continue;  // a shared table: keyed once, by tsrc[j]
      if (kb.count == LOOKUP_KEYS_BATCH_MAX) {
        HIPCHK(lookup_keys_batch(kb, st));
        kb.count = 0;
      }
      kb.in[kb.count] = srcs[side];
      kb.s[kb.count] = shift;
      kb.g[kb.count] = side ? gi1[j] : gi0[j];
      kb.d_or[kb.count++] = pk.lk_or_d.p + (size_t)LKF * j;
    }
  }
  HIPCHK(lookup_keys_batch(kb, st));
  if (nown) {
    bool alt = false;
    HIPCHK(radix_sort_pairs(pk.lkb_key[0].p, pk.lkb_idx[0].p, pk.lkb_key[1].p, pk.lkb_idx[1].p, (size_t)G * u, 0,
                            48 + gbits, pk.lkb_scr.p, st, &alt));
    sidx = pk.lkb_idx[alt ? 1 : 0].p;
  }
  return H2G_OK;
}

int LookupPermute::match_all() {
  if (nown) {
    // the lookups' gathers and matches on LKS streams when none needs the full sort (its
    // radix passes use the key's scratch); lookup q-th of this rank on stream q mod LKS
    bool multi = nown > 1;
    for (int j = 0; j < NLT; j++) multi = multi && (lq[j] < 0 || used[j] != 0);
    const int S = multi ? std::min(nown, ProvingKey::LKS) : 1;
    if (S > 1) {
      if (!pk.lks_a2[1]) {  // (u is the key's: these never grow)
        for (int q = 1; q < ProvingKey::LKS; q++) {
          PALLOC(pk.pool, pk.lks_a2[q], u);
          PALLOC(pk.pool, pk.lks_t2[q], u);
          PALLOC(pk.pool, pk.lks_left[q], u);
          PALLOC(pk.pool, pk.lks_rep[q], u);
          PALLOC(pk.pool, pk.lks_rows[q], u);
          HIPCHK(pk.pool.get(&pk.lks_scr[q], compact_scratch_bytes(u)));
        }
      }
      for (Stream& s : pk.lk_st) HIPCHK(s.ensure());
      for (Event& e : pk.lk_ev) HIPCHK(e.ensure());
      HIPCHK(hipEventRecord(pk.lk_ev[0], st));  // the sort is done
      for (int q = 0; q < S; q++) HIPCHK(hipStreamWaitEvent(pk.lk_st[q], pk.lk_ev[0], 0));
    }
    int qi = 0;
    for (int j = 0; j < NLT; j++) {
      if (lq[j] < 0) continue;
      const int q = S > 1 ? qi % S : 0;
      qi++;
      const Set z = set(q);
      hipStream_t sj = S > 1 ? pk.lk_st[q] : st;
      if (used[j] == 0) {
        RCCHK(full_sort(j));
      } else {
        for (int side = 0; side < 2; side++) {
          const size_t g = (size_t)(side ? gi1[j] : gi0[j]);
          HIPCHK(lookup_gather(pk.lkb_canon.p + g * u, sidx + g * u, u, side ? z.t2 : z.a2,
                               pk.lk_or_d.p + (size_t)LKF * j + 4, sj));
        }
      }
      RCCHK(match_fill(j, false, z, sj));
    }
    if (S > 1) {  // join
      for (int q = 0; q < S; q++) {
        HIPCHK(hipEventRecord(pk.lk_ev[q + 1], pk.lk_st[q]));
        HIPCHK(hipStreamWaitEvent(st, pk.lk_ev[q + 1], 0));
      }
    }
  }
  if (NLT) {
    HIPCHK(hipMemcpyAsync(pk.lk_cnt.p, pk.lk_counters.p, (size_t)NLT * LKC * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          st));
    HIPCHK(hipMemcpyAsync(pk.lk_or_h.p, pk.lk_or_d.p, (size_t)NLT * LKF * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // counters and value masks landed
  }
  return H2G_OK;
}

// the match and fill of lookup j from its sorted columns (z.a2 input, z.t2 table)
int LookupPermute::match_fill(int j, bool again, const Set& z, hipStream_t sj) {
  const CircuitWs& w = ws(j);
  const int l = j % NL;
  uint32_t* cnt = pk.lk_counters.p + (size_t)LKC * j;
  uint8_t* flags = pk.lk_flags.p + (size_t)j * u;
  if (again) {
    HIPCHK(hipMemsetAsync(flags, 1, u, sj));
    HIPCHK(hipMemsetAsync(cnt, 0, LKC * sizeof(uint32_t), sj));
  }
  HIPCHK(lookup_mark(z.a2, z.t2, u, z.rep, flags, cnt + 2, sj));
  HIPCHK(compact_canon(z.t2, flags, u, z.left, cnt, z.scr, sj));
  HIPCHK(compact_index(z.rep, u, z.rows, cnt + 1, z.scr, sj));
  HIPCHK(lookup_assign(z.a2, z.rep, u, w.lk_ap[l], w.lk_sp[l], sj));
  HIPCHK(lookup_scatter(z.left, z.rows, cnt + 1, u, w.lk_sp[l], sj));
  if (again)
    HIPCHK(hipMemcpyAsync(pk.lk_cnt.p + (size_t)LKC * j, cnt, LKC * sizeof(uint32_t), hipMemcpyDeviceToHost, sj));
  return H2G_OK;  // the blinding rows of every lookup land together (rows_upload)
}

// the full sort of lookup j's columns into pk.ck_a2 / ck_t2 (radix sorts on the limbs,
// in lookup j's own regions of the batch's key / index buffers)
int LookupPermute::full_sort(int j) {
  const int l = j % NL;
  const Fr* srcs[2] = {ws(j).lk_a[l], ws(j).lk_s[l]};
  CanonKey* sorted[2] = {pk.ck_a2, pk.ck_t2};
  for (int side = 0; side < 2; side++) {
    CanonKey* canon = pk.lkb_canon.p + (size_t)(side ? gi1[j] : gi0[j]) * u;
    HIPCHK(lookup_keys(srcs[side], u, 0, canon, nullptr, nullptr, pk.lk_or_d.p + (size_t)LKF * j, st));
    const size_t o = (size_t)gi0[j] * u;  // (the sort's scratch: the lookup's input group)
    uint64_t *k0 = pk.lkb_key[0].p + o, *k1 = pk.lkb_key[1].p + o;
    uint32_t *i0 = pk.lkb_idx[0].p + o, *i1 = pk.lkb_idx[1].p + o;
    HIPCHK(iota_u32(i0, u, st));
    for (int limb = 0; limb < 4; limb++) {  // least significant first; 8 passes end where they began
      HIPCHK(canon_limb_keys(canon, i0, u, limb, k0, st));
      bool alt = false;
      HIPCHK(radix_sort_pairs(k0, i0, k1, i1, u, 0, 64, pk.lkb_scr.p, st, &alt));
      if (alt) return fail(H2G_ERR_STATE, "lookup full sort: unexpected pass parity");
    }
    HIPCHK(lookup_gather(canon, i0, u, sorted[side], pk.lk_or_d.p + (size_t)LKF * j + 4, st));
  }
  return H2G_OK;
}

// a sort whose assumption failed (values wider than its window, or a window that tied
// different values out of order) is redone with the full sort; the width is remembered for
// the next proof
int LookupPermute::check_and_redo() {
  bool redo = false;
  std::vector<char> redone(NLT, 0);  // a lookup matched against a shared table redone with it
  for (int j = 0; j < NLT; j++) {
    if (lq[j] < 0 || used[j] == 0) continue;
    const unsigned long long* f = pk.lk_or_h.p + (size_t)LKF * j;
    int hb = 0;
    for (int q = 3; q >= 0 && !hb; q--)
      if (f[q]) hb = 64 * q + 64 - __builtin_clzll(f[q]);
    if (hb == 0) hb = 1;
    const bool tie = f[4] != 0;
    pk.lk_hb[j] = tie && hb == used[j] ? 0 : hb;  // ties at the right width: full sort from now on
    if (tie || hb > used[j] || redone[tsrc[j]]) {
      RCCHK(full_sort(j));
      RCCHK(match_fill(j, true, set(0), st));
      redo = true;
      redone[j] = 1;
    }
  }
  if (redo) HIPCHK(hipStreamSynchronize(st));
  return H2G_OK;
}

// rows: per lookup j the bf + 1 random rows of A'_j, then S'_j's (every rank draws all of
// them; the lookups this rank sorted take theirs)
int LookupPermute::rows_upload(const std::vector<Fr>& rows) {
  const size_t nb = (size_t)r.bf + 1;
  HIPCHK(pk.blind_d.ensure(rows.size()));
  std::vector<CopySeg> segs;
  for (int j = 0; j < NLT; j++) {
    if (lq[j] < 0) continue;
    const CircuitWs& w = ws(j);
    const int l = j % NL;
    for (int which = 0; which < 2; which++)
      segs.push_back(CopySeg{pk.blind_d.p + ((size_t)2 * j + which) * nb, (which ? w.lk_sp[l] : w.lk_ap[l]) + u,
                             (uint64_t)nb});
  }
  return upload_rows_batch(pk, rows.data(), rows.size(), segs, st);
}

bool LookupPermute::matched() const {
  for (int j = 0; j < NLT; j++) {
    const uint32_t* cnt = pk.lk_cnt.p + (size_t)LKC * j;
    if (lq[j] >= 0 && (cnt[2] != 0 || cnt[0] != cnt[1])) return false;
  }
  return true;
}
