// commit.cpp -- the commitment-MSM scheduler: launch, batch, slab-shard and collect.
#include "multiopen.h"  // MsmRingGuard (the batches seam)
#include "prover_state.h"

using namespace h2g;
using namespace h2g::rt;
using namespace h2g::prv;

namespace h2g {
namespace prv {
// ParamsKZG::commit / commit_lagrange (kzg/commitment.rs:305-317,354-366): MSM against a
// prefix of the resident SRS (fixed-base windows).  Launched asynchronously after the
// work queued on `st`; the affine result is collected when it enters the transcript.
// With a shard transport installed (h2g_set_shard_transport) the MSM is split into point
// slabs: this device takes slab 0, the peers the rest.
// slab r of an MSM of length n: the points [P r / world, P (r + 1) / world) of the
// params' P = 2^k, clipped to n (one partition for every MSM length, so each rank's
// slab windows cover all of its MSMs); SPMD with weights: [P S_r / S, P S_{r+1} / S)
size_t shard_lo(size_t P, size_t n, int world, int r) {
  size_t b;
  if (world > 1 && world == g_spmd.world && g_spmd_wprefix.size() == (size_t)world + 1)
    b = (size_t)((unsigned __int128)P * g_spmd_wprefix[(size_t)r] / g_spmd_wprefix[(size_t)world]);
  else
    b = (size_t)((unsigned __int128)P * (unsigned)r / (unsigned)world);
  return b < n ? b : n;
}

int commit_launch(Device* d, const Params& prm, const Fr* scalars, size_t n, int set, hipStream_t st, MsmTicket* t) {
  t->shard_seq = -1;
  size_t toff = 0;
  if (g_spmd.world > 1) {  // this rank's slab of its own copy of the scalars
    const size_t lo = shard_lo(prm.n, n, g_spmd.world, g_spmd.rank);
    const size_t hi = shard_lo(prm.n, n, g_spmd.world, g_spmd.rank + 1);
    const MsmFixedBase& tb = prm.tables(set, lo, hi - lo, &toff);
    RCCHK(msm_fixed_launch(d, scalars + lo, tb, toff, hi - lo, st, t));
    t->shard_seq = (int64_t)g_spmd_seq++;
    return H2G_OK;
  }
  if (g_shard.world <= 1) return msm_fixed_launch(d, scalars, prm.tables(set, 0, n, &toff), 0, n, st, t);
  const size_t n0 = shard_lo(prm.n, n, g_shard.world, 1);
  const MsmFixedBase& tb = prm.tables(set, 0, n0, &toff);
  RCCHK(msm_fixed_launch(d, scalars, tb, toff, n0, st, t));
  HIPCHK(hipStreamSynchronize(st));  // the transport reads the scalars right away
  const uint64_t seq = g_shard_seq++;
  if (g_shard.launch(g_shard.ctx, seq, set, n, scalars) != 0)
    return fail(H2G_ERR_STATE, "shard transport: launch of MSM " + std::to_string(seq) + " failed");
  t->shard_seq = (int64_t)seq;
  return H2G_OK;
}
int commit_collect(Device* d, MsmTicket* t, G1Affine* out) {
  if (t->remote) {  // owned by another rank: this rank's part of the sum is the identity
    std::memset(out, 0, sizeof(G1Affine));
    t->remote = false;
  } else {
    RCCHK(msm_collect(d, t, reinterpret_cast<uint64_t*>(out)));
  }
  if (t->shard_seq < 0) return H2G_OK;
  if (g_spmd.world > 1) {  // every rank's partial, summed in rank order (the same on every rank)
    const int W = g_spmd.world;
    constexpr int SW = H2G_SPMD_WORDS;
    uint64_t mine[SW];
    std::memcpy(mine, out, 64);
    mine[8] = out->is_identity() ? 1 : 0;
    spmd_digest(mine + 9);
    std::vector<uint64_t> all((size_t)W * SW);
    const int64_t seq = t->shard_seq;
    if (spmd_timed(0, (uint64_t)SW * 8 * (W + 1), [&] { return g_spmd.allgather(g_spmd.ctx, (uint64_t)seq, mine, all.data()); }) != 0)
      return fail(H2G_ERR_STATE, "spmd transport: all-gather of MSM " + std::to_string(seq) + " failed");
    t->shard_seq = -1;
    for (int r = 0; r < W; r++)
      if (std::memcmp(&all[(size_t)r * SW + 9], mine + 9, 32) != 0)
        return fail(H2G_ERR_STATE, "spmd: rank " + std::to_string(r) + " diverged from rank " +
                                       std::to_string(g_spmd.rank) + " before MSM " + std::to_string(seq) +
                                       " (different witness, instances, key or RNG draws on the ranks)");
    G1xyzz acc = G1xyzz::identity();
    for (int r = 0; r < W; r++) {
      if (all[(size_t)r * SW + 8]) continue;
      G1Affine p;
      std::memcpy(&p, &all[(size_t)r * SW], 64);
      acc = xyzz_madd(acc, p);
    }
    *out = xyzz_to_affine(acc);
    return H2G_OK;
  }
  const int peers = g_shard.world - 1;
  std::vector<G1Affine> part(peers);
  std::vector<int32_t> ids(peers, 0);
  if (g_shard.collect(g_shard.ctx, (uint64_t)t->shard_seq, reinterpret_cast<uint64_t*>(part.data()), ids.data()) != 0)
    return fail(H2G_ERR_STATE, "shard transport: collect of MSM " + std::to_string(t->shard_seq) + " failed");
  t->shard_seq = -1;
  G1xyzz acc = G1xyzz::identity();
  if (!out->is_identity()) acc = G1xyzz::from_affine(*out);
  for (int i = 0; i < peers; i++)
    if (!ids[i]) acc = xyzz_madd(acc, part[i]);
  *out = xyzz_to_affine(acc);
  return H2G_OK;
}
// The commitments of one stage together (the stage's MSMs were all launched before the
// first is needed): with SPMD and a host all-gather, every rank's partials of all of them
// travel in ONE all-gather (nb x H2G_SPMD_WORDS words per rank, one digest check), not one
// collective per MSM -- a many-column proof at 8 ranks made ~90 of them, each a host
// round trip of the ranks' streams.  The sums are the same, in rank order, as
// commit_collect's; the transcript writes follow in list order.
constexpr uint64_t kSpmdCommitTag = 0x54494d4d4f433248ull;  // "H2COMMIT"
int commit_collect_all(Device* d, MsmTicket* const* t, int nb, G1Affine* out) {
  bool spmd_all = g_spmd.world > 1 && g_spmd.allgather_host && nb > 1;
  bool local_all = nb > 1;  // plain single-GPU tickets
  for (int i = 0; i < nb; i++) {
    spmd_all &= t[i]->shard_seq >= 0;
    local_all &= t[i]->shard_seq < 0 && !t[i]->remote;
  }
  // the results leave the device in XYZZ form and go to affine together, one host inversion
  // per stage instead of one per commitment (~10 us each: ~0.3 ms a stage of 32)
  std::vector<G1xyzz> xz(nb > 0 ? nb : 1);
  if (local_all) {
    for (int i = 0; i < nb; i++) RCCHK(msm_collect_xyzz(d, t[i], &xz[i]));
    xyzz_to_affine_batch(xz.data(), out, nb);
    return H2G_OK;
  }
  if (!spmd_all) {
    for (int i = 0; i < nb; i++) RCCHK(commit_collect(d, t[i], &out[i]));
    return H2G_OK;
  }
  for (int i = 0; i < nb; i++) {
    if (t[i]->remote) {
      xz[i] = G1xyzz::identity();
      t[i]->remote = false;
    } else {
      RCCHK(msm_collect_xyzz(d, t[i], &xz[i]));
    }
  }
  xyzz_to_affine_batch(xz.data(), out, nb);
  const int W = g_spmd.world;
  constexpr int SW = H2G_SPMD_WORDS;
  // per rank: a 2-word header (tag, count -- lets a transport or a test harness recognise
  // a commitment batch), then nb records of H2G_SPMD_WORDS words as in commit_collect
  const size_t per = 2 + (size_t)nb * SW;
  std::vector<uint64_t> mine(per), all((size_t)W * per);
  mine[0] = kSpmdCommitTag;
  mine[1] = (uint64_t)nb;
  uint64_t dg[4];
  spmd_digest(dg);
  for (int i = 0; i < nb; i++) {
    uint64_t* m = &mine[2 + (size_t)i * SW];
    std::memcpy(m, &out[i], 64);
    m[8] = out[i].is_identity() ? 1 : 0;
    std::memcpy(m + 9, dg, 32);
  }
  const int64_t seq0 = t[0]->shard_seq;
  const size_t bytes = mine.size() * 8;
  if (spmd_timed(0, bytes * (W + 1), [&] { return g_spmd.allgather_host(g_spmd.ctx, mine.data(), bytes, all.data()); }) != 0)
    return fail(H2G_ERR_STATE, "spmd transport: all-gather of MSMs " + std::to_string(seq0) + ".. failed");
  for (int r = 0; r < W; r++)
    for (int i = 0; i < nb; i++)
      if (all[(size_t)r * per] != kSpmdCommitTag || all[(size_t)r * per + 1] != (uint64_t)nb ||
          std::memcmp(&all[(size_t)r * per + 2 + (size_t)i * SW + 9], dg, 32) != 0)
        return fail(H2G_ERR_STATE, "spmd: rank " + std::to_string(r) + " diverged from rank " +
                                       std::to_string(g_spmd.rank) + " before MSM " + std::to_string(seq0 + i) +
                                       " (different witness, instances, key or RNG draws on the ranks)");
  for (int i = 0; i < nb; i++) {
    t[i]->shard_seq = -1;
    G1xyzz acc = G1xyzz::identity();
    for (int r = 0; r < W; r++) {
      const uint64_t* a = &all[(size_t)r * per + 2 + (size_t)i * SW];
      if (a[8]) continue;
      G1Affine p;
      std::memcpy(&p, a, 64);
      acc = xyzz_madd(acc, p);
    }
    xz[i] = acc;
  }
  xyzz_to_affine_batch(xz.data(), out, nb);
  return H2G_OK;
}

// Several commitments against one base set as batched MSMs (msm_run_fixed_batch): one
// sort, accumulation and reduction serve a group, so the latency-bound reduction is paid
// once per group instead of once per commitment -- what circuits with many columns at
// small k (C5) are dominated by (commit_batch_chunk); with a shard transport every MSM
// goes alone (point slabs).  SPMD ranks batch their slab MSMs the same way: a 2^19-point
// slab's reduction costs about what a 2^22 MSM's does.
// MSMs per batch for commitments of length n (1: no batching).  Batching pays where
// the reduction's latency is comparable to the accumulation: measured on MI355X, a
// keccak-style k = 18 proof (80 MSMs of 2^18) 127 -> 101 ms, while C3 at k = 22 (MSMs
// of 2^22, 13 x 2^22 entries each) is 0.6 ms better without -- so only MSMs of at most
// 2^25 sorted entries are batched, up to 2^27 entries per batch.
#ifndef H2G_MSM_BATCH_ENTRIES  // A/B builds (tools/build_variant.py --src commit.cpp -D...)
#define H2G_MSM_BATCH_ENTRIES (1ull << 27)
#endif
#ifndef H2G_MSM_BATCH_PER  // the largest MSM (sorted entries) that is batched
#define H2G_MSM_BATCH_PER (1ull << 25)
#endif
int commit_batch_chunk(const MsmFixedBase& tb, size_t n) {
  const uint64_t max_entries = H2G_MSM_BATCH_ENTRIES;
  if (g_shard.world > 1) return 1;
  const uint64_t per = (uint64_t)tb.W * (n ? n : 1);
  if (per > H2G_MSM_BATCH_PER) return 1;
  int chunk = (int)std::max<uint64_t>(1, std::min<uint64_t>(MSM_MAX_BATCH, max_entries / per));
  // ... and never more sets than the pipeline takes (msm_plan: sets x 2^(c-1) buckets within
  // its partition).  Windows chosen for n never get there; a short slab against the windows
  // of the whole SRS does (SPMD without h2g_params_set_slab: 2^19 points at c = 19 would
  // batch 18 sets where 16 fit).
  MsmPlan pl;
  while (chunk > 1 && !msm_plan(n ? n : 1, tb.c, tb.W, 1, chunk, 0, &pl)) chunk--;
  return chunk;
}

}  // namespace prv
}  // namespace h2g

namespace {
// the points this rank's commitments of length n cover ([0, n), or its SPMD slab as in
// commit_launch) and the windows serving them
const MsmFixedBase& commit_tables(const Params& prm, size_t n, int set, size_t* lo, size_t* hi, size_t* toff) {
  *lo = 0;
  *hi = n;
  if (g_spmd.world > 1) {
    *lo = shard_lo(prm.n, n, g_spmd.world, g_spmd.rank);
    *hi = shard_lo(prm.n, n, g_spmd.world, g_spmd.rank + 1);
  }
  return prm.tables(set, *lo, *hi - *lo, toff);
}
}  // namespace

namespace h2g {
namespace prv {
int commit_batch_chunk(const Params& prm, size_t n, int set) {
  size_t lo, hi, toff;
  const MsmFixedBase& tb = commit_tables(prm, n, set, &lo, &hi, &toff);
  return commit_batch_chunk(tb, hi - lo);
}

int commit_launch_batch(Device* d, const Params& prm, const Fr* const* scalars, int nb, size_t n, int set,
                        hipStream_t st, MsmTicket* t) {
  size_t lo, hi, toff;
  const MsmFixedBase& tb = commit_tables(prm, n, set, &lo, &hi, &toff);
  const int chunk = commit_batch_chunk(tb, hi - lo);
  if (chunk < 2) {
    for (int b = 0; b < nb; b++) RCCHK(commit_launch(d, prm, scalars[b], n, set, st, &t[b]));
    return H2G_OK;
  }
  for (int b0 = 0; b0 < nb; b0 += chunk) {
    const int m = std::min(chunk, nb - b0);
    const Fr* sl[MSM_MAX_BATCH];
    for (int b = 0; b < m; b++) sl[b] = scalars[b0 + b] + lo;
    RCCHK(msm_fixed_launch_batch(d, reinterpret_cast<const void* const*>(sl), m, tb, toff, hi - lo, st, t + b0));
    // SPMD: every rank issues the same MSMs in the same order, so the sequence numbers agree
    for (int b = 0; b < m; b++) t[b0 + b].shard_seq = g_spmd.world > 1 ? (int64_t)g_spmd_seq++ : -1;
  }
  return H2G_OK;
}

// SPMD column ownership (wide stages): commitment i of the list is computed whole by rank
// owner[i] (its own ones batched, against the full windows), every other rank contributes
// the identity to its all-gather -- the sum is the owner's commitment, and the transcript
// and the sequence numbers stay the same on every rank.
int commit_launch_owned(Device* d, const Params& prm, const Fr* const* scalars, const int* owner, int nb, size_t n,
                        int set, hipStream_t st, MsmTicket* t) {
  std::vector<const Fr*> mine;
  std::vector<int> at;
  for (int i = 0; i < nb; i++)
    if (owner[i] == g_spmd.rank) {
      mine.push_back(scalars[i]);
      at.push_back(i);
    }
  const MsmFixedBase& tb = set == SRS_G ? prm.fg : (set == SRS_LAGRANGE ? prm.fgl : prm.fgp);
  const int chunk = std::max(1, commit_batch_chunk(tb, n));
  std::vector<MsmTicket> got(mine.size());
  for (size_t b0 = 0; b0 < mine.size(); b0 += (size_t)chunk) {
    const int m = (int)std::min<size_t>((size_t)chunk, mine.size() - b0);
    RCCHK(msm_fixed_launch_batch(d, reinterpret_cast<const void* const*>(mine.data() + b0), m, tb, 0, n, st,
                                 got.data() + b0));
  }
  for (size_t q = 0; q < at.size(); q++) t[at[q]] = got[q];
  for (int i = 0; i < nb; i++) {
    if (owner[i] != g_spmd.rank) {
      t[i] = MsmTicket{};
      t[i].remote = true;
    }
    t[i].shard_seq = (int64_t)g_spmd_seq++;
  }
  return H2G_OK;
}

int commit(Device* d, const Params& prm, const Fr* scalars, size_t n, int set, G1Affine* out, hipStream_t st) {
  MsmTicket t;
  RCCHK(commit_launch(d, prm, scalars, n, set, st, &t));
  return commit_collect(d, &t, out);
}
}  // namespace prv
}  // namespace h2g

// ---------------------------------------------------------------- test seams (include/h2g.h)
// the per-launch capacities the prover's host loops split wide work by, in h2g.h's order
int h2g_debug_limits(int32_t* out, int max, int* count) {
  const int32_t v[] = {COPY_COLS_MAX, PREFIX_DIFF_MAX, COMPRESS_BATCH_MAX, LOOKUP_KEYS_BATCH_MAX, PERM_MAXC,
                       LIN_MAXT,      NTT_MAX_BATCH,   POLY_INV_MAX_BATCH, MSM_MAX_BATCH,         MSM_RING};
  constexpr int N = (int)(sizeof(v) / sizeof(v[0]));
  static_assert(N == H2G_LIMIT_COUNT, "h2g.h lists the limits");
  if (!count || max < 0 || (max > 0 && !out)) return fail(H2G_ERR_ARG, "debug_limits: bad argument");
  for (int i = 0; i < N && i < max; i++) out[i] = v[i];
  *count = N;
  return H2G_OK;
}

// commit_batch_chunk for commitments of n points against windows of table_c bits
int h2g_debug_commit_batch_chunk(int table_c, uint64_t n, int* chunk) {
  if (!chunk) return fail(H2G_ERR_ARG, "debug_commit_batch_chunk: null argument");
  if (table_c < 1 || table_c > 31) return fail(H2G_ERR_ARG, "debug_commit_batch_chunk: window bits out of range");
  MsmFixedBase tb;
  tb.c = table_c;
  tb.W = msm_windows_for(table_c);
  tb.n = (size_t)n;
  *chunk = commit_batch_chunk(tb, (size_t)n);
  return H2G_OK;
}

// nb_total MSMs in batches of `chunk`, every batch launched before the first result is
// collected: commit_launch_batch's loop and commit_collect_all, against a base descriptor
int h2g_debug_msm_batches_dev(uint64_t base, size_t base_offset, const void* const* d_scalars, int nb_total,
                              int chunk, size_t n, uint64_t* out_affine, int32_t* is_identity) {
  NEED_DEV_P();
  Descriptor* ds = find_desc(base);
  if (!ds || !ds->is_base) return fail(H2G_ERR_HANDLE, "unknown base descriptor");
  if (!ds->fb.table) return fail(H2G_ERR_ARG, "debug_msm_batches: the descriptor has no fixed-base windows");
  if (nb_total < 0 || (nb_total && (!d_scalars || !out_affine)))
    return fail(H2G_ERR_ARG, "debug_msm_batches: null argument");
  if (chunk < 1 || chunk > MSM_MAX_BATCH) return fail(H2G_ERR_ARG, "debug_msm_batches: chunk out of range");
  if (base_offset > ds->n || n > ds->n - base_offset) return fail(H2G_ERR_ARG, "msm: bases.len() < size");
  for (int b = 0; b < nb_total; b++)
    if (n && !d_scalars[b]) return fail(H2G_ERR_ARG, "debug_msm_batches: null scalars");
  // a batch the pipeline refuses is an argument error, found before anything is launched
  MsmPlan pl;
  for (int m : {std::min(chunk, nb_total), nb_total % chunk})
    if (n && m > 0 && !msm_plan(n, ds->fb.c, ds->fb.W, 1, m, 0, &pl))
      return fail(H2G_ERR_ARG, "debug_msm_batches: a shape the MSM refuses");
  MsmRingGuard ring_guard{d};
  std::vector<MsmTicket> tk((size_t)nb_total);
  for (int b0 = 0; b0 < nb_total; b0 += chunk) {
    const int m = std::min(chunk, nb_total - b0);
    if (chunk < 2) RCCHK(msm_fixed_launch(d, d_scalars[b0], ds->fb, base_offset, n, d->stream, &tk[b0]));
    else RCCHK(msm_fixed_launch_batch(d, d_scalars + b0, m, ds->fb, base_offset, n, d->stream, &tk[b0]));
  }
  std::vector<MsmTicket*> tp((size_t)nb_total);
  for (int b = 0; b < nb_total; b++) tp[b] = &tk[b];
  std::vector<G1Affine> cm((size_t)nb_total);
  RCCHK(commit_collect_all(d, tp.data(), nb_total, cm.data()));
  for (int b = 0; b < nb_total; b++) {
    std::memcpy(out_affine + 8 * (size_t)b, &cm[b], 64);
    if (is_identity) is_identity[b] = cm[b].is_identity() ? 1 : 0;
  }
  return H2G_OK;
}
