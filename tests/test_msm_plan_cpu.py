"""The MSM's host rule (msm_plan in csrc/msm.hip: the function every MSM pipeline allocates and
launches from) through its host-only seam, h2g_debug_msm_plan: the geometry, the chunk rule,
the kernel variants and the size of every workspace buffer, as functions of the call's shape.
No GPU: the rule is host code and needs no h2g_init.

The expected values are written out from the rule as it stood before msm_plan existed (one
scope of msm_pipeline), by hand.  Notation: W = ceil(255 / c) windows, NB = 2^(c-1) buckets
per set; variable-base MSMs have W bucket sets, fixed-base batches one per MSM; nbt = sets x NB.

Three cases of the issue this file answers name sizes that no shape has, since nbt is a
number of sets (<= 64 fixed, W variable) times a power of two and the entry bound a multiple
of W: the fixup's lane form "at nbt = 32769" is pinned at the next shape above 32768 (33 sets
of 1024), the first refused partition "at nbt = 2^22 + 1" at the next shape above 2^22 (33
sets of 2^17), and the staged fine pass "at 2^25 - 1 entries" at 2^25 - 16 (W = 16).

tests/test_gpu_parity.py::test_msm_every_reachable_variant runs each variant's kernels."""
import ctypes

import pytest

import h2g

ERR_ARG = 1
PT = 144   # bytes of a G1xyzz29
XYZZ = 128  # bytes of a G1xyzz


def windows(c):
    return (255 + c - 1) // c


def variant(**kw):
    """("plane", Q, rgp), ("rscale",) or ("refused",)"""
    try:
        pl = h2g.debug_msm_plan(**kw)
    except h2g.H2GError:
        return ("refused",)
    if pl["red"] == "rscale":
        assert (pl["plane_q"], pl["plane_lb"], pl["rgp"], pl["e0"], pl["m1p"], pl["nblk_p"]) == (0,) * 6
        assert pl["m1"] == (pl["NB"] + 7) // 8 and pl["nblk"] == (pl["m1"] + 255) // 256
        return ("rscale",)
    assert (pl["m1"], pl["nblk"]) == (0, 0)
    assert pl["plane_lb"] == (6 if pl["plane_q"] == 4 else 8)
    assert 1 << pl["e0"] == pl["rgp"]
    assert pl["m1p"] == (pl["NB"] + pl["rgp"] - 1) // pl["rgp"]
    assert pl["nblk_p"] == (pl["m1p"] + (1 << pl["plane_lb"]) - 1) >> pl["plane_lb"] <= 512
    return ("plane", pl["plane_q"], pl["rgp"])


def test_seam_declared_bound_and_exported():
    assert "h2g_debug_msm_plan" in h2g.header_symbols()
    assert "h2g_debug_msm_plan" in h2g._SIGS
    assert hasattr(h2g.lib(), "h2g_debug_msm_plan")
    assert ctypes.sizeof(h2g.MsmPlan) == 8 * (3 + 10 + 1) + 4 * 24  # h2g_msm_plan: no padding
    assert len(h2g.MSM_BUFFERS) == 10
    assert h2g.lib().h2g_abi_version() == 1


# the reduction variant of every window size: {first c: variant} up to the next entry
Q4 = {1: ("plane", 4, 1), 2: ("plane", 4, 2), 4: ("plane", 4, 4), 8: ("plane", 4, 8)}
Q1, RSCALE, REFUSED = ("plane", 1, 8), ("rscale",), ("refused",)
VARIABLE = {2: Q4[1], 13: Q4[2], 14: Q4[4], 15: Q1, 20: REFUSED}
FIXED = {1: {2: Q4[1], 17: Q4[2], 18: Q4[4], 19: Q4[8], 20: Q1, 22: RSCALE, 24: REFUSED},
         2: {2: Q4[1], 17: Q4[2], 18: Q4[4], 19: Q1, 22: RSCALE, 23: REFUSED},
         33: {2: Q4[1], 12: Q4[2], 13: Q4[4], 14: Q1, 18: REFUSED},
         64: {2: Q4[1], 12: Q4[2], 13: Q4[4], 14: Q1, 18: REFUSED}}


def table(steps, c):
    return steps[max(k for k in steps if k <= c)]


@pytest.mark.parametrize("c", range(2, 25))
def test_reduction_variant_variable_base(c):
    assert variant(n=3000, c=c) == table(VARIABLE, c)


@pytest.mark.parametrize("nbatch", sorted(FIXED))
@pytest.mark.parametrize("c", range(2, 25))
def test_reduction_variant_fixed_base(c, nbatch):
    assert variant(n=3000, c=c, fixed=True, nbatch=nbatch) == table(FIXED[nbatch], c)


def test_rgp_loop_clauses_at_their_edges():
    """rgp: the fewest buckets per group (1, 2, 4, else 8) with g = NB / rgp groups per set,
    g x sets <= 65536 and g <= 2^15"""
    # the first clause: 2^15 buckets per set; 2 sets are 65536 groups of one, 4 are not, 5 need rgp 4
    got = [variant(n=3000, c=16, fixed=True, nbatch=s) for s in (1, 2, 4, 5)]
    assert got == [Q4[1], Q4[1], Q4[2], Q4[4]]
    # the second: one set of 2^18 buckets has 2^16 groups even at rgp 4 and falls through to 8;
    # two such sets are past 2^18 buckets and take the lane form
    assert [variant(n=3000, c=19, fixed=True, nbatch=s) for s in (1, 2)] == [Q4[8], Q1]
    # it also decides at 2^16 and 2^17 buckets in one set, where the first clause would allow less
    assert [variant(n=3000, c=c, fixed=True) for c in (17, 18)] == [Q4[2], Q4[4]]
    # 19 sets of 2^13 are within 2^18 buckets (rgp 4), 17 sets of 2^14 are not
    assert (variant(n=3000, c=14), variant(n=3000, c=15)) == (Q4[4], Q1)


def test_rscale_only_where_the_groups_exceed_the_quad_threshold():
    """The deleted quad group kernels were taken for m1 x sets <= 32768 groups (m1 = NB / 8)
    within the rscale scheme; the scheme itself is taken only from 2^21 buckets per set, where
    m1 = 2^18.  Every shape, whatever the batch."""
    seen = 0
    for c in range(2, 25):
        for kw in [dict()] + [dict(fixed=True, nbatch=s) for s in range(1, 65)]:
            try:
                pl = h2g.debug_msm_plan(3000, c, **kw)
            except h2g.H2GError:
                continue
            assert (pl["red"] == "rscale") == (c >= 22), (c, kw)
            if pl["red"] == "rscale":
                seen += 1
                assert pl["m1"] > 32768 and pl["m1"] * pl["WB"] > 32768
                assert pl["m1"] == 1 << (c - 4) and pl["WB"] <= 2 and pl["fixed"] == 1
    assert seen == 3  # fixed c = 22 with one and two sets, c = 23 with one


def test_fixup_lanes_at_the_threshold():
    assert h2g.debug_msm_plan(3000, 16, fixed=True)["nbt"] == 32768
    assert h2g.debug_msm_plan(3000, 16, fixed=True)["fixup_q"] == 4
    pl = h2g.debug_msm_plan(3000, 11, fixed=True, nbatch=32)
    assert (pl["nbt"], pl["fixup_q"]) == (32768, 4)
    pl = h2g.debug_msm_plan(3000, 11, fixed=True, nbatch=33)  # the next shape above
    assert (pl["nbt"], pl["fixup_q"]) == (33792, 1)
    assert h2g.debug_msm_plan(3000, 12)["fixup_q"] == 1  # 22 x 2048 = 45056
    assert h2g.debug_msm_plan(3000, 11)["fixup_q"] == 4  # 24 x 1024 = 24576


def test_staged_fine_pass_below_2_25_entries():
    assert windows(16) == 16
    pl = h2g.debug_msm_plan((1 << 21) - 1, 16, fixed=True)
    assert (pl["total"], pl["staged"]) == ((1 << 25) - 16, 1)
    pl = h2g.debug_msm_plan(1 << 21, 16, fixed=True)
    assert (pl["total"], pl["staged"]) == (1 << 25, 0)
    pl = h2g.debug_msm_plan(1 << 17, 16, fixed=True, nbatch=16)  # the batch counts
    assert (pl["total"], pl["staged"]) == (1 << 25, 0)


@pytest.mark.parametrize("kw,nbt,fb,ncoarse", [
    (dict(c=10, fixed=True), 1 << 9, 9, 1),     # fewer keys than 2^10: every key bit is a fine bit
    (dict(c=11, fixed=True), 1 << 10, 10, 1),
    (dict(c=12, fixed=True), 1 << 11, 10, 2),
    (dict(c=22, fixed=True), 1 << 21, 10, 2048),  # the most bins at 10 fine bits
    (dict(c=19), 14 << 18, 11, 1792),
    (dict(c=23, fixed=True), 1 << 22, 11, 2048),  # the most keys there are bins for
])
def test_partition_geometry(kw, nbt, fb, ncoarse):
    pl = h2g.debug_msm_plan(3000, **kw)
    assert (pl["nbt"], pl["fb"], pl["ncoarse"], pl["kblocks"]) == (nbt, fb, ncoarse, (nbt + 1023) // 1024)


def test_first_refused_partition():
    """more than 2048 coarse bins at 11 fine bits: the next shape above 2^22 keys"""
    assert variant(n=3000, c=18, fixed=True, nbatch=32)[0] == "plane"  # 2^22
    assert variant(n=3000, c=18, fixed=True, nbatch=33) == REFUSED     # 2^22 + 2^17
    assert variant(n=3000, c=20) == REFUSED                            # 13 x 2^19


def test_chunk_rule():
    # the case msm_chunk_len's comment cites: 2^19 points at c = 17 against a table, ~120 entries in
    # each of 2^16 buckets.  15 windows: 7864320 entries; total / 2^20 = 7 is below the quarter
    # bucket 7864320 / (4 x 65536) = 30, itself below total >> 17 = 60
    pl = h2g.debug_msm_plan(1 << 19, 17, fixed=True)
    assert (pl["W"], pl["total"], pl["nb_eff"]) == (15, 7864320, 65536)
    assert (pl["chunk_len"], pl["chunk_adapt"]) == (30, 1)
    # msm_chunk_cap: the host's 262144 chunks, or the device's most, 2^18 x 9 / 8 + 1
    assert pl["nchunks"] == 294913
    # the clamp at 8: few entries; the device cannot make more chunks than total / 8
    pl = h2g.debug_msm_plan(3000, 13)
    assert (pl["total"], pl["nb_eff"], pl["chunk_len"], pl["nchunks"]) == (60000, 20 << 12, 8, 7500)
    # the clamp at 128: 2^28 entries (total / 2^20 = 256; quarter bucket 4096 capped by total >> 17)
    pl = h2g.debug_msm_plan(1 << 24, 16, fixed=True)
    assert (pl["total"], pl["nb_eff"], pl["chunk_len"], pl["nchunks"]) == (1 << 28, 1 << 14, 128, 1 << 21)
    # variable-base windows reach all NB buckets, balanced fixed-base ones 2^(255 // W - 1)
    assert h2g.debug_msm_plan(1 << 19, 17)["nb_eff"] == 15 << 16
    assert h2g.debug_msm_plan(1 << 19, 19, fixed=True, nbatch=3)["nb_eff"] == 3 << 17
    # an explicit chunk length is kept, on the host and on the device
    pl = h2g.debug_msm_plan(3000, 13, item_len=52)
    assert (pl["chunk_len"], pl["chunk_adapt"], pl["nchunks"]) == (52, 0, 1154)


def scratch_words(nbt):
    return 3 * 2048 + 16 + 256 + 2 * ((nbt + 1023) // 1024) + 3 * nbt + 1


def test_buffer_sizes_variable_3000_c13():
    """20 sets of 4096; 60000 entries in 7500 chunks of 8; items 2 x 7500 / 64 + 2 x 7500 / 8 + 2 =
    2111, multi-item buckets 234 + 2.  red: the S/R/P layout's 2 x 512 groups + 8 block sums of 64
    groups per set exceed the planes' 10 x 32 + 32"""
    pl = h2g.debug_msm_plan(3000, 13)
    assert (pl["WB"], pl["NB"], pl["nbt"], pl["total"], pl["nchunks"]) == (20, 4096, 81920, 60000, 7500)
    assert pl["bytes"] == {"ent": 81920 * PT, "vals": 240000, "items": 2111 * 16, "bnd": 15000 * PT,
                           "buckets": 81920 * PT, "red": 1032 * 20 * PT, "windows": 20 * XYZZ,
                           "counters": 16 + 4 * 4097, "multi": 236 * 16, "item_sums": 2111 * PT}
    assert pl["bytes"]["red"] == 2972160 and pl["bytes"]["ent"] == 11796480
    assert pl["scratch_words"] == scratch_words(81920) == 252337


def test_buffer_sizes_fixed_2_20_default_window():
    """c = 19: 14 windows, one set of 2^18; 14680064 entries, chunks of 28 (quarter bucket)"""
    pl = h2g.debug_msm_plan(1 << 20, 0, fixed=True)
    assert (pl["c"], pl["W"], pl["WB"], pl["nbt"], pl["total"]) == (19, 14, 1, 1 << 18, 14680064)
    assert (pl["chunk_len"], pl["nchunks"]) == (28, 524288)
    items = 2 * 524288 // 64 + 2 * 524288 // 8 + 2
    assert items == 147458
    assert pl["bytes"] == {"ent": 14680064 * 8, "vals": 14680064 * 4, "items": items * 16, "bnd": 2 * 524288 * PT,
                           "buckets": (1 << 18) * PT, "red": (2 * 32768 + 512) * PT, "windows": 14 * XYZZ,
                           "counters": 16404, "multi": 16386 * 16, "item_sums": items * PT}
    assert pl["bytes"]["red"] == 9510912 and pl["bytes"]["bnd"] == 150994944
    assert pl["scratch_words"] == scratch_words(1 << 18) == 793361


def test_buffer_sizes_fixed_2_18_batch_of_8():
    """c = 17: 15 windows, 8 sets of 2^16; 31457280 entries in chunks of 30.  65536 groups over the
    sets: 32 block sums of 256 groups per set"""
    pl = h2g.debug_msm_plan(1 << 18, 0, fixed=True, nbatch=8)
    assert (pl["c"], pl["W"], pl["WB"], pl["nbt"], pl["total"]) == (17, 15, 8, 1 << 19, 31457280)
    assert (pl["chunk_len"], pl["nchunks"]) == (30, 1 << 20)
    items = 2 * (1 << 20) // 64 + 2 * (1 << 20) // 8 + 2
    assert pl["bytes"] == {"ent": 31457280 * 8, "vals": 31457280 * 4, "items": items * 16, "bnd": (2 << 20) * PT,
                           "buckets": (1 << 19) * PT, "red": (2 * 8192 + 32) * 8 * PT, "windows": 15 * XYZZ,
                           "counters": 16404, "multi": (32768 + 2) * 16, "item_sums": items * PT}
    assert pl["bytes"]["red"] == 18911232 and pl["bytes"]["item_sums"] == 42467616
    assert pl["scratch_words"] == scratch_words(1 << 19) == 1580305


def test_whole_buckets_fit_the_entries_buffer_either_way():
    for kw in (dict(n=3000, c=17), dict(n=1 << 22, c=13, fixed=True)):
        pl = h2g.debug_msm_plan(**kw)
        assert pl["bytes"]["ent"] == max(pl["total"] * 8, pl["nbt"] * PT)


def test_rejections_return_the_argument_error_and_leave_the_plan_untouched():
    pl = h2g.MsmPlan()
    pl.c = 77
    f = h2g.lib().h2g_debug_msm_plan
    out = ctypes.byref(pl)
    assert f(3000, 13, 0, 1, 0, None) == ERR_ARG
    assert f(3000, -1, 0, 1, 0, out) == ERR_ARG
    assert f(3000, 32, 0, 1, 0, out) == ERR_ARG
    for nbatch in (0, -1, 65):                      # the batch range
        assert f(3000, 13, 1, nbatch, 0, out) == ERR_ARG
    assert f(3000, 13, 0, 2, 0, out) == ERR_ARG     # variable-base MSMs are not batched
    assert f(1 << 27, 16, 1, 1, 0, out) == ERR_ARG  # 2^31 entries
    assert f(1 << 21, 16, 1, 64, 0, out) == ERR_ARG
    assert f(1 << 31, 16, 1, 1, 0, out) == ERR_ARG
    assert f(3000, 20, 0, 1, 0, out) == ERR_ARG     # more than 2048 coarse bins
    assert f(3000, 24, 1, 1, 0, out) == ERR_ARG
    assert pl.c == 77 and pl.total == 0
    assert f((1 << 27) - 1, 16, 1, 1, 0, out) == 0 and pl.total == (1 << 31) - 16
    assert f(3000, 13, 1, 64, 0, out) == 0 and pl.WB == 64


def test_window_choosers():
    """msm_choose_c minimises W (n + 2.8 NB), msm_choose_c_fixed W n + 3 NB with a 2 % bias to the
    smaller table, both over c = 2 .. 22"""
    variable = [6, 7, 8, 8, 9, 10, 11, 12, 13, 13, 15, 15, 16, 17, 17, 19, 20, 20, 22, 22]
    fixed = [9, 10, 10, 11, 13, 13, 15, 15, 15, 16, 17, 17, 19, 20, 20, 22, 22, 22, 22, 22]
    for k, cv, cf in zip(range(8, 28), variable, fixed):
        pl = h2g.debug_msm_plan(1 << k, 0, fixed=True)
        assert (pl["c"], pl["W"]) == (cf, windows(cf)), k
        if cv < 20:
            pl = h2g.debug_msm_plan(1 << k, 0)
            assert (pl["c"], pl["W"], pl["WB"]) == (cv, windows(cv), windows(cv)), k
        else:
            assert variant(n=1 << k) == REFUSED, k
    assert h2g.debug_msm_plan(3)["c"] == 2 and h2g.debug_msm_plan(3, fixed=True)["c"] == 2


def test_variable_base_default_window_is_refused_from_2_24_points():
    """A latent rejection, pinned as it stands: msm_choose_c picks c = 20 from 2^24
    points, whose 13 x 2^19 buckets exceed the partition's 2048 coarse bins of 2^11 keys.  The
    prover commits against fixed-base tables and never asks for it."""
    assert variant(n=1 << 23) == Q1 and h2g.debug_msm_plan(1 << 23)["c"] == 19
    assert variant(n=1 << 24) == REFUSED and variant(n=1 << 24, c=20) == REFUSED
    assert variant(n=1 << 24, c=19) == Q1


# ----------------------------------------------------------------------------- the commitment batch
FIXED_C = dict(zip(range(8, 28), [9, 10, 10, 11, 13, 13, 15, 15, 15, 16, 17, 17, 19, 20, 20, 22, 22, 22, 22, 22]))


def test_commit_batch_chunk_rule():
    """commit_batch_chunk (csrc/commit.cpp): min(64, 2^27 / (W n)) commitments of n points in one
    pipeline, none batched past 2^25 entries each"""
    assert h2g.debug_commit_batch_chunk(17, 1 << 18) == (1 << 27) // (15 << 18) == 34   # keccak-style k = 18
    assert h2g.debug_commit_batch_chunk(11, 128) == 64
    assert h2g.debug_commit_batch_chunk(16, 1 << 21) == 4     # 2^25 entries each: still batched
    assert h2g.debug_commit_batch_chunk(16, (1 << 21) + 1) == 1
    assert h2g.debug_commit_batch_chunk(20, 1 << 22) == 1     # C3 at k = 22: 13 x 2^22


@pytest.mark.parametrize("k", range(8, 25))
def test_commit_batch_chunk_is_a_batch_the_plan_takes(k):
    """Whatever slab of 2^k points a rank commits on (the whole, down to an eighth: the SPMD
    point slabs), against windows chosen for the slab's length or against the windows of the
    whole SRS (Params::tables without h2g_params_set_slab), the batch commit_batch_chunk
    chooses -- and every smaller one, the stage's remainder -- is a shape msm_plan accepts.
    Before the rule asked the plan, 2^19-point slabs of k = 20 against c = 19 gave 18 sets
    where 16 fit, and the slabs of k = 21 against c = 20 gave 9 and 14 where 8 fit."""
    full_c = FIXED_C[k]
    assert h2g.debug_msm_plan(1 << k, 0, fixed=True)["c"] == full_c
    for parts in range(1, 9):
        for r in range(parts):
            n = ((r + 1) << k) // parts - (r << k) // parts   # shard_lo's slabs
            slab_c = h2g.debug_msm_plan(n, 0, fixed=True)["c"]
            for c in sorted({slab_c, full_c}):
                chunk = h2g.debug_commit_batch_chunk(c, n)
                assert 1 <= chunk <= 64
                w = windows(c)
                want = 1 if w * n > 1 << 25 else max(1, min(64, (1 << 27) // (w * n)))
                fits = (1 << 22) >> (c - 1)   # sets of 2^(c-1) buckets within 2048 bins of 2^11 keys
                assert chunk == max(1, min(want, fits)), (k, parts, c)
                for nb in range(1, chunk + 1):
                    assert variant(n=n, c=c, fixed=True, nbatch=nb) != REFUSED, (k, parts, c, nb)


def test_commit_batch_chunk_is_bound_by_the_plan_only_on_short_slabs():
    """the two never meet on one device (closest: k = 18, 34 sets of 2^16 against 64); the cases
    worked by hand where they do"""
    for k in range(8, 25):
        c = FIXED_C[k]
        w = windows(c)
        if w << k <= 1 << 25:
            assert min(64, (1 << 27) // (w << k)) <= (1 << 22) >> (c - 1), k
    assert h2g.debug_commit_batch_chunk(19, 1 << 19) == 16                 # k = 20 on 2 ranks: was 18
    assert h2g.debug_commit_batch_chunk(19, (1 << 20) // 3) == 16          # 3 ranks: was 27
    assert h2g.debug_commit_batch_chunk(20, 1 << 20) == 8                  # k = 21 on 2 ranks: was 9
    assert h2g.debug_commit_batch_chunk(20, (1 << 21) // 3) == 8           # 3 ranks: was 14
