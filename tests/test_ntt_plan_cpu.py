"""The NTT's host rule (ntt_plan in csrc/ntt.hip: the function ntt_run launches from) through
its host-only seam, h2g_debug_ntt_plan: which split, first-pass kernel, persistent grid and
last-pass variant serve which shape.  No GPU: the rule is host code and needs no h2g_init.

A pass's work is 2^L / 512 wave items in blocks of 4, so `blocks` = 2^L / 2048; the passes
after the first and before the last are persistent, on min(blocks, 2 CUs / count) blocks.

Not reachable from any public entry, and so run by no test: ntt_last29_kernel<true, true>,
a truncated last pass without an epilogue constant.  Truncation comes from extended_to_coeff
alone, and its zeta undistribution always leaves a constant; the rule itself still names the
variant (test_last_pass_variants).  No entry point exists to reach it, on purpose.

Five-pass plans (L = 25 .. 28) are pinned here; their kernel side -- the last pass's digit
reversal with three middle digits -- rests on test_c3_k24_proof_bytes_match_oracle_and_verify
alone (1-2 GiB buffers; the shape cannot be made small).

tests/test_gpu_ntt_shapes.py runs the kernels at the shapes of _ntt_shapes.CASES."""
import ctypes

import pytest

import _ntt_shapes as S
import h2g

ERR_ARG = 1

SPLITS = {11: (5, 6), 12: (6, 6), 13: (3, 4, 6), 14: (3, 5, 6), 15: (3, 6, 6), 16: (4, 6, 6), 17: (5, 6, 6),
          18: (6, 6, 6), 19: (3, 4, 6, 6), 20: (3, 5, 6, 6), 21: (3, 6, 6, 6), 22: (4, 6, 6, 6), 23: (5, 6, 6, 6),
          24: (6, 6, 6, 6), 25: (3, 4, 6, 6, 6), 26: (3, 5, 6, 6, 6), 27: (3, 6, 6, 6, 6), 28: (4, 6, 6, 6, 6)}


def test_seam_declared_bound_and_exported():
    assert "h2g_debug_ntt_plan" in h2g.header_symbols()
    assert "h2g_debug_ntt_plan" in h2g._SIGS
    assert hasattr(h2g.lib(), "h2g_debug_ntt_plan")
    assert ctypes.sizeof(h2g.NttPlan) == 4 * (1 + 6 + 4 + 2 + 6)  # h2g_ntt_plan: 19 32-bit fields, no padding
    assert h2g.lib().h2g_abi_version() == 1


@pytest.mark.parametrize("L", range(0, 29))
def test_split(L):
    N = 1 << L
    pl = h2g.debug_ntt_plan(L, N)
    if L <= 10:
        assert pl["split"] == (L,) and pl["first"] == "one_block"
        assert (pl["blocks"], pl["first_grid"], pl["pgrid"]) == (0, 1, {})
        assert (pl["trunc"], pl["one"]) == (False, False)
        return
    assert pl["split"] == SPLITS[L]
    assert sum(pl["split"]) == L and pl["split"][-1] == 6 and all(3 <= m <= 6 for m in pl["split"])
    assert pl["blocks"] == N // 2048
    assert pl["first"] == "plain" and pl["first_grid"] == pl["blocks"]
    assert pl["pgrid"] == {p: min(N // 2048, 512) for p in range(1, len(pl["split"]) - 1)}


def test_one_block_is_one_block_per_transform_twisted_or_not():
    for L in (0, 6, 10):
        for tw in (False, True):
            pl = h2g.debug_ntt_plan(L, 1 << L, count=5, in_twist=tw)
            assert (pl["first"], pl["first_grid"], pl["split"]) == ("one_block", 5, (L,))
    assert h2g.debug_ntt_plan(11, 1 << 11, in_twist=True)["first"] == "twisted"


@pytest.mark.parametrize("L", [13, 14, 15, 19, 20, 21, 25])
def test_sparse_rule_at_its_threshold(L):
    """lg[0] == 3 and n_in <= N / 4; a twisted transform never takes it"""
    N = 1 << L
    assert SPLITS[L][0] == 3
    for n_in, want in ((0, "sparse"), (1, "sparse"), (N // 16, "sparse"), (N // 8, "sparse"), (N // 4, "sparse"),
                       (N // 4 + 1, "plain"), (N // 2, "plain"), (N, "plain")):
        pl = h2g.debug_ntt_plan(L, n_in)
        assert pl["first"] == want, (L, n_in)
        assert pl["first_grid"] == (N // 8 // 256 if want == "sparse" else N // 2048)
    assert h2g.debug_ntt_plan(L, N // 4, in_twist=True)["first"] == "twisted"


@pytest.mark.parametrize("L", [11, 12, 16, 17, 18, 22, 23, 24, 28])
def test_sparse_rule_needs_a_three_bit_first_pass(L):
    assert SPLITS[L][0] != 3
    for n_in in (1, (1 << L) // 4):
        assert h2g.debug_ntt_plan(L, n_in)["first"] == "plain"


@pytest.mark.parametrize("L", [11, 13, 18, 19, 25])
def test_last_pass_variants(L):
    """TRUNC: out_len < N, with 0 standing for N; ONE: as the caller says"""
    N = 1 << L
    for out_len, trunc in ((N - 1, True), (N, False), (0, False), (1, True), (N // 2, True)):
        for one in (False, True):
            pl = h2g.debug_ntt_plan(L, N, out_len, epilogue_one=one)
            assert (pl["trunc"], pl["one"]) == (trunc, one), (L, out_len, one)
    # truncation changes nothing else
    a, b = h2g.debug_ntt_plan(L, N, N - 1), h2g.debug_ntt_plan(L, N, N)
    assert {k: v for k, v in a.items() if k != "trunc"} == {k: v for k, v in b.items() if k != "trunc"}


def test_persistent_grid_per_batch_size_at_256_cus():
    want = {1: 512, 2: 256, 3: 170, 4: 128, 5: 102, 6: 85, 7: 73, 8: 64}
    for count, g in want.items():
        for L in (18, 20, 24):
            blocks = (1 << L) // 2048
            pl = h2g.debug_ntt_plan(L, 1 << L, count=count, cus=256)
            assert pl["cus"] == 256 and pl["blocks"] == blocks
            assert set(pl["pgrid"].values()) == {min(blocks, g)}, (count, L)
    # at 2^18 (128 blocks) the batches of 5, 6 and 7 leave a ragged tail (3: 170 > 128 blocks, one
    # item per wave), from 2^19 on the batches of 3 as well; 1, 2, 4, 8 never do
    ragged = [c for c in want if 128 % h2g.debug_ntt_plan(18, 1 << 18, count=c)["pgrid"][1]]
    assert ragged == [5, 6, 7]
    ragged = [c for c in want if 256 % h2g.debug_ntt_plan(19, 1 << 19, count=c)["pgrid"][1]]
    assert ragged == [3, 5, 6, 7]
    assert not [c for c in (1, 2, 4, 8) for L in range(17, 29)
                if ((1 << L) // 2048) % h2g.debug_ntt_plan(L, 1 << L, count=c)["pgrid"][1]]
    # two-pass transforms have no middle pass; other CU counts scale the grid; never below one block
    assert h2g.debug_ntt_plan(12, 1 << 12, count=3)["pgrid"] == {}
    assert h2g.debug_ntt_plan(20, 1 << 20, count=3, cus=304)["pgrid"] == {1: 202, 2: 202}
    assert h2g.debug_ntt_plan(20, 1 << 20, count=8, cus=1)["pgrid"] == {1: 1, 2: 1}


def test_argument_errors_need_no_device():
    pl = h2g.NttPlan()
    pl.passes = -1
    f = h2g.lib().h2g_debug_ntt_plan
    assert f(12, 1, 0, 1, 0, 256, 1, None) == ERR_ARG
    assert f(29, 1, 0, 1, 0, 256, 1, ctypes.byref(pl)) == ERR_ARG
    assert f(12, 1, (1 << 12) + 1, 1, 0, 256, 1, ctypes.byref(pl)) == ERR_ARG
    assert f(12, 1, 0, 9, 0, 256, 1, ctypes.byref(pl)) == ERR_ARG  # more than NTT_MAX_BATCH
    assert f(12, 1, 0, 1, 0, -1, 1, ctypes.byref(pl)) == ERR_ARG
    assert pl.passes == -1
    assert h2g.debug_ntt_plan(12, 1, count=0)["first_grid"] == h2g.debug_ntt_plan(12, 1, count=1)["first_grid"]
    assert h2g.debug_ntt_plan(18, 1, cus=0)["cus"] > 0  # the library's own count (256 without a device)


@pytest.mark.parametrize("j,k", sorted(S.CASES))
def test_gpu_shape_selects_the_variant_it_is_listed_for(j, k):
    pl = S.require(j, k)
    ek, split, first, keep = S.CASES[(j, k)]
    # lagrange_to_coeff and the sub-coset transform are n-point: never truncated, never sparse
    for name in ("l2c", "subcoset"):
        assert not pl[name]["trunc"] and pl[name]["first"] != "sparse"
        assert pl[name]["split"] == (SPLITS[k] if k > 10 else (k,))
    assert pl["subcoset"]["first"] == ("twisted" if k > 10 else "one_block")


def test_the_listed_shapes_cover_every_variant_they_claim():
    got = {(j, k): S.require(j, k) for (j, k) in S.CASES}
    # every first-pass width under truncation, three and four passes
    assert {p["e2c"]["split"][0] for p in got.values()} == {3, 4, 5, 6}
    assert {len(p["e2c"]["split"]) for p in got.values()} == {2, 3, 4}
    # the sparse pass with both inputs (4n), with x[1] zero (8n) and with half of x[0] zero (16n)
    ratio = {(1 << S.CASES[c][0]) >> c[1] for c, p in got.items() if p["c2e"]["first"] == "sparse"}
    assert ratio == {4, 8, 16}
    # the twisted first pass at lg[0] == 4 (test_gpu_subcoset_transform's (16, 4))
    assert h2g.debug_ntt_plan(16, 1 << 16, in_twist=True)["split"][0] == 4
