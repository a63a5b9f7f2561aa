"""The NTT's truncated, sparse and ragged paths at multi-pass sizes, against the C oracle,
exact equality.

What the other NTT tests' shapes leave out (every Domain(j, k) they build above 2^10 points
has j - 1 a power of two, and every batch at size has 1 or 8 transforms):
  * ntt_last29_kernel<true, false>, the truncated last pass of extended_to_coeff: stores
    under y < out_len and the epilogue product per y mod 3.  Needs out_len = n (j - 1) <
    2^extended_k, so j - 1 no power of two, and extended_k > 10.  The host wrapper copies
    out_len elements back, so a store past the truncation shows in the guard test only.
  * ntt_first_sparse29_kernel with x[1] all zero (an 8n extension) and with half of x[0]
    zero as well (16n).
  * ntt_pass29p_kernel with a grid that does not divide its items (batches of 5 and 7).
A shape's variant is not a comment: it is read from the library's plan (_ntt_shapes.require,
h2g.debug_ntt_plan), and tests/test_ntt_plan_cpu.py pins the rule itself.
"""
import functools

import numpy as np
import pytest

import _ntt_shapes as S
import _oracle as O
import h2g

pytestmark = pytest.mark.gpu

CASES = sorted(S.CASES, key=lambda c: (S.CASES[c][0], c))


@pytest.fixture(scope="module", autouse=True)
def engine():
    h2g.init()
    yield
    h2g.shutdown()


@functools.lru_cache(maxsize=None)
def _random_h(j, k):
    """a random extended-domain vector and the oracle's extended_to_coeff of it, once per shape"""
    h = S.vector("random", 1 << S.extended_k(j, k), seed=1000 * j + k)
    want = O.extended_to_coeff(h, j, k, 8)
    h.setflags(write=False)
    want.setflags(write=False)
    return h, want


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("j,k", CASES)
def test_domain_maps_vs_oracle(j, k, kind):
    S.require(j, k)
    d = h2g.Domain(j, k)
    try:
        n, N, out_len = d.n, d.extended_len, d.n * (j - 1)
        assert d.extended_k == S.CASES[(j, k)][0] and out_len < N
        a = S.vector(kind, n, seed=100 * j + k)
        assert np.array_equal(d.lagrange_to_coeff(a), O.lagrange_to_coeff(a, j, k, 8))
        ext = d.coeff_to_extended(a)
        assert np.array_equal(ext, O.coeff_to_extended(a, j, k, 8))
        if kind == "random":
            h, want = _random_h(j, k)
        else:
            h = S.vector(kind, N)
            want = O.extended_to_coeff(h, j, k, 8)
        got = d.extended_to_coeff(h)
        assert got.shape == (out_len, 4) and np.array_equal(got, want)
        assert np.array_equal(d.divide_by_vanishing_poly(h), O.divide_by_vanishing_poly(h, j, k))
        # the round trip: the polynomial's n coefficients (every vector is a reduced stored
        # integer, so they come back as they went), then zeros up to the truncation
        back = d.extended_to_coeff(ext)
        assert np.array_equal(back[:n], a)
        assert back.shape == (out_len, 4) and not back[n:].any()
    finally:
        d.close()


@pytest.mark.parametrize("j,k", CASES)
def test_nothing_is_stored_behind_the_truncation(j, k):
    """extended_to_coeff into a device buffer of 2^extended_k elements that the test owns to its
    end, filled with a sentinel: [0, out_len) is the oracle's result, [out_len, 2^extended_k)
    is untouched.  A wrong store predicate changes a sentinel; it cannot leave the buffer."""
    S.require(j, k)
    d = h2g.Domain(j, k)
    try:
        N, out_len = d.extended_len, d.n * (j - 1)
        h, want = _random_h(j, k)
        sentinel = (np.arange(4 * N, dtype=np.uint64).reshape(N, 4) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1 << 63)
        src, dst = h2g.DevBuf.from_array(h), h2g.DevBuf.from_array(sentinel)
        try:
            h2g.check(h2g.lib().h2g_extended_to_coeff_dev(d.h, src.ptr, dst.ptr, None))
            got = dst.download((N, 4))
            assert src.download((N, 4)).tobytes() == h.tobytes()  # the input is left alone
        finally:
            src.close()
            dst.close()
        assert np.array_equal(got[out_len:], sentinel[out_len:]), np.flatnonzero((got != sentinel).any(axis=1)
                                                                                 [out_len:])[:8] + out_len
        assert np.array_equal(got[:out_len], want)
    finally:
        d.close()


@pytest.mark.parametrize("count", [5, 7])
def test_persistent_pass_with_a_ragged_tail(count):
    """Domain(3, 18), sub-coset transforms in batches of 5 and 7: 128 blocks of items against a
    persistent grid of 2 CUs / count blocks, so some waves walk one item more than others
    (count = 1 and 8, the batches the other tests have at this size, always divide)."""
    j, k = 3, 18
    pl = h2g.debug_ntt_plan(k, 1 << k, 1 << k, count=count, in_twist=True, cus=0, epilogue_one=True)
    assert pl["split"] == (6, 6, 6) and pl["first"] == "twisted" and pl["blocks"] == 128
    grid = pl["pgrid"][1]
    assert grid < pl["blocks"] and pl["blocks"] % grid, ("the grid divides the items: not ragged", pl)
    d = h2g.Domain(j, k)
    try:
        assert d.extended_k - d.k == 1
        kinds = ["random", "storage_rm1", "random", "spike_last", "random", "alternating_canonical", "zero"]
        polys = [S.vector(kind, d.n, seed=50 + i) for i, kind in enumerate(kinds)][:count]
        ext = [d.coeff_to_extended(p) for p in polys]  # pinned to the oracle by test_gpu_parity at (3, 18)
        for t in (0, 1):
            got = d.coeff_to_subcoset(polys, t)
            for i in range(count):
                assert got[i].tobytes() == np.ascontiguousarray(ext[i][t::2]).tobytes(), (count, t, i)
                alone = d.coeff_to_subcoset([polys[i]], t)
                assert alone[0].tobytes() == got[i].tobytes(), (count, t, i, "count 1")
    finally:
        d.close()
