"""The asm-block F29 products and the in-register lane exchange on the device, against the C
oracle, exact equality.

The NTT passes take their products from f29.h's block forms (a pair block per two
independent products) and exchange lanes with v_permlane32_swap / v_permlane16_swap / a DPP
row rotation; the MSM accumulation's mixed addition is ten blocks.  The interpreter test
(tests/test_f29_asm_cpu.py) proves the blocks' text; this file runs what the compiler made
of them around that text -- operand allocation, the exchange's lane and register pairing --
at transforms of 2^12 .. 2^17 points, whose splits put 3-, 4-, 5- and 6-bit passes first, 4-,
5- and 6-bit passes in the persistent middle kernel and the 6-bit pass last.  Besides a random
and an all-(r - 1) vector every unit impulse at a position 2^j goes through each map: a
single nonzero input reaches an output through exactly one lane or register bit per exchange.
"""
import functools

import numpy as np
import pytest

import _ntt_shapes as S
import _oracle as O
import h2g

pytestmark = pytest.mark.gpu

LOGS = [12, 13, 14, 15, 16, 17]


@pytest.fixture(scope="module", autouse=True)
def engine():
    h2g.init()
    yield
    h2g.shutdown()


def test_the_sizes_cover_every_pass_width():
    first, middle, last = set(), set(), set()
    for L in LOGS:
        for twist in (False, True):
            pl = h2g.debug_ntt_plan(L, 1 << L, 1 << L, count=3 if twist else 1, in_twist=twist)
            split = pl["split"]
            first.add(split[0])
            middle |= {split[p] for p in pl["pgrid"]}
            last.add(split[-1])
    assert first == {3, 4, 5, 6} and middle == {4, 5, 6} and last == {6}, (first, middle, last)


@functools.lru_cache(maxsize=None)
def vectors(log_n):
    """random, every stored integer r - 1, and the unit impulses at 2^j, j < log_n"""
    n = 1 << log_n
    one = O.fr_from_canonical(np.array([[1, 0, 0, 0]], dtype=np.uint64))[0]
    out = [("random", S.vector("random", n, seed=log_n)), ("rm1", S.vector("storage_rm1", n))]
    for j in range(log_n):
        v = np.zeros((n, 4), dtype=np.uint64)
        v[1 << j] = one
        out.append(("impulse 2^%d" % j, v))
    for _, v in out:
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("L", LOGS)
def test_fft_and_lagrange_to_coeff(L):
    _, consts, _ = O.domain_constants(2, L)
    d = h2g.Domain(3, L)
    try:
        for name, a in vectors(L):
            assert np.array_equal(h2g.fft(a, consts[0]), O.fft(a, consts[0], 8)), (L, name)
            assert np.array_equal(d.lagrange_to_coeff(a), O.lagrange_to_coeff(a, 3, L, 8)), (L, name)
    finally:
        d.close()


@pytest.mark.parametrize("j,e", [(3, 1), (5, 2)])
@pytest.mark.parametrize("L", LOGS)
def test_coset_extension_and_back(L, j, e):
    """the 2x (j = 3) and 4x (j = 5) extensions into 2^L points and extended_to_coeff of 2^L"""
    k = L - e
    d = h2g.Domain(j, k)
    try:
        assert d.extended_k == L
        for name, a in vectors(k):
            ext = d.coeff_to_extended(a)
            assert np.array_equal(ext, O.coeff_to_extended(a, j, k, 8)), (L, j, name)
        for name, h in vectors(L):
            assert np.array_equal(d.extended_to_coeff(h), O.extended_to_coeff(h, j, k, 8)), (L, j, name)
    finally:
        d.close()


@pytest.mark.parametrize("L", LOGS)
def test_three_column_batches(L):
    """sub-coset transforms of three columns at once -- the only maps that take the twisted
    first pass (ntt_pass29_kernel<M, true>), here beside the persistent passes over a batch:
    random, r - 1 and an impulse side by side, every impulse 2^j in turn, on both sub-cosets"""
    d = h2g.Domain(3, L)
    try:
        vs = vectors(L)
        rnd, rm1 = vs[0][1], vs[1][1]
        want = {name: O.coeff_to_extended(a, 3, L, 8) for name, a in vs}  # once per vector
        for name, imp in vs[2:]:
            for t in (0, 1):
                got = d.coeff_to_subcoset([rnd, imp, rm1], t)
                for g, nm in zip(got, ("random", name, "rm1")):
                    assert g.tobytes() == np.ascontiguousarray(want[nm][t::2]).tobytes(), (L, name, nm, t)
    finally:
        d.close()


def _scalars(kind, n, r):
    if kind == "random":
        return O.random_fr(r, n)
    if kind == "ones":
        return O.fr_from_canonical(np.tile(np.array([1, 0, 0, 0], dtype=np.uint64), (n, 1)))
    return np.tile(O.fr_from_canonical(S.R_MINUS_1.copy())[0], (n, 1))  # the element r - 1


@pytest.fixture(scope="module")
def bases():
    """3000 distinct points, and 3000 points that are three points repeated (equal points
    meet in a bucket: the accumulation's doubling case and its repair)"""
    n = 3000
    d = h2g.DevBuf(n * 64)
    try:
        h2g.srs_setup_dev(O.random_fr(np.random.default_rng(5), 1)[0], n, d.ptr)
        distinct = d.download((n, 8))
    finally:
        d.close()
    return {"distinct": distinct, "repeated": np.tile(distinct[:3], (n // 3, 1)).copy()}


@pytest.mark.parametrize("pts", ["distinct", "repeated"])
@pytest.mark.parametrize("kind", ["random", "rminus1", "ones"])
def test_msm_generic_and_fixed_base(bases, kind, pts):
    b = bases[pts]
    sc = _scalars(kind, len(b), np.random.default_rng(len(kind)))
    want = O.msm_best(sc, b, 8)
    assert np.array_equal(h2g.msm(sc, b), want), (kind, pts)
    hb = h2g.base_descriptor(b)
    try:
        assert np.array_equal(h2g.msm_with_cached_base(sc, hb), want), (kind, pts, "fixed base")
    finally:
        h2g.descriptor_free(hb)
