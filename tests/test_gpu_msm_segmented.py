"""h2g_msm_segmented / _dev (csrc/msm_seg.hip) against oracle/py/bn254_ref.py.

The bases are known multiples of the generator, B_i = [b0 + i d] G (built with g1_add), so a
segment's expected sum is one g1_mul: [sum_j s_j (b0 + index_j d) mod r] G.  Identity bases
and negated bases are placed by hand.  One call covers the segment lengths 0, 1, 2, 63, 64,
65 (around the 64-lane wave), 257 (more than the 128-thread group: lanes take several terms)
and 1100, the scalars 0, 1 and r - 1, a base listed twice, a base with its negation, and an
all-zero segment; every other test reuses its inputs.
"""
import numpy as np
import pytest

import bn254_ref as B
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

R = B.R
B0, D = 0x1234567890ABCDEF0FEDCBA987654321 % R, 0xDEADBEEFCAFEF00D5EED
NB = 1700                       # plain bases B_0 .. B_{NB-1}
IDENT, NEG7 = NB, NB + 1        # then an identity base and -B_7
LENS = [0, 1, 2, 63, 64, 65, 257, 1100]


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield


@pytest.fixture(scope="module")
def world():
    """(bases array, mult) -- mult[i]: B_i = [mult[i]] G (0 for the identity)"""
    step = B.g1_mul(B.G1_GEN, D)
    pts = [B.g1_mul(B.G1_GEN, B0)]
    for _ in range(NB - 1):
        pts.append(B.g1_add(pts[-1], step))
    mult = [(B0 + i * D) % R for i in range(NB)] + [0, (-(B0 + 7 * D)) % R]
    pts += [None, B.g1_neg(pts[7])]
    bases = np.array([B.g1_affine_mont_limbs(p) for p in pts], dtype=np.uint64)
    return bases, mult


def expected(mult, scalars, index, seg_off):
    out = []
    for s in range(len(seg_off) - 1):
        k = sum(scalars[j] * mult[index[j]] for j in range(seg_off[s], seg_off[s + 1])) % R
        out.append(B.g1_affine_mont_limbs(B.g1_mul(B.G1_GEN, k)))
    return np.array(out, dtype=np.uint64).reshape(-1, 8)


def edge_call(rng):
    """scalars (ints), index, seg_off of the one call with every edge case"""
    sc, ix, off = [], [], [0]

    def seg(terms):
        for s, i in terms:
            sc.append(s % R)
            ix.append(i)
        off.append(len(sc))

    rnd = lambda: int.from_bytes(rng.bytes(32), "little") % R  # noqa: E731
    for n in LENS:                                        # random scalars, indices shared across segments
        seg([(rnd(), int(rng.integers(NB))) for _ in range(n)])
    seg([(0, 3), (1, 4), (R - 1, 5), (rnd(), IDENT)])     # scalars 0, 1, r - 1; an identity base
    seg([(5, 9), (5, 9)])                                 # a base twice, equal scalars: P + P in the tree
    s = rnd()
    seg([(s, 7), (s, NEG7)])                              # a base and its negation: the identity
    seg([(0, int(rng.integers(NB))) for _ in range(70)])  # an all-zero segment
    seg([(rnd(), IDENT)] * 3)                             # only identity bases
    seg([(R - 1, 11)] * 130)                              # one base 130 times: doublings at every tree level
    return sc, ix, off


@pytest.fixture(scope="module")
def edge(world):
    bases, mult = world
    sc, ix, off = edge_call(np.random.default_rng(77))
    return sc, ix, off, expected(mult, sc, ix, off)


def test_edge_cases_host_entry(world, edge):
    bases, _ = world
    sc, ix, off, want = edge
    got = h2g.msm_segmented(bases, hc.ints_to_mont(sc), off, index=ix)
    assert got.shape == want.shape
    for s in range(len(want)):
        assert np.array_equal(got[s], want[s]), f"segment {s} (terms {off[s]}..{off[s + 1]})"
    # the identities really are all-zero limbs
    assert not got[0].any() and not got[len(LENS) + 2].any() and not got[len(LENS) + 3].any()


def test_dev_entry_agrees_with_host(world, edge):
    bases, _ = world
    sc, ix, off, want = edge
    d_b = h2g.DevBuf.from_array(bases)
    d_s = h2g.DevBuf.from_array(hc.ints_to_mont(sc))
    d_i = h2g.DevBuf.from_array(np.asarray(ix, dtype=np.uint32))
    d_o = h2g.DevBuf.from_array(np.asarray(off, dtype=np.uint32))
    nseg = len(off) - 1
    d_out = h2g.DevBuf(nseg * 64)
    h2g.msm_segmented_dev(d_b.ptr, len(bases), d_s.ptr, d_i.ptr, d_o.ptr, nseg, d_out.ptr)
    h2g.check(h2g.lib().h2g_synchronize())
    assert np.array_equal(d_out.download((nseg, 8)), want)
    for b in (d_b, d_s, d_i, d_o, d_out):
        b.close()


def test_null_index_and_one_segment(world):
    """index NULL: term j uses base j; nseg = 1; also on the device entry point"""
    bases, mult = world
    rng = np.random.default_rng(5)
    n = 300
    sc = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]
    want = expected(mult, sc, list(range(n)), [0, n])
    got = h2g.msm_segmented(bases, hc.ints_to_mont(sc), [0, n])
    assert np.array_equal(got, want)
    # several segments over consecutive bases, the first offset past 0
    off = [10, 10, 74, 75, 300]
    got = h2g.msm_segmented(bases, hc.ints_to_mont(sc), off)
    assert np.array_equal(got, expected(mult, sc, list(range(n)), off))
    d_b = h2g.DevBuf.from_array(bases)
    d_s = h2g.DevBuf.from_array(hc.ints_to_mont(sc))
    d_o = h2g.DevBuf.from_array(np.asarray([0, n], dtype=np.uint32))
    d_out = h2g.DevBuf(64)
    h2g.msm_segmented_dev(d_b.ptr, len(bases), d_s.ptr, None, d_o.ptr, 1, d_out.ptr)
    h2g.check(h2g.lib().h2g_synchronize())
    assert np.array_equal(d_out.download((1, 8)), want)
    for b in (d_b, d_s, d_o, d_out):
        b.close()


def test_300_segments(world):
    bases, mult = world
    rng = np.random.default_rng(300)
    lens = [int(v) for v in rng.integers(0, 6, size=300)]
    off = [0]
    for v in lens:
        off.append(off[-1] + v)
    nnz = off[-1]
    sc = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(nnz)]
    ix = [int(v) for v in rng.integers(0, 40, size=nnz)]     # 40 bases shared by 300 segments
    got = h2g.msm_segmented(bases, hc.ints_to_mont(sc), off, index=ix)
    assert np.array_equal(got, expected(mult, sc, ix, off))


def test_bad_arguments_are_err_arg(world):
    bases, _ = world
    one = hc.ints_to_mont([1, 2, 3])
    for index, off in (([0, 1, len(bases)], [0, 3]),       # an index past the last base
                       ([0, 1, 2], [0, 2, 1])):            # offsets that decrease
        with pytest.raises(h2g.H2GError, match="h2g error 1"):
            h2g.msm_segmented(bases, one, off, index=index)
    with pytest.raises(h2g.H2GError, match="h2g error 1"):   # index NULL: more terms than bases
        h2g.msm_segmented(bases[:2], one, [0, 3])
    # no segments: nothing to do
    assert h2g.msm_segmented(bases, one[:0], [0]).shape == (0, 8)
