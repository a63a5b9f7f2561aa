"""The self-check kernels (csrc/selfcheck.hip) through their seams against the plain-Python
restatement tests/_selfcheck_ref.py (pinned by tests/test_selfcheck_ref_cpu.py).

Shapes: n in {2, 63, 64, 65, 64 * 4 + 1, 5000} -- below, at and above a wave's 64 rows, past one
256-thread block, and enough rows for several grid-stride passes once max_blocks caps the grid
at 1 or 2 blocks -- with u in {1, n - 6, n - 1} where that is a valid row count.  Faults go in
at the rows where a wave, a block or the argument begins and ends."""
import numpy as np
import pytest

import _selfcheck_ref as S
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

R = S.R
NS = [2, 63, 64, 65, 64 * 4 + 1, 5000]
BLOCKS = [1, 2, 0]
FAULT_ROWS = [0, 1, 62, 63, 64, 65]


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()


def us(n):
    return sorted({u for u in (1, n - 6, n - 1) if 1 <= u < n})


def rand_ints(rng, count):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(count)]


def dev(vals):
    return h2g.DevBuf.from_array(hc.ints_to_mont(vals))


def mont1(v):
    return hc.ints_to_mont([v])[0]


class Product:
    """one random argument of u rows on the device: the reference's z, and the seam on any z"""

    def __init__(self, n, u, two, seed):
        rng = np.random.default_rng([n, u, int(two), seed])
        self.n, self.u, self.two = n, u, two
        self.beta, self.gamma = rand_ints(rng, 2)
        self.cols = [rand_ints(rng, u) for _ in range(4 if two else 2)]
        if two:
            self.num_a, self.num_b, self.den_a, self.den_b = self.cols
        else:
            (self.num_a, self.den_a), self.num_b, self.den_b = self.cols, None, None
        self.z = S.make_product(self.num_a, self.num_b, self.den_a, self.den_b, self.beta, self.gamma, u, n,
                                filler=12345)
        self.z[u] = 1   # as a satisfied argument closes (random arrays do not)
        self.fix_last()
        self.d = {k: dev(getattr(self, k)) for k in ("num_a", "num_b", "den_a", "den_b") if getattr(self, k)}
        self.d_z = h2g.DevBuf(32 * n)

    def fix_last(self):
        """choose the last numerator so that the product reaches z[u] = 1 by its recurrence"""
        u, ca = self.u, (self.beta if self.two else self.gamma)
        den = self.den_a[u - 1] + ca
        if self.two:
            den = den * (self.den_b[u - 1] + self.gamma) % R
            den = den * pow((self.num_b[u - 1] + self.gamma) % R, -1, R) % R
        # z[u] = z[u-1] (num_a + ca) [..] / den = 1
        self.num_a[u - 1] = (den * pow(self.z[u - 1], -1, R) - ca) % R

    def want(self, z):
        return S.product_check(z, self.num_a, self.num_b, self.den_a, self.den_b, self.beta, self.gamma, self.u)

    def run(self, z, max_blocks=0, cap=None):
        self.d_z.upload(hc.ints_to_mont(z))
        p = lambda k: self.d[k].ptr if k in self.d else None
        return h2g.debug_selfcheck_product_dev(self.d_z.ptr, p("num_a"), p("num_b"), p("den_a"), p("den_b"),
                                               mont1(self.beta), mont1(self.gamma), self.n, self.u, max_blocks,
                                               cap=len(z) + 8 if cap is None else cap)

    def close(self):
        for b in self.d.values():
            b.close()
        self.d_z.close()


def agree(arg, z, max_blocks):
    want = arg.want(z)
    total, recs = arg.run(z, max_blocks)
    assert total == len(want)
    assert recs == sorted(want)
    return want


@pytest.mark.parametrize("two", [True, False], ids=["two-factor", "one-factor"])
@pytest.mark.parametrize("n", NS)
def test_product_against_the_restatement(n, two):
    for u in us(n):
        arg = Product(n, u, two, seed=1)
        rows = sorted({r for r in FAULT_ROWS + [u - 1, u] if 0 <= r <= u})
        for mb in BLOCKS:
            assert agree(arg, arg.z, mb) == set()          # a correct product: no records
        for k, r in enumerate(rows):                        # one fault at a time
            z = list(arg.z)
            z[r] = (z[r] + 1 + r) % R
            want = agree(arg, z, BLOCKS[k % len(BLOCKS)])
            assert (S.PRODUCT, 0, r) in want and len(want) <= 2
        z = list(arg.z)                                     # all of them together
        for r in rows:
            z[r] = (z[r] + 1 + r) % R
        for mb in BLOCKS:
            assert len(agree(arg, z, mb)) >= len(rows)
        if u + 1 < n:                                       # rows above u are not the argument's
            z = list(arg.z)
            z[u + 1] = 99
            assert agree(arg, z, 0) == set()
        arg.close()


@pytest.mark.parametrize("two", [True, False], ids=["two-factor", "one-factor"])
def test_product_every_row_failing_and_a_small_cap(two):
    n, u = 5000, 4994
    arg = Product(n, u, two, seed=2)
    z = rand_ints(np.random.default_rng(3), n)
    want = arg.want(z)
    assert len(want) == u + 1                               # every recurrence, and the closing value
    for mb in BLOCKS:
        for cap in (0, 1, 64, 100, 4000):
            total, recs = arg.run(z, mb, cap=cap)
            assert total == len(want)                       # exact past the cap
            assert len(recs) == cap and recs == sorted(recs) and len(set(recs)) == cap
            assert set(recs) <= want
    total, recs = arg.run(z, 2, cap=u + 1)
    assert (total, recs) == (u + 1, sorted(want))
    arg.close()


@pytest.mark.parametrize("n", NS)
def test_permuted_pair_against_the_restatement(n):
    for u in us(n) + [n]:
        rng = np.random.default_rng([n, u, 7])
        # runs of repeated values whose first member meets the table side, as the prover lays them
        a, s = [], []
        while len(a) < u:
            v, run = rand_ints(rng, 1)[0], int(rng.integers(1, 5))
            for j in range(run):
                a.append(v)
                s.append(v if j == 0 else rand_ints(rng, 1)[0])
        a, s = a[:u], s[:u]
        assert S.permuted_check(a, s, u) == set()
        d_a, d_s = dev(a), dev(s)

        def agree_pair(aa, ss, mb):
            d_a.upload(hc.ints_to_mont(aa))
            d_s.upload(hc.ints_to_mont(ss))
            want = S.permuted_check(aa, ss, u)
            total, recs = h2g.debug_selfcheck_permuted_dev(d_a.ptr, d_s.ptr, u, mb, cap=u + 8)
            assert (total, recs) == (len(want), sorted(want))
            return want

        for mb in BLOCKS:
            assert agree_pair(a, s, mb) == set()
        rows = sorted({r for r in FAULT_ROWS + [u - 2, u - 1] if 0 <= r < u})
        for k, r in enumerate(rows):                        # a stray value in A'
            aa = list(a)
            aa[r] = (aa[r] + 1) % R
            assert (S.PERMUTED_PAIR, 0, r) in agree_pair(aa, s, BLOCKS[k % 3])
        aa = [(v + 1 + i) % R if i in rows else v for i, v in enumerate(a)]   # (+ i: neighbours stay apart)
        for mb in BLOCKS:
            assert len(agree_pair(aa, s, mb)) >= len(rows)
        ss = list(s)                                        # a wrong first table value: row 0 only
        ss[0] = (ss[0] + 1) % R
        assert agree_pair(a, ss, 1) == {(S.PERMUTED_PAIR, 0, 0)}
        d_a.close()
        d_s.close()


def test_permuted_pair_every_row_failing_and_a_small_cap():
    u = 5000
    rng = np.random.default_rng(11)
    a, s = rand_ints(rng, u), rand_ints(rng, u)
    d_a, d_s = dev(a), dev(s)
    for mb in BLOCKS:
        for cap in (0, 3, 64, 4999):
            total, recs = h2g.debug_selfcheck_permuted_dev(d_a.ptr, d_s.ptr, u, mb, cap=cap)
            assert total == u and len(recs) == cap and len(set(recs)) == cap
            assert all(k == S.PERMUTED_PAIR and i == 0 and r < u for k, i, r in recs)
    d_a.close()
    d_s.close()


class PermSet:
    """one column set of m columns over u rows: random values, sigma and z built by the recurrence"""

    def __init__(self, m, u, seed, first=None):
        rng = np.random.default_rng([m, u, seed])
        self.m, self.u, self.first = m, u, first
        self.beta, self.gamma = rand_ints(rng, 2)
        self.omega = pow(7, (R - 1) >> 20, R)                   # some element of large order
        self.delta = [pow(5, c + 3, R) for c in range(m)]
        self.v = [rand_ints(rng, u) for _ in range(m)]
        self.sig = [rand_ints(rng, u) for _ in range(m)]
        z, w = [1 if first is None else first], 1
        for i in range(u):
            num = den = 1
            for c in range(m):
                num = num * (self.v[c][i] + self.beta * self.delta[c] % R * w + self.gamma) % R
                den = den * (self.v[c][i] + self.beta * self.sig[c][i] + self.gamma) % R
            z.append(z[-1] * num % R * pow(den, -1, R) % R)
            w = w * self.omega % R
        self.z = z
        self.d_v, self.d_s = [dev(c) for c in self.v], [dev(c) for c in self.sig]
        self.d_z = h2g.DevBuf(32 * (u + 1))

    def want(self, z, first=None):
        f = (1 if self.first is None else self.first) if first is None else first
        return S.permutation_check(z, f, self.v, self.sig, self.beta, self.gamma, self.delta, self.omega, self.u)

    def run(self, z, first="own", cap=None):
        f = self.first if first == "own" else first
        self.d_z.upload(hc.ints_to_mont(z))
        return h2g.debug_selfcheck_permutation_dev(
            self.d_z.ptr, None if f is None else mont1(f), [b.ptr for b in self.d_v], [b.ptr for b in self.d_s],
            hc.ints_to_mont(self.delta), mont1(self.beta), mont1(self.gamma), mont1(self.omega), self.u,
            cap=self.u + 8 if cap is None else cap)

    def close(self):
        for b in self.d_v + self.d_s + [self.d_z]:
            b.close()


@pytest.mark.parametrize("m", [1, 3, 8, 9, 17])   # 8: a full launch; 9, 17: two and three launches, carried products
def test_permutation_set_against_the_restatement(m):
    for u, first in ((1, None), (65, None), (300, 12345), (5000 if m <= 3 else 700, None)):
        arg = PermSet(m, u, seed=5, first=first)
        assert arg.want(arg.z) == set()
        assert arg.run(arg.z) == (0, [])                                  # a correct set: no records
        rows = sorted({r for r in FAULT_ROWS + [u - 1, u] if 0 <= r <= u})
        for r in rows:                                                     # one wrong z at a time
            z = list(arg.z)
            z[r] = (z[r] + 1 + r) % R
            want = arg.want(z)
            assert {w[2] for w in want} == {x for x in (r - 1, r) if 0 <= x < u}
            assert arg.run(z) == (len(want), sorted(want))
        z = [(v + 1 + i) % R if i in rows else v for i, v in enumerate(arg.z)]
        want = arg.want(z)
        assert arg.run(z) == (len(want), sorted(want)) and len(want) >= len(rows) - 1
        # the chaining: the same z against another starting value fails row 0 only
        other = 777 if first is None else None
        want = arg.want(arg.z, first=1 if other is None else other)
        assert want == {(S.PERMUTATION, 0, 0)}
        assert arg.run(arg.z, first=other) == (1, [(S.PERMUTATION, 0, 0)])
        # one wrong value in the last column (a carried launch's, for m > 8) fails its row
        r = u // 2
        old = arg.v[m - 1][r]
        arg.v[m - 1][r] = (old + 1) % R
        arg.d_v[m - 1].upload(hc.ints_to_mont(arg.v[m - 1]))
        want = arg.want(arg.z)
        assert want == {(S.PERMUTATION, 0, r)}
        assert arg.run(arg.z) == (1, sorted(want))
        arg.close()


def test_permutation_set_every_row_failing_and_a_small_cap():
    arg = PermSet(9, 3000, seed=6)
    z = rand_ints(np.random.default_rng(8), 3001)
    z[0] = 2
    for cap in (0, 5, 2999):
        total, recs = arg.run(z, cap=cap)
        assert total == 3000 and len(recs) == cap and len(set(recs)) == cap
        assert all(k == S.PERMUTATION and i == 0 and r < 3000 for k, i, r in recs)
    arg.close()


def test_seam_argument_errors():
    d = h2g.DevBuf(32 * 8)
    one = mont1(1)
    for n, u in ((1, 1), (8, 0), (8, 8), (8, 9)):
        with pytest.raises(h2g.H2GError, match="h2g error 1"):
            h2g.debug_selfcheck_product_dev(d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, one, one, n, u)
    with pytest.raises(h2g.H2GError, match="h2g error 1"):   # one factor of the second pair only
        h2g.debug_selfcheck_product_dev(d.ptr, d.ptr, d.ptr, d.ptr, None, one, one, 8, 5)
    with pytest.raises(h2g.H2GError, match="h2g error 1"):
        h2g.debug_selfcheck_product_dev(d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, one, one, 8, 5, max_blocks=-1)
    with pytest.raises(h2g.H2GError, match="h2g error 1"):
        h2g.debug_selfcheck_permuted_dev(d.ptr, d.ptr, 0)
    d.close()
