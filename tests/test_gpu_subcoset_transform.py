"""Domain.coeff_to_subcoset: sub-coset t of a polynomial's extended coset by one n-point
transform whose first pass forms the twist w_ext^(t j) zeta^(j mod 3) itself.

The reference is Domain.coeff_to_extended(a)[t::2^e] (pinned to the oracle by
test_gpu_parity / the golden fixtures): row t + 2^e m of the extended coset is the point
zeta w_ext^t w^m.  Outputs are compared as bytes -- fully reduced limbs, not values mod r.

Sizes: k = 6 and 10 are the one-block kernel and its upper edge; k = 11 two passes with the
short (5-bit) pass first; k = 13 the borrowed-bits split 3 + 4 + 6; k = 16 the split
4 + 6 + 6 (the twisted first pass of 4 bits); k = 18 three 6-bit passes with the persistent
middle pass.  Extended domains 2n and 16n at k = 6, 10, 13 and 4n at k = 11, 16 and 18; every t
of each.
"""
import numpy as np
import pytest

import _oracle as O
import h2g

pytestmark = pytest.mark.gpu

R_MINUS_1 = np.array([0x43e1f593f0000000, 0x2833e84879b97091, 0xb85045b68181585d, 0x30644e72e131a029],
                     dtype=np.uint64)  # the largest stored integer

ERR_ARG = 1  # H2G_ERR_ARG

# (k, j): extended_k - k = ceil(log2(j - 1))
# (16, 4): the twisted first pass at lg[0] == 4 (the split 4 + 6 + 6), a 4n extension of three pieces
CASES = [(6, 3), (6, 17), (10, 3), (10, 17), (11, 5), (13, 3), (13, 17), (18, 5), (16, 4)]


@pytest.fixture(scope="module", autouse=True)
def engine():
    h2g.init()
    yield
    h2g.shutdown()


def _inputs(n, seed):
    """nine polynomials: six random, all r - 1, one spike at j = n - 1, all zero"""
    r = np.random.default_rng(seed)
    polys = [O.random_fr(r, n) for _ in range(6)]
    polys.append(np.tile(R_MINUS_1, (n, 1)))
    spike = np.zeros((n, 4), dtype=np.uint64)
    spike[n - 1] = O.random_fr(r, 1)[0]
    polys.append(spike)
    polys.append(np.zeros((n, 4), dtype=np.uint64))
    return polys


@pytest.mark.parametrize("k,j", CASES)
def test_subcoset_equals_rows_of_extended(k, j):
    d = h2g.Domain(j, k)
    try:
        e = d.extended_k - d.k
        assert (1 << e) >= j - 1 > (1 << e) // 2
        polys = _inputs(d.n, 100 * k + j)
        ext = [d.coeff_to_extended(p) for p in polys]  # the reference, once
        for t in range(1 << e):
            want = [x[t::1 << e] for x in ext]
            got9 = d.coeff_to_subcoset(polys, t)  # 9: crosses NTT_MAX_BATCH
            for i in range(9):
                assert got9[i].tobytes() == np.ascontiguousarray(want[i]).tobytes(), (k, j, t, i)
            got8 = d.coeff_to_subcoset(polys[1:], t)
            assert got8.tobytes() == got9[1:].tobytes(), (k, j, t, "count 8")
            for i in (0, 6, 7, 8):
                got1 = d.coeff_to_subcoset([polys[i]], t)
                assert got1[0].tobytes() == got9[i].tobytes(), (k, j, t, i, "count 1")
        assert not got9[8].any()  # the zero polynomial
    finally:
        d.close()


def _ptrs(arrs):
    return (h2g.VP * len(arrs))(*[a.ctypes.data for a in arrs])


@pytest.mark.parametrize("k", [6, 13])
def test_subcoset_argument_errors(k):
    d = h2g.Domain(5, k)
    try:
        a = O.random_fr(np.random.default_rng(3), d.n)
        b = O.random_fr(np.random.default_rng(4), d.n)
        out = np.zeros((2, d.n, 4), dtype=np.uint64)
        lib = h2g.lib()
        E = 1 << (d.extended_k - d.k)
        # t = 2^e is past the last sub-coset
        assert lib.h2g_coeff_to_subcoset(d.h, _ptrs([a, b]), 2, E, _ptrs([out[0], out[1]])) == ERR_ARG
        # in place, and an output over another polynomial of the call
        assert lib.h2g_coeff_to_subcoset(d.h, _ptrs([a]), 1, 0, _ptrs([a])) == ERR_ARG
        assert lib.h2g_coeff_to_subcoset(d.h, _ptrs([a, b]), 2, 1, _ptrs([out[0], a])) == ERR_ARG
        with pytest.raises(h2g.H2GError):
            d.coeff_to_subcoset([a], E)
        # the device-pointer form refuses the same
        buf = h2g.DevBuf(2 * d.n * 32)
        try:
            p0, p1 = buf.ptr, buf.ptr + d.n * 32
            one = lambda *v: (h2g.VP * len(v))(*v)
            assert lib.h2g_coeff_to_subcoset_dev(d.h, one(p0), 1, 0, one(p0), None) == ERR_ARG
            assert lib.h2g_coeff_to_subcoset_dev(d.h, one(p0), 1, E, one(p1), None) == ERR_ARG
            assert lib.h2g_coeff_to_subcoset_dev(d.h, one(p0, p0), 2, 0, one(p1, p1), None) == ERR_ARG
        finally:
            buf.close()
        # and none of that disturbed the domain
        assert d.coeff_to_subcoset([a], 1)[0].tobytes() == np.ascontiguousarray(d.coeff_to_extended(a)[1::E]).tobytes()
    finally:
        d.close()


def test_subcoset_dev_on_device_buffers():
    """the device-pointer seam, as a caller with resident polynomials uses it"""
    k, j = 11, 9
    d = h2g.Domain(j, k)
    try:
        E = 1 << (d.extended_k - d.k)
        polys = _inputs(d.n, 7)[:3]
        nb = d.n * 32
        src = h2g.DevBuf(3 * nb)
        dst = h2g.DevBuf(3 * nb)
        try:
            src.upload(np.concatenate(polys))
            sp = (h2g.VP * 3)(*[src.ptr + i * nb for i in range(3)])
            dp = (h2g.VP * 3)(*[dst.ptr + i * nb for i in range(3)])
            for t in (0, E - 1):
                h2g.check(h2g.lib().h2g_coeff_to_subcoset_dev(d.h, sp, 3, t, dp, None))
                got = dst.download((3, d.n, 4))
                for i in range(3):
                    want = np.ascontiguousarray(d.coeff_to_extended(polys[i])[t::E])
                    assert got[i].tobytes() == want.tobytes(), (t, i)
                # and the composition it replaces (a twist launch per column, then the NTT)
                h2g.check(h2g.lib().h2g_debug_coeff_to_subcoset_unfused_dev(d.h, sp, 3, t, dp, None))
                assert dst.download((3, d.n, 4)).tobytes() == got.tobytes(), t
        finally:
            src.close()
            dst.close()
    finally:
        d.close()
