"""The tiled scans under the multi-open and the grand products, each compiled variant on its
own and at the lengths where the dispatch changes: kate_division (kate_phase1/2/3 for 8, 16,
32 and 64 coefficients per thread, plain and accumulating, through the seam
h2g_debug_kate_division_dev), poly_eval_batch past 256 blocks (eval_level2 with more than one
partial sum per thread) and poly_batch_invert at 2, 4, 8 and 16 elements per thread.

Every comparison is exact (field elements).  The reference is the C oracle; every case of at
most 4097 coefficients is also compared with Python big integers (oracle/py/bn254_ref.py), so
the oracle functions the large cases rest on -- or_kate_division, or_fr_eval,
or_fr_batch_invert, or_fr_add -- are each pinned against a second reference in this file.

"Storage r - 1" below is the element whose stored (Montgomery) integer is r - 1: the kernels'
Horner chains take stored integers raw, so this, not the Montgomery form of r - 1, is the
largest input their accumulator bounds are stated for.
"""
import numpy as np
import pytest

import _oracle as O
import bn254_ref as B
import h2g

pytestmark = pytest.mark.gpu

R = B.R
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)
ERR_ARG = 1
KD_T = 256            # threads per kate tile
EV_BLK = 16384        # coefficients per eval_level1 block
TILES = (8, 16, 32, 64)
GUARD = 8             # elements kept behind every quotient array, checked untouched
POOL_LEN = 4_186_114 + 8193


def limbs(v):
    return np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


R_LIMBS = limbs(R)
RM1 = limbs(R - 1)                    # storage r - 1
POISON = np.uint64(0xDEADBEEFDEADBEEF)  # >= r in the top limb: never a reduced element


def fr(x):
    return limbs(x % R * MONT % R)


def stored(arr):
    """the stored integers of (n, 4) limbs"""
    raw = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def values(arr):
    """the field elements (canonical integers) of (n, 4) Montgomery limbs"""
    return [v * MONT_INV % R for v in stored(arr)]


def from_stored(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(-1, 4).copy()


def from_values(ints):
    return from_stored([v * MONT % R for v in ints])


def below_r(q):
    lt, eq = np.zeros(len(q), dtype=bool), np.ones(len(q), dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (q[:, i] < R_LIMBS[i])
        eq &= q[:, i] == R_LIMBS[i]
    return bool(lt.all())


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield


@pytest.fixture(scope="module")
def pool():
    """the one random array every test slices (never written)"""
    a = O.random_fr(np.random.default_rng(0x5CA9), POOL_LEN)
    a.setflags(write=False)
    return a


def rand_point():
    return O.random_fr(np.random.default_rng(77), 1)[0]


def points():
    return [("0", fr(0)), ("1", fr(1)), ("r-1", fr(R - 1)), ("rand", rand_point())]


# ----------------------------------------------------------------------------- a. kate division
def kate_inputs(pool, M):
    """(name, a, b): random coefficients and one top coefficient at every point, all storage
    r - 1 at the point storage r - 1"""
    n = M + 1
    top = np.zeros((n, 4), dtype=np.uint64)
    top[-1] = pool[7]
    out = [(f"random@{nm}", pool[:n], b) for nm, b in points()]
    out.append(("rm1@rm1", np.tile(RM1, (n, 1)), RM1))
    out += [(f"top@{nm}", top, b) for nm, b in points()]
    return out


_KATE_REF = {}


def kate_ref(M, name, a, b):
    """O.kate_division, computed once per case; pinned by big integers up to 4097 coefficients"""
    if (M, name) not in _KATE_REF:
        q = O.kate_division(a, b)
        if len(a) <= 4097:
            assert np.array_equal(q, from_values(B.kate_division(values(a), values(b.reshape(1, 4))[0]))), (M, name)
        q.setflags(write=False)
        _KATE_REF[(M, name)] = q
    return _KATE_REF[(M, name)]


def acc_ref(q_old, q):
    want = O.binop("or_fr_add", q_old, q)
    if len(q) <= 4096:  # Montgomery form is linear: the sum of the stored integers mod r
        assert np.array_equal(want, from_stored([(x + y) % R for x, y in zip(stored(q_old), stored(q))]))
    return want


class KateRun:
    """device arrays for one polynomial; run() -> the M quotients one call leaves"""

    def __init__(self, a):
        self.n, self.M = len(a), len(a) - 1
        self.da = h2g.DevBuf.from_array(a)
        self.dq = h2g.DevBuf(32 * (self.M + GUARD))

    def run(self, b, tile_s=0, q_old=None, public=False):
        init = np.full((self.M + GUARD, 4), POISON, dtype=np.uint64)
        if q_old is not None:
            init[:self.M] = q_old
        self.dq.upload(init)
        if public:
            h2g.kate_division_dev(self.da.ptr, self.n, b, self.dq.ptr)
        else:
            h2g.debug_kate_division_dev(self.da.ptr, self.n, b, self.dq.ptr, q_old is not None, tile_s)
        out = self.dq.download((self.M + GUARD, 4))
        assert (out[self.M:] == POISON).all(), "a store past the last quotient"
        return out[:self.M]

    def close(self):
        self.da.close()
        self.dq.close()


def check_kate(pool, M, tile_s, acc):
    rule = h2g.debug_kate_tile_s(M + 1)
    for name, a, b in kate_inputs(pool, M):
        want = kate_ref(M, name, a, b)
        olds = [None]
        if acc:
            olds = [np.ascontiguousarray(pool[POOL_LEN - M:])]
            if name in ("rm1@rm1", "random@rand"):
                olds.append(np.tile(RM1, (M, 1)))
        kr = KateRun(a)
        try:
            for i, q_old in enumerate(olds):
                tag = (M, tile_s, acc, name, i)
                exp = acc_ref(q_old, want) if acc else want
                got = kr.run(b, tile_s, q_old)
                assert np.array_equal(got, exp), tag
                assert below_r(got), tag
                # the rule's choice is the forced variant it names, byte for byte
                by_rule = kr.run(b, 0, q_old)
                assert np.array_equal(by_rule, got if rule == tile_s else kr.run(b, rule, q_old)), tag
                if not acc:
                    assert np.array_equal(kr.run(b, public=True), by_rule), tag
        finally:
            kr.close()


def edge_lengths(tile_s):
    T = KD_T * tile_s
    return sorted({1, 3, 4, 5, tile_s - 1, tile_s, tile_s + 1, T - 1, T, T + 1, 2 * T, 2 * T + 1})


@pytest.mark.parametrize("acc", [0, 1], ids=["assign", "accumulate"])
@pytest.mark.parametrize("tile_s", TILES)
def test_kate_variant_at_its_tile_edges(pool, tile_s, acc):
    """kate_phase1<S> / kate_phase3<S, ACC> at M = len - 1 around one thread's run (S), one
    tile (256 S) and two tiles: the j < M predicates, the KD_SUB staging runs, the level
    weights pw.p[l] = b^(S 2^l) and the one-tile / two-tile carries"""
    for M in edge_lengths(tile_s):
        check_kate(pool, M, tile_s, acc)


@pytest.mark.parametrize("tiles", [257, 258])
def test_kate_phase2_two_tiles_per_thread(pool, tiles):
    """M = 256 T + 1 and 257 T + 1 at S = 8 (T = 2048): 257 and 258 tiles, so kate_phase2's
    threads take per = 2 tiles each and the last thread groups are partly / wholly empty"""
    M = (tiles - 1) * KD_T * 8 + 1
    assert -(-M // (KD_T * 8)) == tiles
    for acc in (0, 1):
        check_kate(pool, M, 8, acc)
    for key in [k for k in _KATE_REF if k[0] == M]:
        del _KATE_REF[key]


def test_kate_seam_argument_errors(pool):
    kr = KateRun(pool[:9])
    b = rand_point()
    try:
        for bad in (-8, 1, 4, 7, 9, 24, 48, 128):
            with pytest.raises(h2g.H2GError) as e:
                h2g.debug_kate_division_dev(kr.da.ptr, 9, b, kr.dq.ptr, False, bad)
            assert int(str(e.value).split()[2].rstrip(":")) == ERR_ARG
        for args in ((kr.da.ptr + 8, 9, b, kr.dq.ptr), (kr.da.ptr, 9, b, kr.dq.ptr + 8), (kr.da.ptr, 0, b, kr.dq.ptr)):
            with pytest.raises(h2g.H2GError) as e:
                h2g.debug_kate_division_dev(*args, False, 8)
            assert int(str(e.value).split()[2].rstrip(":")) == ERR_ARG
    finally:
        kr.close()


# ----------------------------------------------------------------------------- b. the size rule at its thresholds
@pytest.mark.parametrize("length,tile_s", [(2_093_057, 8), (2_093_058, 16), (2_093_058 + 4097, 16),
                                           (4_186_113, 16), (4_186_114, 32), (4_186_114 + 8193, 32)])
def test_kate_public_entry_at_the_rule_thresholds(pool, length, tile_s):
    """h2g_kate_division_dev at the last length of S = 8, the first and last of S = 16 and the
    first of S = 32 (each one past a multiple of its tile), and one length per arm that is not"""
    assert h2g.debug_kate_tile_s(length) == tile_s
    a, b = pool[:length], rand_point()
    kr = KateRun(a)
    try:
        got = kr.run(b, public=True)
    finally:
        kr.close()
    assert np.array_equal(got, O.kate_division(a, b))


# ----------------------------------------------------------------------------- c. evaluation past 256 blocks
def root_of_unity(log_order):
    w = pow(B.ROOT_OF_UNITY, 1 << (B.S - log_order), R)
    assert pow(w, 1 << log_order, R) == 1 and pow(w, 1 << (log_order - 1), R) == R - 1
    return w


def eval_points():
    """... and x with x^EV_BLK = 1 (every block weight collapses) and = -1"""
    assert EV_BLK == 1 << 14
    return points() + [("w14", fr(root_of_unity(14))), ("w15", fr(root_of_unity(15)))]


@pytest.fixture(scope="module")
def all_rm1():
    a = np.tile(RM1, ((1 << 22) + 2 * EV_BLK + 7, 1))
    a.setflags(write=False)
    return a


def check_eval(a, pin):
    buf = h2g.DevBuf.from_array(a)
    try:
        ints = values(a) if pin else None
        for nm, x in eval_points():
            want = O.eval_poly(a, x)
            if pin:
                assert np.array_equal(want, fr(B.eval_polynomial(ints, values(x.reshape(1, 4))[0]))), (len(a), nm)
            assert np.array_equal(h2g.fr_eval(buf.ptr, x, dev_len=len(a)), want), (len(a), nm)
            assert np.array_equal(h2g.fr_eval(a, x), want), (len(a), nm)
    finally:
        buf.close()


@pytest.mark.parametrize("length", [1, 2, 257, 4097])
def test_eval_references_agree_at_small_lengths(pool, all_rm1, length):
    """or_fr_eval against big-integer Horner at the points and coefficient kinds used below"""
    check_eval(pool[:length], True)
    check_eval(all_rm1[:length], True)


@pytest.mark.parametrize("length,nb", [(1 << 22, 256), ((1 << 22) + 1, 257), ((1 << 22) + EV_BLK, 257),
                                       ((1 << 22) + EV_BLK + 1, 258), ((1 << 22) + 2 * EV_BLK + 7, 259)])
def test_eval_past_256_blocks(pool, all_rm1, length, nb):
    """nb = 256 is the last length with one partial sum per eval_level2 thread; 257 .. 259 take
    per = 2 (thread step x^(2 EV_BLK)), with the last group half empty or empty"""
    assert -(-length // EV_BLK) == nb
    check_eval(pool[:length], False)
    check_eval(all_rm1[:length], False)


# ----------------------------------------------------------------------------- d. batch inversion
def inv_threads(n):
    """poly_batch_invert_multi's split for one array, restated: (per, T)"""
    per = 16
    while per > 2 and n // per < (1 << 18):
        per >>= 1
    return per, -(-n // per)


def check_invert(a):
    want = O.batch_invert(a)
    if len(a) <= 4097:
        assert np.array_equal(want, from_values([pow(u, -1, R) if u else 0 for u in values(a)]))
    got = h2g.batch_invert(a)
    zero = ~a.any(axis=1)
    assert not got[zero].any(), "a zero did not stay zero"
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n,per", [((1 << 20) - 1, 2), (1 << 20, 4), ((1 << 21) - 1, 4), (1 << 21, 8),
                                   ((1 << 22) - 1, 8), (1 << 22, 16)])
def test_batch_invert_at_every_split(pool, n, per):
    assert inv_threads(n)[0] == per
    a = pool[:n].copy()
    a[::7] = 0
    check_invert(a)


@pytest.mark.parametrize("n", [1, 2, 17, 4097, (1 << 16) + 3, (1 << 20) - 1, 1 << 20, 1 << 21, 1 << 22])
def test_batch_invert_zero_patterns(pool, n):
    """zeros where the kernels treat them specially: slot t (the thread's first element, whose
    scratch slot holds its total), one thread's whole strided subset {t + k T}, everything,
    and everything but one element"""
    per, T = inv_threads(n)
    idx = np.arange(n)
    a = pool[:n].copy()
    a[:T] = 0  # every thread's first slot
    check_invert(a)
    a = pool[:n].copy()
    a[idx % T == 3 % T] = 0  # one thread's whole subset
    check_invert(a)
    check_invert(np.zeros((n, 4), dtype=np.uint64))
    for i in sorted({0, min(T, n - 1), n - 1}):  # exactly one nonzero
        a = np.zeros((n, 4), dtype=np.uint64)
        a[i] = pool[i]
        assert a[i].any()
        check_invert(a)
