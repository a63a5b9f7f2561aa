"""The polynomial-commitment layer through the library -- h2g_params_commit{,_lagrange},
h2g_fr_eval, h2g_kate_division, h2g_multiopen_prove / _verify over the library's transcript
objects -- against the Python restatement (tests/_multiopen_ref.py, pinned by
tests/test_multiopen_ref_cpu.py) and the C oracle.  The params come from a known secret
(h2g_params_setup), so a commitment is [p(s)] G and DualMSM::check is [s] left == right.
"""
import random

import numpy as np
import pytest

import _multiopen_ref as M
import _oracle as O
import bn254_ref as B
import h2g
import h2g_circuit as hc
import verifier as V

pytestmark = pytest.mark.gpu

OK, REJECTED, MALFORMED = h2g.VERIFY_OK, h2g.VERIFY_REJECTED, h2g.VERIFY_MALFORMED
ERR_ARG, ERR_STATE, ERR_HANDLE = 1, 4, 5
S_INT = 0xC0FFEE
COMBOS = [(m, t) for m in ("shplonk", "gwc") for t in ("blake2b", "keccak256")]
COMBO_IDS = [f"{m}-{t}" for m, t in COMBOS]
_PARAMS = {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for p in _PARAMS.values():
        p.close()
    _PARAMS.clear()


def params(k):
    if k not in _PARAMS:
        _PARAMS[k] = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(S_INT), dtype=np.uint64))
    return _PARAMS[k]


def fr(x):
    return np.asarray(B.fr_mont_limbs(x % B.R), dtype=np.uint64)


def pt(p):
    return np.asarray(B.g1_affine_mont_limbs(p), dtype=np.uint64)


def mont(poly):
    return hc.ints_to_mont([int(v) % B.R for v in poly]).reshape(-1, 4)


def code(fn, *args, **kw):
    with pytest.raises(h2g.H2GError) as e:
        fn(*args, **kw)
    return int(str(e.value).split()[2].rstrip(":"))


def lib_prove(prm, scheme, kind, polys, queries, head=(), dev=()):
    """the library's opening of `polys` (lists of ints) -> bytes; head: points / ints written
    first; dev: indices of the polynomials handed over resident on the device"""
    T = h2g.Transcript(kind)
    for v in head:
        T.write_scalar(fr(v)) if isinstance(v, int) else T.write_point(pt(v))
    bufs = {i: h2g.DevBuf.from_array(mont(polys[i])) for i in dev}
    refs = [(bufs[i].ptr, len(p)) if i in bufs else mont(p) for i, p in enumerate(polys)]
    try:
        prm.multiopen_prove(T, refs, [(i, fr(z)) for i, z in queries], scheme)
        return T.bytes()
    finally:
        T.close()
        for b in bufs.values():
            b.close()


def lib_verify(vp, scheme, kind, proof, commitments, queries, nhead=(0, 0, 0)):
    """-> (verdict, lr) for the argument at the end of `proof` (after a head of nhead = (points,
    challenges, scalars), read and squeezed in that order)"""
    T = h2g.Transcript(kind, proof=proof)
    try:
        for _ in range(nhead[0]):
            T.read_point()
        for _ in range(nhead[1]):
            T.squeeze()
        for _ in range(nhead[2]):
            T.read_scalar()
        cm = np.stack([pt(c) for c in commitments])
        return h2g.multiopen_verify(vp, T, cm, [(c, fr(z), fr(e)) for c, z, e in queries], scheme)
    finally:
        T.close()


def ref_prove(scheme, kind, polys, queries):
    T = M.writer(kind)
    M.prove(scheme, T, S_INT, polys, queries)
    return T.finalize()


def ref_verify(scheme, kind, proof, commitments, queries):
    return M.verify(scheme, M.reader(kind, proof), S_INT, commitments, queries, proof)


# ----------------------------------------------------------------------------- a. the reference's round trip
@pytest.mark.parametrize("scheme,kind", COMBOS, ids=COMBO_IDS)
def test_round_trip(scheme, kind):
    """multiopen_test.rs:140-304 at k = 4 through the library"""
    k = 4
    prm = params(k)
    polys = M.round_trip_polys(k)
    want = M.round_trip_prove(scheme, kind, k, S_INT)
    # the head as the reference's create_proof writes it, on the library's transcript
    T = h2g.Transcript(kind)
    cms = [M.commit(p, S_INT) for p in polys]
    for c in cms:
        T.write_point(pt(c))
    x, y = (B.from_mont(B.from_limbs(T.squeeze()), B.R) for _ in range(2))
    evs = [B.eval_polynomial(p, z) for p, z in zip(polys, (x, x, y))]
    for e in evs:
        T.write_scalar(fr(e))
    prm.multiopen_prove(T, [mont(p) for p in polys], [(0, fr(x)), (1, fr(x)), (2, fr(y))], scheme)
    proof = T.bytes()
    T.close()
    assert proof == want
    valid = [(0, x, evs[0]), (1, x, evs[1]), (2, y, evs[2])]
    invalid = [(0, x, evs[0]), (1, x, evs[0]), (2, y, evs[2])]
    vp = prm.verifier()
    assert lib_verify(vp, scheme, kind, proof, cms, valid, (3, 2, 3))[0] == OK
    assert lib_verify(vp, scheme, kind, proof, cms, invalid, (3, 2, 3))[0] == REJECTED
    RT, rcms, rvalid, rinvalid = M.round_trip_open(kind, proof)
    assert (rcms, rvalid, rinvalid) == (cms, valid, invalid)
    assert M.verify(scheme, RT, S_INT, rcms, rvalid, proof) is True


# ----------------------------------------------------------------------------- b. the shapes
K = 6
N = 1 << K


def _shapes():
    """30 polynomials of lengths 1, 2, n/2, n - 1, n; rotation sets {x}, {x, wx},
    {x, wx, w^-1 x}, {y}, one polynomial at 5 points, {y, 0} and {1}; 25 polynomials at x
    (three lincomb launches of LIN_MAXT - 1 = 11 terms, so the accumulating launch runs); the
    points 0 and 1 (division by X) and w (a domain element) among them"""
    rnd = random.Random(20)
    w = B.omega_for(K)
    x, y = rnd.randrange(B.R), rnd.randrange(B.R)
    wx, wix = w * x % B.R, pow(w, -1, B.R) * x % B.R
    lens = [1, 2, N // 2, N - 1, N]
    polys = [[rnd.randrange(B.R) for _ in range(lens[i % 5])] for i in range(30)]
    sets = [[x]] * 12 + [[x, wx]] * 8 + [[x, wx, wix]] * 4 + [[y]] * 3 + [[0, 1, w, x, y]] + [[y, 0]] + [[1]]
    queries = [(i, z) for i, zs in enumerate(sets) for z in zs]
    assert sum(1 for _, z in queries if z == x) == 25
    return polys, queries


@pytest.fixture(scope="module")
def shapes():
    polys, queries = _shapes()
    cms = [M.commit(p, S_INT) for p in polys]
    vq = [(i, z, B.eval_polynomial(polys[i], z)) for i, z in queries]
    proofs = {c: lib_prove(params(K), c[0], c[1], polys, queries) for c in COMBOS}
    return polys, queries, cms, vq, proofs


@pytest.mark.parametrize("scheme,kind", COMBOS, ids=COMBO_IDS)
def test_shapes_bytes_and_verdicts(shapes, scheme, kind):
    polys, queries, cms, vq, proofs = shapes
    proof = proofs[(scheme, kind)]
    assert proof == ref_prove(scheme, kind, polys, queries)
    assert lib_verify(params(K).verifier(), scheme, kind, proof, cms, vq)[0] == OK
    assert ref_verify(scheme, kind, proof, cms, vq) is True


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_shapes_every_change_is_rejected(shapes, scheme):
    polys, queries, cms, vq, proofs = shapes
    proof = proofs[(scheme, "blake2b")]
    vp = params(K).verifier()
    for i in range(len(vq)):  # every evaluation, changed by 1
        bad = list(vq)
        bad[i] = (vq[i][0], vq[i][1], (vq[i][2] + 1) % B.R)
        assert lib_verify(vp, scheme, "blake2b", proof, cms, bad)[0] == REJECTED, i
    for i in range(len(cms) - 1):  # every pair of neighbouring commitments, swapped
        bad = list(cms)
        bad[i], bad[i + 1] = bad[i + 1], bad[i]
        assert lib_verify(vp, scheme, "blake2b", proof, bad, vq)[0] == REJECTED, i


def _no_curve_x():
    x = 1
    while B.fq_sqrt((x * x * x + 3) % B.P) is not None:
        x += 1
    return x


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_shapes_malformed(shapes, scheme):
    polys, queries, cms, vq, proofs = shapes
    proof = proofs[(scheme, "blake2b")]
    vp = params(K).verifier()
    assert lib_verify(vp, scheme, "blake2b", proof[:-1], cms, vq) == (MALFORMED, None)
    bad = _no_curve_x().to_bytes(32, "little") + proof[32:]  # the first point of the argument (SHPLONK: h)
    assert lib_verify(vp, scheme, "blake2b", bad, cms, vq) == (MALFORMED, None)
    with pytest.raises(V.VerifyError):
        ref_verify(scheme, "blake2b", bad, cms, vq)


# ----------------------------------------------------------------------------- c. device residence
@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_device_resident_polynomials(shapes, scheme):
    polys, queries, cms, vq, proofs = shapes
    want = proofs[(scheme, "blake2b")]
    assert lib_prove(params(K), scheme, "blake2b", polys, queries, dev=range(len(polys))) == want
    assert lib_prove(params(K), scheme, "blake2b", polys, queries, dev=range(0, len(polys), 3)) == want


# ----------------------------------------------------------------------------- d. lr
@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_lr_is_the_dual_msm(shapes, scheme):
    polys, queries, cms, vq, proofs = shapes
    proof = proofs[(scheme, "blake2b")]
    vp = params(K).verifier()
    verdict, lr = lib_verify(vp, scheme, "blake2b", proof, cms, vq)
    left, right = V.affine_from_limbs(lr[0]), V.affine_from_limbs(lr[1])
    assert verdict == OK and left is not None and B.g1_mul(left, S_INT) == right
    bad = [(vq[0][0], vq[0][1], (vq[0][2] + 1) % B.R)] + vq[1:]
    verdict, lr = lib_verify(vp, scheme, "blake2b", proof, cms, bad)
    left, right = V.affine_from_limbs(lr[0]), V.affine_from_limbs(lr[1])
    assert verdict == REJECTED and B.g1_mul(left, S_INT) != right
    if scheme == "shplonk":
        ok, h2, r = M.verify_shplonk(M.reader("blake2b", proof), S_INT, cms, vq, proof)
        verdict, lr = lib_verify(vp, scheme, "blake2b", proof, cms, vq)
        assert ok and (V.affine_from_limbs(lr[0]), V.affine_from_limbs(lr[1])) == (h2, r)


# ----------------------------------------------------------------------------- e. identity commitment
@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_identity_commitment_is_an_argument_error(scheme):
    prm = params(4)
    T = h2g.Transcript("blake2b")
    T.write_scalar(fr(3))
    O2 = V.Blake2bRead(B.fr_to_repr(3))
    O2.read_scalar()
    assert code(prm.multiopen_prove, T, [mont([5])], [(0, fr(77))], scheme) == ERR_ARG
    assert b"infinity" in h2g.lib().h2g_last_error()
    assert T.bytes() == B.fr_to_repr(3)
    assert B.from_mont(B.from_limbs(T.squeeze()), B.R) == O2.squeeze()  # the transcript is as it was
    T.close()
    polys, queries = [[5, 1]], [(0, 77)]
    assert lib_prove(prm, scheme, "blake2b", polys, queries) == ref_prove(scheme, "blake2b", polys, queries)


# ----------------------------------------------------------------------------- f. argument errors
def test_argument_errors():
    prm = params(4)
    n = 16
    p = mont(list(range(1, n + 1)))
    q = [(0, fr(9))]
    T = h2g.Transcript("blake2b")
    assert code(prm.multiopen_prove, T, [p], [(1, fr(9))]) == ERR_ARG            # index out of range
    assert code(prm.multiopen_prove, T, [mont(list(range(n + 1)))], q) == ERR_ARG  # len > n
    assert code(prm.multiopen_prove, T, [p], []) == ERR_ARG                      # nqueries == 0
    assert code(prm.multiopen_prove, T, [p[:0]], q) == ERR_ARG                   # an empty polynomial
    buf = h2g.DevBuf.from_array(np.concatenate([p, p]))
    assert code(prm.multiopen_prove, T, [(buf.ptr + 8, n)], q) == ERR_ARG        # misaligned device polynomial
    r_limbs = np.asarray(B.to_limbs(B.R), dtype=np.uint64)
    assert code(prm.multiopen_prove, T, [p], [(0, r_limbs)]) == ERR_ARG          # a point >= r
    assert T.bytes() == b""
    prm.multiopen_prove(T, [(buf.ptr, n)], q)                                    # and the same call, well formed
    proof = T.bytes()
    buf.close()
    R = h2g.Transcript("blake2b", proof=proof)
    assert code(prm.multiopen_prove, R, [p], q) == ERR_ARG                       # read mode given to prove
    vp = prm.verifier()
    cm = np.stack([pt(M.commit(list(range(1, n + 1)), S_INT))])
    vq = [(0, fr(9), fr(B.eval_polynomial(list(range(1, n + 1)), 9)))]
    assert code(h2g.multiopen_verify, vp, T, cm, vq) == ERR_ARG                  # write mode given to verify
    assert code(h2g.multiopen_verify, vp, R, cm, [(1,) + vq[0][1:]]) == ERR_ARG
    assert code(h2g.multiopen_verify, vp, R, cm, []) == ERR_ARG
    assert R.remaining() == len(proof)
    assert h2g.multiopen_verify(vp, R, cm, vq)[0] == OK
    T.close()
    R.close()
    assert code(prm.multiopen_prove, T, [p], q) == ERR_HANDLE                    # a freed transcript
    assert code(h2g.multiopen_verify, vp, R, cm, vq) == ERR_HANDLE
    dead = h2g.Params(4, _handle=0xDEAD)
    W = h2g.Transcript("blake2b")
    assert code(dead.multiopen_prove, W, [p], q) == ERR_HANDLE
    assert code(dead.commit, p) == ERR_HANDLE
    dead.handle = 0
    assert code(prm.commit, mont(list(range(n + 1)))) == ERR_ARG                 # the reference's assert!
    W.close()


# ----------------------------------------------------------------------------- g. commit / commit_lagrange
@pytest.mark.parametrize("k", [4, 6])
def test_commit_and_commit_lagrange(k):
    prm = params(k)
    n = 1 << k
    rnd = random.Random(k)
    omega = fr(B.omega_for(k))
    for length in (0, 1, n - 1, n):
        poly = [rnd.randrange(B.R) for _ in range(length)]
        a = mont(poly) if length else np.zeros((0, 4), dtype=np.uint64)
        got = prm.commit(a)
        assert V.affine_from_limbs(got) == M.commit(poly, S_INT), length
        if length:
            buf = h2g.DevBuf.from_array(a)
            assert np.array_equal(prm.commit(buf.ptr, dev_len=length), got)
            buf.close()
    # the reference's own relation (kzg/commitment.rs:381-408): commit_lagrange(fft(a)) == commit(a)
    poly = [rnd.randrange(B.R) for _ in range(n)]
    a = mont(poly)
    evals = h2g.fft(a, omega)
    want = prm.commit(a)
    assert np.array_equal(prm.commit_lagrange(evals), want)
    buf = h2g.DevBuf.from_array(evals)
    assert np.array_equal(prm.commit_lagrange(buf.ptr, dev_len=n), want)
    buf.close()


# ----------------------------------------------------------------------------- h. eval_polynomial / kate_division
# kate_division's tiles hold 256 x 8 = 2048 quotient coefficients (len - 1): 2048 .. 2050 straddle
# one; poly_eval_batch's blocks 256 x 64 = 16384 coefficients
LENGTHS = [1, 2, 3, 64, 65, 1000, 2048, 2049, 2050]


@pytest.fixture(scope="module")
def rand_poly():
    return O.random_fr(np.random.default_rng(8), 16385)


def _points():
    return [fr(0), fr(1), fr(B.R - 1), O.random_fr(np.random.default_rng(9), 1)[0]]


@pytest.mark.parametrize("length", LENGTHS + [16384, 16385])
def test_fr_eval(rand_poly, length):
    a = np.ascontiguousarray(rand_poly[:length])
    buf = h2g.DevBuf.from_array(a)
    for x in _points():
        want = O.eval_poly(a, x)
        assert np.array_equal(h2g.fr_eval(a, x), want)
        assert np.array_equal(h2g.fr_eval(buf.ptr, x, dev_len=length), want)
    buf.close()


@pytest.mark.parametrize("length", LENGTHS)
def test_kate_division(rand_poly, length):
    a = np.ascontiguousarray(rand_poly[:length])
    for b in _points():
        got = h2g.kate_division(a, b)
        assert got.shape == (length - 1, 4)
        if length > 1:
            assert np.array_equal(got, O.kate_division(a, b))
    if length > 1:
        da, dq = h2g.DevBuf.from_array(a), h2g.DevBuf(32 * length)
        h2g.kate_division_dev(da.ptr, length, _points()[3], dq.ptr)
        assert np.array_equal(dq.download((length - 1, 4)), O.kate_division(a, _points()[3]))
        da.close()
        dq.close()


def test_eval_and_division_argument_errors():
    a = O.random_fr(np.random.default_rng(1), 4)
    assert np.array_equal(h2g.fr_eval(a[:0], fr(5)), fr(0))
    assert code(h2g.kate_division, a[:0], fr(5)) == ERR_ARG
    buf = h2g.DevBuf.from_array(a)
    assert code(h2g.fr_eval, buf.ptr + 8, fr(5), dev_len=2) == ERR_ARG
    assert code(h2g.kate_division_dev, buf.ptr + 8, 2, fr(5), buf.ptr) == ERR_ARG
    buf.close()


# ----------------------------------------------------------------------------- i. create_proof and verify_proof unchanged
def test_prover_and_verifier_unchanged_by_standalone_calls(shapes):
    circ, wit = hc.mixed_circuit(7)
    prm = params(7)
    pk = h2g.ProvingKey(prm, circ)
    before = pk.create_proof(wit)
    polys, queries, cms, vq, proofs = shapes
    for scheme in ("shplonk", "gwc"):  # the same params (k = 7: the polynomials are shorter than n)
        assert lib_prove(prm, scheme, "blake2b", polys, queries) == proofs[(scheme, "blake2b")]
        assert lib_verify(prm.verifier(), scheme, "blake2b", proofs[(scheme, "blake2b")], cms, vq)[0] == OK
    after = pk.create_proof(wit)
    assert after == before
    vk = h2g.VerifyingKey.from_pk(pk)
    assert vk.verify(after, [h2g.instance_columns(wit, circ)]) == OK
    vk.close()
    pk.close()


# ----------------------------------------------------------------------------- j. transports
def test_transports_take_no_part(shapes):
    polys, queries, cms, vq, proofs = shapes
    prm = params(K)
    called = []

    def boom(*a):
        called.append(a)
        raise RuntimeError("the standalone opening must not reach the transport")

    h2g.set_spmd_transport(2, 0, allgather=boom, allgather_host=boom)
    try:
        T = h2g.Transcript("blake2b")
        refs = [mont(p) for p in polys]
        assert code(prm.multiopen_prove, T, refs, [(i, fr(z)) for i, z in queries]) == ERR_STATE
        assert T.bytes() == b""
        T.close()
        # commit is a plain local MSM (as h2g_params_msm_dev): it runs, whole, without the transport
        assert V.affine_from_limbs(prm.commit(mont(polys[4]))) == cms[4]
    finally:
        h2g.set_spmd_transport(1)
    assert not called and not h2g.transport_errors()
    h2g.set_shard_transport(2, launch=boom, collect=boom)
    try:
        T = h2g.Transcript("blake2b")
        assert code(prm.multiopen_prove, T, [mont(polys[4])], [(0, fr(3))]) == ERR_STATE
        T.close()
    finally:
        h2g.set_shard_transport(1)
    assert not called
    assert lib_prove(prm, "shplonk", "blake2b", polys, queries) == proofs[("shplonk", "blake2b")]
