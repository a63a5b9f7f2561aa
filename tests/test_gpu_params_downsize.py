"""h2g_g1_to_lagrange* (csrc/g1_fft.hip), h2g_params_from_parts and h2g_params_downsize.

Expected values come from tests/_g1_fft_ref.py: the inputs are arbitrary known multiples of
the generator, so every output is one oracle g1_mul of a scalar from a field FFT in Python
integers; the params are checked against h2g_params_setup's closed-form Lagrange basis and the
oracle's SRS.

Where the kernels change form: a stage launch is 64-thread blocks, one butterfly per thread.
  - k <= 6: a single, partly filled block (one lane at k = 1, one full wave at k = 7);
  - stage s reads one twiddle per WAVE when k - s >= 6 and one per LANE otherwise, so every
    k >= 7 runs both forms (k = 7: stage 1 uniform; k = 12: stages 1..6 uniform, 7..12 not).
All of that lies inside k = 1 .. 12; nothing changes form above it (no LDS-resident stages,
one grid mapping), so no larger k is added.
"""
import ctypes

import numpy as np
import pytest

import _g1_fft_ref as G
import _oracle as O
import bn254_ref as B
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

R = B.R
ERR_ARG, ERR_STATE, ERR_HANDLE = 1, 4, 5
S_INT = 0x5EED5EED1234567890ABCDEF
EDGE_KS = [3, 7, 9]  # 9: 256 butterflies per stage, four blocks


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield


def s_limbs(s=S_INT):
    return np.asarray(hc.fr_to_limbs(s), dtype=np.uint64)


def rc_of(fn):
    try:
        fn()
    except h2g.H2GError as e:
        return int(str(e).split()[2].rstrip(":"))
    return 0


def small_transform_works():
    ms = G.random_ms(3, 1)
    assert np.array_equal(h2g.g1_to_lagrange(G.points(ms)), G.points(G.lagrange_scalars(ms)))


def assert_points(got, ms, what):
    want = G.points(G.lagrange_scalars(ms))
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: outputs {bad[:8].tolist()} of {len(want)} differ"


# ----------------------------------------------------------------------------- the transform
@pytest.mark.parametrize("k", range(1, 13))
def test_random_multiples_every_output(k):
    ms = G.random_ms(k, 100 + k)
    assert_points(h2g.g1_to_lagrange(G.points(ms)), ms, f"k={k}")


@pytest.mark.parametrize("k", EDGE_KS)
def test_edge_vectors(k):
    for name, ms in G.edge_vectors(k).items():
        got = h2g.g1_to_lagrange(G.points(ms))
        assert_points(got, ms, f"k={k} {name}")
        if name == "all_equal":       # (P, identity, ...)
            assert np.array_equal(got[0], G.gmul(ms[0])) and not got[1:].any()
        if name == "omega_powers":    # exactly one non-identity output
            assert got[3].any() and not np.delete(got, 3, axis=0).any()
        if name == "all_identity":
            assert not got.any()


def _caller_stream():
    """a stream of the HIP runtime libh2g itself runs on (found among the loaded objects)"""
    h2g.lib()
    paths = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
    paths = [p for p in paths if "torch" not in p] or paths
    hip = ctypes.CDLL(paths[0])
    st = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(st)) == 0
    return hip, st


def test_in_place_and_on_a_callers_stream():
    k = 8
    ms = G.random_ms(k, 100 + k)  # test_random_multiples_every_output's inputs: memoised
    pts = G.points(ms)
    want = G.points(G.lagrange_scalars(ms))
    hip, st = _caller_stream()
    try:
        for stream in (None, st.value):
            d_in, d_out = h2g.DevBuf.from_array(pts), h2g.DevBuf(pts.nbytes)
            h2g.g1_to_lagrange_dev(d_in.ptr, k, d_out.ptr, stream=stream)
            assert np.array_equal(d_out.download(pts.shape), want)
            assert np.array_equal(d_in.download(pts.shape), pts)      # the input is only read
            h2g.g1_to_lagrange_dev(d_in.ptr, k, d_in.ptr, stream=stream)
            assert np.array_equal(d_in.download(pts.shape), want)
            d_in.close()
            d_out.close()
    finally:
        assert hip.hipStreamDestroy(st) == 0


# ----------------------------------------------------------------------------- the params
@pytest.mark.parametrize("k_big,k", [(6, 6), (9, 4), (13, 10)])
def test_downsize_against_setup_and_oracle(k_big, k):
    big = h2g.Params(k_big, s=s_limbs())
    small = big.downsize(k)
    ref = h2g.Params(k, s=s_limbs())
    _, og, ogl = O.srs(k, S_INT)
    g, gl = small.export()
    rg, rgl = ref.export()
    assert np.array_equal(g, rg) and np.array_equal(g, og)
    assert np.array_equal(gl, rgl) and np.array_equal(gl, ogl)
    for a, b in zip(small.g2(), ref.g2()):
        assert np.array_equal(a, b)
    assert small.k == k and small.handle != big.handle
    # the source is unchanged
    bg, _ = big.export()
    assert np.array_equal(bg[: 1 << k], og)
    # from_parts on the truncated powers: the same params
    parts = h2g.Params.from_parts(k, bg[: 1 << k], g2=ref.g2()[0], s_g2=ref.g2()[1])
    pg, pgl = parts.export()
    assert np.array_equal(pg, og) and np.array_equal(pgl, ogl)
    assert parts.write() == ref.write()
    for p in (big, small, ref, parts):
        p.close()


def test_from_parts_keeps_a_given_lagrange_basis():
    k = 4
    _, g, gl = O.srs(k, S_INT)
    other = gl[::-1].copy()  # deliberately not g's Lagrange basis
    p = h2g.Params.from_parts(k, g, g_lagrange=other)
    pg, pgl = p.export()
    assert np.array_equal(pg, g) and np.array_equal(pgl, other)
    p.close()


@pytest.mark.parametrize("fmt", [h2g.PROCESSED, h2g.RAW_BYTES, h2g.RAW_BYTES_UNCHECKED])
def test_written_bytes_equal_setups(fmt):
    big = h2g.Params(7, s=s_limbs())
    small = big.downsize(5)
    ref = h2g.Params(5, s=s_limbs())
    data = small.write(fmt)
    assert data == ref.write(fmt)
    back = h2g.Params.read(data, fmt)
    assert back.write(fmt) == data
    for a, b in zip(back.export(), ref.export()):
        assert np.array_equal(a, b)
    for p in (big, small, ref, back):
        p.close()


def test_proof_under_downsized_params():
    """keygen + create_proof under the downsized params: the bytes of Params(k, s), and they
    verify; the source still proves at its own k with the bytes it gave before"""
    circ, wit = hc.lookup_circuit(8)
    circ_big, wit_big = hc.lookup_circuit(9)
    big = h2g.Params(9, s=s_limbs())
    pk_big = h2g.ProvingKey(big, circ_big)
    before = pk_big.create_proof(wit_big)
    small = big.downsize(8)
    ref = h2g.Params(8, s=s_limbs())
    pk, pk_ref = h2g.ProvingKey(small, circ), h2g.ProvingKey(ref, circ)
    proof = pk.create_proof(wit)
    assert proof == pk_ref.create_proof(wit)
    vk = h2g.VerifyingKey.from_pk(pk)
    assert vk.verify(proof, [h2g.instance_columns(wit, circ)]) == h2g.VERIFY_OK
    assert pk_big.create_proof(wit_big) == before
    pk_again = h2g.ProvingKey(big, circ_big)
    assert pk_again.create_proof(wit_big) == before
    for x in (vk, pk, pk_ref, pk_big, pk_again, small, ref, big):
        x.close()


def test_errors():
    """every refusal's code, and after each one a small transform still gives the right points"""
    L = h2g.lib()
    h = ctypes.c_uint64()

    def refused(fn, code):
        assert rc_of(fn) == code
        small_transform_works()

    def raw(call):  # a C call's return code through rc_of's path
        return lambda: h2g.check(call())

    p = h2g.Params(5, s=s_limbs())
    g, _ = p.export()
    g2, s_g2 = p.g2()
    refused(lambda: p.downsize(6), ERR_ARG)                                   # k above the source's
    refused(lambda: h2g.Params(5, _handle=0xDEAD0000).downsize(3), ERR_HANDLE)  # never a handle
    gone = h2g.Params(3, s=s_limbs())
    handle = gone.handle
    gone.close()
    refused(lambda: h2g.Params(3, _handle=handle).downsize(2), ERR_HANDLE)    # a freed handle
    refused(lambda: h2g.Params.from_parts(5, g, g2=g2), ERR_ARG)              # one of g2 / s_g2 missing
    refused(lambda: h2g.Params.from_parts(5, g, s_g2=s_g2), ERR_ARG)
    off = g2.copy()
    off[8] ^= np.uint64(1)  # y.c0: no longer on the twist
    refused(lambda: h2g.Params.from_parts(5, g, g2=off, s_g2=s_g2), ERR_ARG)
    refused(raw(lambda: L.h2g_params_from_parts(28, h2g.p64(g), None, None, None, ctypes.byref(h))), ERR_ARG)
    refused(raw(lambda: L.h2g_params_downsize(p.handle, 3, None)), ERR_ARG)
    refused(raw(lambda: L.h2g_params_from_parts(5, None, None, None, None, ctypes.byref(h))), ERR_ARG)
    refused(raw(lambda: L.h2g_g1_to_lagrange(None, 3, h2g.p64(g))), ERR_ARG)
    refused(raw(lambda: L.h2g_g1_to_lagrange_dev(None, 3, None, None)), ERR_ARG)
    # params without G2 downsize to params without G2
    bare = h2g.Params.from_parts(5, g)
    low = bare.downsize(4)
    a = np.zeros(16, dtype=np.uint64)
    refused(raw(lambda: L.h2g_params_g2(low.handle, h2g.p64(a), h2g.p64(a.copy()))), ERR_STATE)
    assert np.array_equal(low.export()[1], O.srs(4, S_INT)[2])
    for x in (p, bare, low):
        x.close()
