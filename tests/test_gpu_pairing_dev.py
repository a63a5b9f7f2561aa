"""The device pairing check (csrc/pairing_dev.hip; h2g_pairing_check_batch, its _dev form,
h2g_debug_pairing_values) and h2g_verify_batch's isolation mode 1.

The params come from h2g_params_setup with a known s, so the expected verdict of a pair follows
from the scalars alone: with L = [a]G, R = [a s]G is valid and R = [a s + 1]G is not.  The
values behind the verdicts are compared with oracle/py/pairing_ref.py: the Miller value exactly,
the final value as the reference's final exponentiation raised to m = 2u (6u^2 + 3u + 1), the
fixed multiple of the exponent that the kernel's chain through powers of u computes.
"""
import ctypes
import random

import numpy as np
import pytest

import bn254_ref as B
import h2g
import h2g_circuit as hc
import pairing_ref as PR

pytestmark = pytest.mark.gpu

OK, REJECTED, MALFORMED = h2g.VERIFY_OK, h2g.VERIFY_REJECTED, h2g.VERIFY_MALFORMED
U = 0x44E992B44A6909F1
PAIRING_DEV_M = 2 * U * (6 * U * U + 3 * U + 1)
S1, S2 = 0xC0FFEE, 0x1F2E3D4C5B6A7988012345
A_VALUES = [1, 2, 0x51A7F00D5EED, 0xFEDCBA0987654321, 0x1234567890ABCDEF1234, B.R - 1, B.R - 2, 77]


class Side:
    """the params of one secret s, and a pool of inputs whose verdicts the scalars decide"""

    def __init__(self, s):
        self.s = s
        self.params = h2g.Params(4, s=np.asarray(hc.fr_to_limbs(s), dtype=np.uint64))
        self.vp = self.params.verifier()
        self.s_g2 = B.g2_mul(B.G2_GEN, s)
        self.L = [B.g1_mul(B.G1_GEN, a) for a in A_VALUES]
        self.good = [B.g1_mul(B.G1_GEN, a * s % B.R) for a in A_VALUES]
        self.bad = [B.g1_mul(B.G1_GEN, (a * s + 1) % B.R) for a in A_VALUES]

    def specials(self):
        """(left, right, expected): the identities, a negated left, one valid pair twice"""
        L, good = self.L, self.good
        return [(None, None, 1), (None, good[2], 0), (L[3], None, 0), (B.g1_neg(L[4]), good[4], 0),
                (L[5], good[5], 1), (L[5], good[5], 1)]

    def pattern(self, n, seed):
        rng = random.Random(seed)
        out = []
        for _ in range(n):
            i, valid = rng.randrange(len(A_VALUES)), rng.random() < 0.5
            out.append((self.L[i], (self.good if valid else self.bad)[i], int(valid)))
        return out

    def close(self):
        self.params.close()


_SIDES = {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for s in _SIDES.values():
        s.close()
    _SIDES.clear()


def side(s):
    if s not in _SIDES:
        _SIDES[s] = Side(s)
    return _SIDES[s]


def limbs(cases):
    return np.array([B.g1_affine_mont_limbs(l) + B.g1_affine_mont_limbs(r) for l, r, _ in cases],
                    dtype=np.uint64).reshape(-1, 2, 8)


def f12_from_limbs(a):
    return [tuple(B.from_mont(B.from_limbs([int(v) for v in a[i][j]]), B.P) for j in range(2)) for i in range(6)]


# ----------------------------------------------------------------------------- values
def test_miller_and_final_values_match_the_reference():
    sd = side(S1)
    cases = [(sd.L[2], sd.good[2], 1), (sd.L[3], sd.bad[3], 0), (None, sd.good[4], 0), (sd.L[5], sd.good[5], 1)]
    miller, gt = h2g.debug_pairing_values(sd.vp, limbs(cases))
    for i, (l, r, want) in enumerate(cases):
        f = PR.f12_mul(PR.miller_loop(l, sd.s_g2), PR.miller_loop(B.g1_neg(r) if r else None, PR.G2))
        assert f12_from_limbs(miller[i]) == [tuple(c) for c in f], i
        e = PR.f12_pow(PR.final_exponentiation(f), PAIRING_DEV_M)
        assert f12_from_limbs(gt[i]) == [tuple(c) for c in e], i
        assert PR.f12_is_one(e) == bool(want)
    assert list(h2g.pairing_check_batch(sd.vp, limbs(cases))) == [c[2] for c in cases]
    # either output alone
    only_m, none = h2g.debug_pairing_values(sd.vp, limbs(cases), gt=False)
    assert none is None and np.array_equal(only_m, miller)
    none, only_g = h2g.debug_pairing_values(sd.vp, limbs(cases), miller=False)
    assert none is None and np.array_equal(only_g, gt)


# ----------------------------------------------------------------------------- verdicts
def arrangements(sd, count):
    """inputs of `count` checks holding the special inputs: all of them ahead of a seeded
    pattern, or, where the count is smaller, every window of them"""
    sp = sd.specials()
    if count >= len(sp):
        return [sp + sd.pattern(count - len(sp), 1000 + count)]
    return [sp[o:o + count] for o in range(len(sp) - count + 1)]


@pytest.mark.parametrize("count", [1, 5, 63, 64, 65, 200])
def test_verdicts(count):
    sd = side(S1)
    cases = arrangements(sd, count)
    if count < 8:
        cases += [sd.pattern(count, 2000 + count + i) for i in range(3)]
    for c in cases:
        assert len(c) == count
        got = h2g.pairing_check_batch(sd.vp, limbs(c))
        assert got.dtype == np.int32 and list(got) == [w for _, _, w in c]
    if count == 200:
        assert 0 < sum(w for _, _, w in cases[0]) < count


# ----------------------------------------------------------------------------- _dev
def _caller_stream():
    """a stream of the HIP runtime libh2g itself runs on (found among the loaded objects)"""
    h2g.lib()
    paths = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
    paths = [p for p in paths if "torch" not in p] or paths
    hip = ctypes.CDLL(paths[0])
    st = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(st)) == 0
    return hip, st


def test_dev_entry_on_a_callers_stream_and_the_table_cache_key():
    a, b = side(S1), side(S2)
    cases = a.specials() + a.pattern(30, 7)            # valid for S1; under S2 only the identities hold
    lr = limbs(cases)
    want_a = [w for _, _, w in cases]
    want_b = [int(l is None and r is None) for l, r, _ in cases]
    assert sum(want_a) > sum(want_b) == 1
    hip, st = _caller_stream()
    try:
        d_lr = h2g.DevBuf.from_array(lr)
        for sd, want in ((a, want_a), (b, want_b), (a, want_a)):
            assert list(h2g.pairing_check_batch(sd.vp, lr)) == want
            d_ok = h2g.DevBuf.from_array(np.full(len(cases), 7, dtype=np.int32))
            h2g.pairing_check_batch(sd.vp, d_lr.ptr, dev_count=len(cases), d_ok=d_ok.ptr, stream=st.value)
            assert hip.hipStreamSynchronize(st) == 0
            assert list(d_ok.download(len(cases), np.int32)) == want
            assert np.array_equal(d_lr.download(lr.shape), lr)     # the input is only read
            d_ok.close()
        # the library's own stream, and a pair that holds under S2
        cases_b = b.pattern(12, 8)
        assert list(h2g.pairing_check_batch(b.vp, limbs(cases_b))) == [w for _, _, w in cases_b]
        d_ok = h2g.DevBuf.from_array(np.full(len(cases), 7, dtype=np.int32))
        h2g.pairing_check_batch(a.vp, d_lr.ptr, dev_count=len(cases), d_ok=d_ok.ptr)
        assert list(d_ok.download(len(cases), np.int32)) == want_a
        d_ok.close()
        d_lr.close()
    finally:
        assert hip.hipStreamDestroy(st) == 0


# ----------------------------------------------------------------------------- arguments
def test_arguments():
    sd = side(S1)
    L = h2g.lib()
    ok_t = ctypes.POINTER(ctypes.c_int32)
    good = limbs(sd.pattern(8, 3))

    def call(lr):
        ok = np.full(len(lr), 7, dtype=np.int32)
        rc = L.h2g_pairing_check_batch(ctypes.byref(sd.vp), h2g.p64(lr), len(lr), ok.ctypes.data_as(ok_t))
        return rc, ok, L.h2g_last_error().decode()

    rc, ok, _ = call(good)
    assert rc == 0 and set(ok) <= {0, 1}
    off = good.copy()
    x, y = sd.L[1]
    off[3, 0] = B.fq_mont_limbs(x) + B.fq_mont_limbs((y + 1) % B.P)      # an off-curve left point
    big = good.copy()
    big[3, 1, 4:] = B.to_limbs(B.P)                                        # a coordinate >= p (raw limbs)
    for bad in (off, big):
        rc, ok, msg = call(bad)
        assert rc == 1 and "3" in msg, msg                                 # H2G_ERR_ARG, naming the index
        assert list(ok) == [7] * 8                                         # untouched
    with pytest.raises(h2g.H2GError):
        h2g.pairing_check_batch(sd.vp, off)
    # count == 0
    assert L.h2g_pairing_check_batch(ctypes.byref(sd.vp), None, 0, None) == 0
    assert len(h2g.pairing_check_batch(sd.vp, np.zeros((0, 2, 8), dtype=np.uint64))) == 0
    assert L.h2g_pairing_check_batch_dev(ctypes.byref(sd.vp), None, 0, None, None) == 0
    # modes
    assert L.h2g_verify_set_isolation(2) == 1
    assert L.h2g_verify_set_isolation(-1) == 1
    assert L.h2g_verify_set_isolation(0) == 0


# ----------------------------------------------------------------------------- the batch verifier
N_PROOFS = 9


@pytest.fixture(scope="module")
def batch():
    """nine proofs of the lookup / shuffle circuit of tests/test_gpu_verify.py (k = 6)"""
    params = h2g.Params(6, s=np.asarray(hc.fr_to_limbs(S1), dtype=np.uint64))
    made = [hc.my_circuit(6, input_value=42 + i) for i in range(N_PROOFS)]
    circ = made[0][0]
    pk = h2g.ProvingKey(params, circ)
    vk = h2g.VerifyingKey.from_pk(pk)
    proofs = [pk.create_proof_multi([w], seed=bytes([i + 1] * 32), fills=[f]) for i, (_, w, f) in enumerate(made)]
    insts = [[h2g.instance_columns(w, circ)] for _, w, _ in made]
    n_evals = (pk.n_adv_q + pk.n_fix_q + 1 + len(circ.perm_columns) + (3 * pk.nsets - 1 if pk.nsets else 0)
               + 5 * len(circ.lookups) + 2 * len(circ.shuffles))
    ev0 = 32 * (len(proofs[0]) // 32 - n_evals - 2)      # the first evaluation (SHPLONK: two tail points)
    yield vk, proofs, insts, ev0
    vk.close()
    pk.close()
    params.close()


def tampered(proof, pos):
    t = bytearray(proof)
    t[pos] ^= 1
    return bytes(t)


def test_batch_isolation_by_one_device_launch(batch):
    vk, proofs, insts, ev0 = batch
    single = [vk.verify(p, i) for p, i in zip(proofs, insts)]
    assert single == [OK] * N_PROOFS
    batches = []
    for bad_set in ([], [0], [8], [3, 4], list(range(N_PROOFS))):
        batches.append(([tampered(p, ev0 + 32) if i in bad_set else p for i, p in enumerate(proofs)], len(bad_set)))
    trunc = list(batches[1][0])
    trunc[5] = trunc[5][:-1]                                  # MALFORMED beside a bad proof
    batches.append((trunc, 1))
    trunc_only = list(proofs)
    trunc_only[5] = proofs[5][:-1]                            # MALFORMED among valid proofs: the combined check holds
    batches.append((trunc_only, 0))
    log2_b = 4                                                # ceil(log2 9)
    try:
        for ps, f in batches:
            each = [vk.verify(p, i) for p, i in zip(ps, insts)]
            well = sum(v != MALFORMED for v in each)
            assert sum(v == REJECTED for v in each) == f
            h2g.verify_set_isolation(1)
            v1, st1 = vk.verify_batch(ps, insts, rng_seed=bytes([5] * 32))
            h2g.verify_set_isolation(0)
            v0, st0 = vk.verify_batch(ps, insts, rng_seed=bytes([5] * 32))
            assert v1 == v0 == each
            assert st1[0] == (1 if f == 0 else 1 + well)
            # mode 0 afterwards: what tests/test_gpu_verify.py asserts of the number of checks
            assert (st0[0] == 1) if f == 0 else (2 <= st0[0] <= 1 + 2 * f * log2_b)
            assert st1[1:3] == st0[1:3]
    finally:
        h2g.verify_set_isolation(0)
