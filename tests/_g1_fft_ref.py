"""Expected values for the G1 group FFT (g_to_lagrange, arithmetic.rs:30-54), shared by
tests/test_g1_fft_host_cpu.py and tests/test_gpu_params_downsize.py.

The inputs are known multiples of the generator, g_j = [m_j] G with arbitrary m_j, so
    L_i = [n^-1 sum_j omega^(-ij) m_j mod r] G:
one inverse field FFT in Python integers (oracle/py/bn254_ref.py) and one oracle g1_mul per
output, the identity where the scalar is 0.  Nothing of an SRS's structure is in the m_j.
"""
import numpy as np

import _oracle as O
import bn254_ref as B
import h2g_circuit as hc

R = B.R
_GEN = np.array(B.g1_affine_mont_limbs(B.G1_GEN), dtype=np.uint64)
_MUL = {0: np.zeros(8, dtype=np.uint64)}


def gmul(m):
    """[m] G as 8 Montgomery limbs (zeros: the identity), memoised"""
    m %= R
    if m not in _MUL:
        _MUL[m] = O.g1_mul(_GEN, np.array(hc.fr_to_limbs(m), dtype=np.uint64))
    return _MUL[m]


def points(ms):
    return np.array([gmul(m) for m in ms], dtype=np.uint64).reshape(-1, 8)


def lagrange_scalars(ms):
    """n^-1 sum_j omega^(-ij) m_j for every i"""
    n = len(ms)
    k = n.bit_length() - 1
    assert n == 1 << k
    ninv = pow(n, -1, R)
    return [v * ninv % R for v in B.fft([m % R for m in ms], pow(B.omega_for(k), -1, R))]


def rnd(rng):
    return int.from_bytes(rng.bytes(32), "little") % R


def random_ms(k, seed):
    rng = np.random.default_rng(seed)
    return [rnd(rng) for _ in range(1 << k)]


def edge_vectors(k, seed=9):
    """name -> m_j (n = 2^k >= 8): the inputs that meet every special case of a butterfly"""
    n = 1 << k
    assert n >= 8
    rng = np.random.default_rng(seed + k)
    w = B.omega_for(k)
    c, a, j = 3, rnd(rng), 2
    v = {}
    v["all_equal"] = [a] * n                                  # -> (P, identity, ...): P + P, P + (-P) in every stage
    v["single_at_0"] = [a] + [0] * (n - 1)
    v["single_at_5"] = [a if i == 5 else 0 for i in range(n)]
    v["omega_powers"] = [pow(w, c * i, R) for i in range(n)]  # -> one non-identity output (at c)
    v["all_identity"] = [0] * n
    v["identity_every_third"] = [0 if i % 3 == 0 else rnd(rng) for i in range(n)]
    for name, d in (("half", n // 2), ("next", 1)):           # first / last stage partners
        sparse = [0] * n
        sparse[j], sparse[j + d] = a, R - a
        dense = [rnd(rng) for _ in range(n)]
        dense[j + d] = R - dense[j]
        v[f"negation_at_{name}_sparse"] = sparse
        v[f"negation_at_{name}_dense"] = dense
    v["zero_one_minus_one"] = [(0, 1, R - 1)[int(x)] for x in rng.integers(0, 3, n)]
    return v
