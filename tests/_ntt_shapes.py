"""The domain shapes of tests/test_gpu_ntt_shapes.py and the NTT kernel variants each is there
for, read from the library's own plan (h2g.debug_ntt_plan, the function every transform
launches from).  tests/test_ntt_plan_cpu.py asserts the table without a GPU; the GPU tests
call `require` in their setup, so a shape that stops selecting its variant fails instead of
passing hollow.
"""
import numpy as np

import _oracle as O
import h2g

R_MINUS_1 = np.array([0x43e1f593f0000000, 0x2833e84879b97091, 0xb85045b68181585d, 0x30644e72e131a029],
                     dtype=np.uint64)  # r - 1, the largest stored integer


def extended_k(j, k):
    ek = k
    while (1 << ek) < (j - 1) << k:
        ek += 1
    return ek


def domain_plans(j, k, cus=256, count=1):
    """The plans of EvaluationDomain::new(j, k)'s transforms, by the arguments the library
    passes for them (csrc/abi.cpp): lagrange_to_coeff, coeff_to_extended and the sub-coset
    transform leave the last pass no constant above 2^10 points (the scale rides in the first
    pass's table), extended_to_coeff always does (the zeta powers) and keeps n (j - 1) outputs."""
    ek = extended_k(j, k)
    n, N = 1 << k, 1 << ek
    return {"l2c": h2g.debug_ntt_plan(k, n, n, count=count, cus=cus, epilogue_one=k > 10),
            "c2e": h2g.debug_ntt_plan(ek, n, N, count=count, cus=cus, epilogue_one=True),
            "e2c": h2g.debug_ntt_plan(ek, N, n * (j - 1), cus=cus, epilogue_one=False),
            "subcoset": h2g.debug_ntt_plan(k, n, n, count=count, in_twist=True, cus=cus, epilogue_one=True)}


# (j, k) -> extended_k, the split of the extended transforms, the first pass of
# coeff_to_extended, and what of the 2^extended_k outputs extended_to_coeff keeps (out_len =
# keep[0] N / keep[1] < N: the truncated last pass with its epilogue product, every case)
CASES = {
    (4, 9): (11, (5, 6), "plain", (3, 4)),
    (6, 9): (12, (6, 6), "plain", (5, 8)),
    (7, 10): (13, (3, 4, 6), "sparse", (6, 8)),     # 8n: x[1] is all zero
    (8, 11): (14, (3, 5, 6), "sparse", (7, 8)),     # 8n: x[1] is all zero
    (4, 13): (15, (3, 6, 6), "sparse", (3, 4)),     # 4n: both inputs present
    (10, 11): (15, (3, 6, 6), "sparse", (9, 16)),   # 16n: half of x[0] zero as well
    (12, 12): (16, (4, 6, 6), "plain", (11, 16)),
    (16, 13): (17, (5, 6, 6), "plain", (15, 16)),
    (6, 15): (18, (6, 6, 6), "plain", (5, 8)),      # persistent middle pass
    (7, 16): (19, (3, 4, 6, 6), "sparse", (6, 8)),  # four passes: two middle digits under truncation
    (4, 18): (20, (3, 5, 6, 6), "sparse", (3, 4)),  # the 5-bit middle digit; ragged-free persistent passes
}


def require(j, k):
    """assert that Domain(j, k) takes the kernels it is listed for; -> its plans"""
    ek, split, first, keep = CASES[(j, k)]
    assert extended_k(j, k) == ek, (j, k)
    pl = domain_plans(j, k)
    N, n = 1 << ek, 1 << k
    for name in ("c2e", "e2c"):
        assert pl[name]["split"] == split, (j, k, name, pl[name])
    assert pl["c2e"]["first"] == first and (pl["c2e"]["trunc"], pl["c2e"]["one"]) == (False, True), (j, k, pl["c2e"])
    assert n * (j - 1) * keep[1] == N * keep[0] and n * (j - 1) < N, (j, k)
    assert pl["e2c"]["first"] == "plain" and (pl["e2c"]["trunc"], pl["e2c"]["one"]) == (True, False), (j, k, pl["e2c"])
    if first == "sparse":
        assert 4 * n <= N and split[0] == 3
    assert set(pl["e2c"]["pgrid"]) == set(range(1, len(split) - 1))
    return pl


KINDS = ["random", "storage_rm1", "canonical_rm1", "alternating", "alternating_canonical", "spikes", "spike_last",
         "zero"]


def vector(kind, n, seed=0):
    """random, all zero, and the six adversarial kinds of test_gpu_adversarial: the stored
    integer r - 1 and the element r - 1 everywhere, each alternating with 0, and spikes"""
    out = np.zeros((n, 4), dtype=np.uint64)
    can_rm1 = O.fr_from_canonical(R_MINUS_1.copy())[0]  # the element r - 1
    if kind == "random":
        return O.random_fr(np.random.default_rng(seed), n)
    if kind == "zero":
        return out
    if kind == "storage_rm1":
        out[:] = R_MINUS_1
    elif kind == "canonical_rm1":
        out[:] = can_rm1
    elif kind == "alternating":
        out[1::2] = R_MINUS_1
    elif kind == "alternating_canonical":
        out[::2] = can_rm1
    elif kind == "spikes":
        out[0] = R_MINUS_1
        out[n // 2 + 1] = R_MINUS_1
        out[n - 1] = R_MINUS_1
    elif kind == "spike_last":
        out[n - 1] = can_rm1
    else:
        raise ValueError(kind)
    return out
