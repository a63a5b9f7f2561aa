"""Plain-Python restatement, over Python integers mod r, of the prover's self-checks
(include/h2g.h, "the prover's self-checks"; csrc/selfcheck.hip, csrc/vanishing.h) -- the
yardstick of tests/test_selfcheck_kernels_gpu.py, pinned by tests/test_selfcheck_ref_cpu.py.
Written from the formulas, u = the number of usable rows:

  S2  permuted pair      for i < u:  a'[i] == s'[i], or i > 0 and a'[i] == a'[i-1]
  S3  lookup product     z[0] = 1;  for i < u:  z[i+1] (a'[i] + beta) (s'[i] + gamma)
                                              = z[i] (A[i] + beta) (S[i] + gamma);  z[u] = 1
  S4  shuffle product    z[0] = 1;  for i < u:  z[i+1] (gamma + S[i]) = z[i] (gamma + A[i])
  S5  permutation set    z[0] = first;  for i < u:  z[i+1] prod_c (v_c[i] + beta sigma_c[i] + gamma)
                                              = z[i] prod_c (v_c[i] + beta delta^c omega^i + gamma)
  verdict                h(x) = sum_i x^(n i) h_i(x)  against  expected_h

A row that fails any of its conditions gives one record (kind, index, row); row u carries only
the closing value.
"""
import h2g_circuit as hc

R = hc.R_MOD
PERMUTATION, PRODUCT, PERMUTED_PAIR, UNUSABLE_ROW, IDENTITY = 6, 7, 8, 9, 10


def product_check(z, num_a, num_b, den_a, den_b, beta, gamma, u, index=0, closing=True):
    """S3 (two factors) or, with num_b = den_b = None, S4 (one factor: gamma goes with it)"""
    one_factor = num_b is None
    assert (den_b is None) == one_factor
    ca = gamma if one_factor else beta
    out = set()
    for i in range(u):
        left = z[i + 1] * (den_a[i] + ca)
        right = z[i] * (num_a[i] + ca)
        if not one_factor:
            left *= den_b[i] + gamma
            right *= num_b[i] + gamma
        if (left - right) % R or (i == 0 and z[0] % R != 1):
            out.add((PRODUCT, index, i))
    if closing and z[u] % R != 1:
        out.add((PRODUCT, index, u))
    return out


def make_product(num_a, num_b, den_a, den_b, beta, gamma, u, n, filler=0):
    """the z a prover builds: z[0] = 1, z[i+1] = z[i] num / den for i < u; rows above u: filler"""
    one_factor = num_b is None
    ca = gamma if one_factor else beta
    z = [1]
    for i in range(u):
        num = num_a[i] + ca
        den = den_a[i] + ca
        if not one_factor:
            num *= num_b[i] + gamma
            den *= den_b[i] + gamma
        z.append(z[-1] * num % R * pow(den % R, -1, R) % R)
    return z + [filler] * (n - u - 1)


def permuted_check(a, s, u, index=0):
    """S2"""
    return {(PERMUTED_PAIR, index, i) for i in range(u)
            if (a[i] - s[i]) % R and not (i > 0 and (a[i] - a[i - 1]) % R == 0)}


def permutation_check(z, first, values, sigmas, beta, gamma, delta_pows, omega, u, index=0):
    """S5 for one column set: values[c], sigmas[c] the set's columns, delta_pows[c] = delta^(the
    column's index in the whole permutation)"""
    out = set()
    w = 1
    for i in range(u):
        left, right = z[i + 1], z[i]
        for v, s, d in zip(values, sigmas, delta_pows):
            left = left * (v[i] + beta * s[i] + gamma) % R
            right = right * (v[i] + beta * d % R * w + gamma) % R
        if (left - right) % R or (i == 0 and (z[0] - first) % R):
            out.add((PERMUTATION, index, i))
        w = w * omega % R
    return out


def h_at(pieces, x, n):
    """h(x) = sum_i x^(n i) h_i(x), each piece a list of at most n coefficients (Horner)"""
    xn = pow(x, n, R)
    acc = 0
    for piece in reversed(pieces):
        v = 0
        for c in reversed(piece):
            v = (v * x + c) % R
        acc = (acc * xn + v) % R
    return acc


def verdict(pieces, x, n, expected_h):
    """the proof verifies iff h(x) is what the verifier expects"""
    return h_at(pieces, x, n) == expected_h % R
