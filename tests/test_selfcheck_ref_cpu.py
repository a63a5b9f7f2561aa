"""tests/_selfcheck_ref.py on hand-made arrays: what each of its checks reports for a correct
argument and for each way an argument can be wrong.  Small numbers, worked by hand in the
comments, so that the yardstick of the GPU tests does not rest on itself."""
import _selfcheck_ref as S

R = S.R
P7, P8 = S.PRODUCT, S.PERMUTED_PAIR


def inv(x):
    return pow(x, -1, R)


# n = 8, u = 5 (rows 5, 6, 7 are the blinding rows); beta = 2, gamma = 3.
# A' is a permutation of A and S' of S, so the product closes.
A = [5, 1, 4, 1, 5]
S_ = [1, 4, 5, 9, 9]
AP = [1, 1, 4, 5, 5]
SP = [1, 9, 4, 5, 9]
BETA, GAMMA, U, N = 2, 3, 5, 8


def lookup_z():
    return S.make_product(A, S_, AP, SP, BETA, GAMMA, U, N, filler=77)


def test_a_correct_lookup_product():
    z = lookup_z()
    assert z[0] == 1 and len(z) == N and z[6] == 77
    # row 0 by hand: z[1] = (5 + 2)(1 + 3) / ((1 + 2)(1 + 3)) = 7 / 3
    assert z[1] == 7 * inv(3) % R
    assert z[U] == 1   # the same multisets on both sides
    assert S.product_check(z, A, S_, AP, SP, BETA, GAMMA, U) == set()
    assert S.permuted_check(AP, SP, U) == set()


def test_z0_not_one():
    z = lookup_z()
    z[0] = 2
    # row 0 fails twice over (z[0] != 1, and z[1] no longer follows from it): ONE record
    assert S.product_check(z, A, S_, AP, SP, BETA, GAMMA, U) == {(P7, 0, 0)}
    # a z scaled throughout keeps every recurrence: only the ends say so
    z = [2 * v % R for v in lookup_z()]
    assert S.product_check(z, A, S_, AP, SP, BETA, GAMMA, U) == {(P7, 0, 0), (P7, 0, U)}


def test_one_wrong_z_fails_the_rows_on_both_sides():
    for i in (1, 2, 4):
        z = lookup_z()
        z[i] = (z[i] + 1) % R
        assert S.product_check(z, A, S_, AP, SP, BETA, GAMMA, U, index=3) == {(P7, 3, i - 1), (P7, 3, i)}


def test_closing_value():
    z = lookup_z()
    z[U] = 5
    # z[u] enters row u - 1's recurrence and is the closing value
    assert S.product_check(z, A, S_, AP, SP, BETA, GAMMA, U) == {(P7, 0, U - 1), (P7, 0, U)}
    assert S.product_check(z, A, S_, AP, SP, BETA, GAMMA, U, closing=False) == {(P7, 0, U - 1)}
    # a witness whose multisets differ: every recurrence holds, the product does not close
    a2 = [5, 1, 4, 1, 6]
    z = S.make_product(a2, S_, AP, SP, BETA, GAMMA, U, N)
    assert z[U] == (6 + BETA) * inv(5 + BETA) % R
    assert S.product_check(z, a2, S_, AP, SP, BETA, GAMMA, U) == {(P7, 0, U)}
    # the blinding rows above u are never read
    z[6] = z[7] = 123456
    assert S.product_check(z, a2, S_, AP, SP, BETA, GAMMA, U) == {(P7, 0, U)}


def test_one_factor_form():
    a, s = [3, 1, 2, 0], [0, 3, 2, 1]
    z = S.make_product(a, None, s, None, BETA, GAMMA, 4, 6)
    # by hand: z[1] = (3 + 3) / (0 + 3) = 2 -- gamma, not beta, goes with the single factor
    assert z[1] == 2 and z[4] == 1
    assert S.product_check(z, a, None, s, None, BETA, GAMMA, 4) == set()
    assert S.product_check(z, a, None, s, None, GAMMA, BETA, 4) != set()   # the constants swapped
    z[2] = 0
    assert S.product_check(z, a, None, s, None, BETA, GAMMA, 4) == {(P7, 0, 1), (P7, 0, 2)}


def test_permuted_pair_with_one_stray_value():
    ap = list(AP)
    ap[3] = 6                      # neither S'[3] = 5 nor A'[2] = 4
    assert S.permuted_check(ap, SP, U, index=2) == {(P8, 2, 3), (P8, 2, 4)}   # and A'[4] = 5 lost its run
    sp = list(SP)
    sp[0] = 2                      # row 0 has no row before it to repeat
    assert S.permuted_check(AP, sp, U) == {(P8, 0, 0)}
    sp = list(SP)
    sp[1] = 2                      # A'[1] = 1 repeats A'[0]: the table side is free there
    assert S.permuted_check(AP, sp, U) == set()
    assert S.permuted_check(ap, SP, 3) == set()   # rows >= u are not read


def test_permutation_set():
    # two columns over u = 3 rows of n = 4 (omega = a 4th root of unity), wired as one 2-cycle
    # between (column 0, row 1) and (column 1, row 2): sigma holds delta^c omega^row of the image
    omega = pow(5, (R - 1) // 4, R)
    delta = 7
    ids = [[pow(omega, i, R) for i in range(4)], [delta * pow(omega, i, R) % R for i in range(4)]]
    sig = [list(ids[0]), list(ids[1])]
    sig[0][1], sig[1][2] = ids[1][2], ids[0][1]
    v = [[10, 42, 12, 0], [20, 21, 42, 0]]      # the two wired cells are equal
    beta, gamma, u = 11, 13, 3

    def build(vals):
        z = [9]
        for i in range(u):
            num = den = 1
            for c in range(2):
                num = num * (vals[c][i] + beta * ids[c][i] + gamma) % R
                den = den * (vals[c][i] + beta * sig[c][i] + gamma) % R
            z.append(z[-1] * num % R * inv(den) % R)
        return z + [0]

    z = build(v)
    assert z[u] == 9                            # closes on its starting value: the copy holds
    args = (v, sig, beta, gamma, [1, delta], omega, u)
    assert S.permutation_check(z, 9, *args) == set()
    assert S.permutation_check(z, 1, *args) == {(S.PERMUTATION, 0, 0)}        # the chaining
    z[2] = (z[2] + 1) % R
    assert S.permutation_check(z, 9, *args, index=1) == {(S.PERMUTATION, 1, 1), (S.PERMUTATION, 1, 2)}
    v2 = [list(v[0]), list(v[1])]
    v2[1][2] = 43                               # a broken copy: every row holds, z[u] != z[0]
    z = build(v2)
    assert S.permutation_check(z, 9, v2, sig, beta, gamma, [1, delta], omega, u) == set()
    assert z[u] != 9


def test_verdict():
    # h = h_0 + X^4 h_1 with h_0 = 1 + 2 X, h_1 = 3 + X^3; at x = 2: 5 + 16 * 11 = 181
    pieces = [[1, 2], [3, 0, 0, 1]]
    assert S.h_at(pieces, 2, 4) == 181
    assert S.verdict(pieces, 2, 4, 181) and S.verdict(pieces, 2, 4, 181 + R)
    assert not S.verdict(pieces, 2, 4, 180)
    assert S.h_at([[R - 1]], 12345, 8) == R - 1
