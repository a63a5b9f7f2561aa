"""The slots of a proof, from the circuit alone, and the mutations the binding tests apply.

A proof is a sequence of 32-byte slots: compressed G1 points and canonical Fr scalars in the
order verify_proof reads them (reference paths relative to halo2_backend/src):
  plonk/verifier.rs:145-256    advice per phase, lookup permuted, permutation / lookup / shuffle
                               products, the random polynomial, the h pieces
  plonk/verifier.rs:307-347    advice, fixed, random, sigma, permutation-set, lookup and shuffle
                               evaluations
  plonk/permutation/verifier.rs:33-95, lookup/verifier.rs:36-90, shuffle/verifier.rs:27-55,
  vanishing/verifier.rs:40-85
  poly/kzg/multiopen/shplonk/verifier.rs:45-75   h1, h2
  poly/kzg/multiopen/gwc/verifier.rs:42-60       one witness per distinct opening point, in the
                                                 first-appearance order of plonk/verifier.rs:449-501
`slots` knows nothing of either verifier under test: it reads the circuit's queries, degree,
blinding factors, phases, lookups, shuffles and permutation columns, so a test that asserts
len(slots) * 32 == len(proof) and sweeps every slot cannot share a verifier's miscount.
"""
import bn254_ref as B

POINT, SCALAR = "point", "scalar"


def opening_rotations(circ):
    """the distinct rotations (mod n) of verify_proof's queries, first appearance first"""
    adv_q, fix_q, _ = circ.queries()
    nsets = num_perm_sets(circ)
    rots = [r for _, r in adv_q]
    if nsets:
        rots += [0, 1]
        if nsets > 1:
            rots.append(-(circ.blinding_factors() + 1))
    if circ.lookups:
        rots += [0, 0, 0, -1, 1]
    if circ.shuffles:
        rots += [0, 1]
    rots += [r for _, r in fix_q]
    rots.append(0)   # sigma, h(X), the random polynomial
    out = []
    for r in rots:
        if r % circ.n not in out:
            out.append(r % circ.n)
    return out


def num_perm_sets(circ):
    chunk = circ.degree() - 2
    return (len(circ.perm_columns) + chunk - 1) // chunk


def slots(circ, num_circuits=1, multiopen="shplonk"):
    """[(kind, name)] per 32-byte slot of a proof of `num_circuits` circuits of `circ`"""
    adv_q, fix_q, _ = circ.queries()
    nsets = num_perm_sets(circ)
    NC = range(num_circuits)
    out = []

    def point(name):
        out.append((POINT, name))

    def scalar(name):
        out.append((SCALAR, name))

    for ph in range(circ.max_phase + 1):
        for c in NC:
            for col in range(circ.num_advice):
                if int(circ.advice_phase[col]) == ph:
                    point(f"c{c}.advice{col}")
    for c in NC:
        for l in range(len(circ.lookups)):
            point(f"c{c}.lookup{l}.permuted_input")
            point(f"c{c}.lookup{l}.permuted_table")
    for c in NC:
        for i in range(nsets):
            point(f"c{c}.perm_set{i}.product")
    for c in NC:
        for l in range(len(circ.lookups)):
            point(f"c{c}.lookup{l}.product")
    for c in NC:
        for l in range(len(circ.shuffles)):
            point(f"c{c}.shuffle{l}.product")
    point("random")
    for i in range(circ.degree() - 1):   # quotient_poly_degree
        point(f"h[{i}]")

    for c in NC:
        for col, rot in adv_q:
            scalar(f"c{c}.advice{col}@{rot}.eval")
    for col, rot in fix_q:
        scalar(f"fixed{col}@{rot}.eval")
    scalar("random.eval")
    for i in range(len(circ.perm_columns)):
        scalar(f"sigma{i}.eval")
    for c in NC:
        for i in range(nsets):
            scalar(f"c{c}.perm_set{i}.eval")
            scalar(f"c{c}.perm_set{i}.eval_next")
            if i + 1 < nsets:
                scalar(f"c{c}.perm_set{i}.eval_last")
    for c in NC:
        for l in range(len(circ.lookups)):
            for what in ("product_eval", "product_next_eval", "permuted_input_eval", "permuted_input_inv_eval",
                         "permuted_table_eval"):
                scalar(f"c{c}.lookup{l}.{what}")
    for c in NC:
        for l in range(len(circ.shuffles)):
            scalar(f"c{c}.shuffle{l}.product_eval")
            scalar(f"c{c}.shuffle{l}.product_next_eval")

    if multiopen == "shplonk":
        point("shplonk.h1")
        point("shplonk.h2")
    else:
        for r in opening_rotations(circ):
            point(f"gwc.w[omega^{r if r <= circ.n // 2 else r - circ.n}]")
    return out


def counts(layout):
    """(head points, scalars, tail points)"""
    kinds = [k for k, _ in layout]
    head = kinds.index(SCALAR)
    nsc = kinds.count(SCALAR)
    assert kinds == [POINT] * head + [SCALAR] * nsc + [POINT] * (len(kinds) - head - nsc)
    return head, nsc, len(kinds) - head - nsc


# ----------------------------------------------------------------------------- mutations
def _get(proof, i):
    return bytes(proof[32 * i:32 * i + 32])


def _put(proof, i, b):
    assert len(b) == 32
    out = bytes(proof[:32 * i]) + bytes(b) + bytes(proof[32 * i + 32:])
    assert len(out) == len(proof) and out != bytes(proof)
    return out


def _x_sign(b):
    return int.from_bytes(b, "little") & ((1 << 255) - 1), b[31] >> 7


def _point_bytes(x, sign):
    assert x < 1 << 255
    return (x | (sign << 255)).to_bytes(32, "little")


def negate(proof, i):
    """a point's y sign flipped: another valid encoding, of -P"""
    b = bytearray(_get(proof, i))
    b[31] ^= 0x80
    return _put(proof, i, b)


def plus_one(proof, i):
    v = int.from_bytes(_get(proof, i), "little")
    assert v < B.R
    return _put(proof, i, ((v + 1) % B.R).to_bytes(32, "little"))


def next_x(proof, i):
    """-> (bytes, decodes): x + 1 with the sign bit kept; `decodes` is bn254_ref's verdict on
    the new encoding (a point other than the identity), never a verifier's"""
    x, sign = _x_sign(_get(proof, i))
    b = _point_bytes(x + 1, sign)
    ok, pt = B.g1_from_bytes(b)
    return _put(proof, i, b), bool(ok and pt is not None)


def alias(proof, i, kind):
    """the same value in a non-canonical encoding: v + r (2r < 2^256), x + p (2p < 2^255)"""
    b = _get(proof, i)
    if kind == SCALAR:
        return _put(proof, i, (int.from_bytes(b, "little") + B.R).to_bytes(32, "little"))
    x, sign = _x_sign(b)
    return _put(proof, i, _point_bytes(x + B.P, sign))


def can_swap(proof, layout, i):
    return i + 1 < len(layout) and layout[i][0] == layout[i + 1][0] and _get(proof, i) != _get(proof, i + 1)


def swap_with_next(proof, i):
    a, b = _get(proof, i), _get(proof, i + 1)
    return _put(_put(proof, i, b), i + 1, a)


def replace_point(proof, i, pt):
    return _put(proof, i, B.g1_to_bytes(pt))


def point_at(proof, i):
    ok, pt = B.g1_from_bytes(_get(proof, i))
    assert ok and pt is not None
    return pt


def mutate_by_kind(proof, layout, i):
    """the mutation that keeps the encoding valid: negate a point, add one to a scalar"""
    return negate(proof, i) if layout[i][0] == POINT else plus_one(proof, i)
