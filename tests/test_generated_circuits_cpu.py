"""The generated circuits of tests/_gen_circuit.py, pinned on the CPU: for every case of the
committed list the oracle returns a proof, oracle/py/verifier.py accepts it, the plain-Python
MockProver restatement finds no failure, and a second call gives identical arrays.  Then what
the whole list covers is asserted shape by shape, so thinning the list fails here.  The device
is compared with the oracle on the same list in tests/test_gpu_generated_circuits.py."""
import numpy as np
import pytest

import _check_ref as CR
import _gen_circuit as G
import _oracle as O
import h2g_circuit as hc
import verifier as V
from h2g_circuit import ADVICE, FIXED, INSTANCE, OP_CHALLENGE, OP_CONST, OP_NEG, OP_PROD, OP_QUERY, OP_SUM

_made = {}


def made(i):
    if i not in _made:
        _made[i] = G.generate(**G.CASES[i])
    return _made[i]


def _instances(circ, wit):
    return [hc.mont_to_ints(wit.instance[i])[: int(wit.instance_lens[i])] for i in range(circ.num_instance)]


def _same(a, b):
    (ca, wa, _), (cb, wb, _) = a, b
    return (np.array_equal(ca.nodes, cb.nodes) and np.array_equal(ca.constants, cb.constants)
            and np.array_equal(ca.fixed_values, cb.fixed_values) and np.array_equal(ca.copies, cb.copies)
            and np.array_equal(ca.gate_roots, cb.gate_roots) and np.array_equal(ca.lookup_roots, cb.lookup_roots)
            and np.array_equal(ca.shuffle_roots, cb.shuffle_roots) and np.array_equal(ca.perm_array, cb.perm_array)
            and np.array_equal(ca.transcript_repr(), cb.transcript_repr())
            and np.array_equal(wa.advice, wb.advice) and np.array_equal(wa.instance, wb.instance))


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=[G.case_id(c) for c in G.CASES])
def test_case_is_valid(i):
    circ, wit, fill = made(i)
    s, g, gl = O.srs(circ.k)
    chs = []
    proof = O.create_proof(circ, wit, g, gl, fill=fill, challenges_out=chs)
    assert V.verify(circ, _instances(circ, wit), proof, s)
    full = fill.full(chs) if fill else wit
    assert CR.check(circ, full, chs) == set()
    if fill:
        assert O.create_proof(circ, full, g, gl) == proof
    again = G.generate(**G.CASES[i])
    assert _same((circ, full, None), (again[0], again[2].full(chs) if fill else again[1], None))
    if circ.k <= 7:   # another witness of the same circuit (two circuits in one proof)
        other = G.generate(**G.CASES[i], witness_seed=9000 + i)
        assert np.array_equal(other[0].transcript_repr(), circ.transcript_repr())
        w2 = other[2].full(chs) if fill else other[1]
        assert not np.array_equal(w2.advice, full.advice)
        assert CR.check(circ, w2, chs) == set()


# ----------------------------------------------------------------------------- coverage
def _spine(e, side):
    """binary operations down one side of the tree (a NEG between them does not end the run)"""
    m = 0
    while True:
        while e.op == OP_NEG:
            e = e.a
        if e.op not in (OP_SUM, OP_PROD):
            return m
        m += 1
        e = e.a if side == 0 else e.b


def _facts(circ, wit):
    f = set()
    rs = G.roots(circ)
    n = circ.n
    ids = {}
    rots = {}
    for r in rs:
        if r.op == OP_QUERY:
            f.add("root bare query")
        if r.op == OP_CONST:
            f.add("root bare constant")
        for x in G.walk(r):
            ids[id(x)] = ids.get(id(x), 0) + 1
            if x.op == OP_NEG and x.a.op == OP_NEG:
                f.add("NEG(NEG x)")
            if x.op == OP_SUM and x.b.op == OP_NEG and x.b.a.op == OP_NEG:
                f.add("x + NEG(NEG y)")
            if x.op == OP_SUM and x.a.op == OP_NEG and x.b.op != OP_NEG:
                f.add("NEG(x) + y")
            if x.op == OP_QUERY:
                rots.setdefault((x.a, x.b), set()).add(x.c)
                big = abs(x.c) >= n // 2 or x.c == 37
                if x.a == ADVICE and not circ.unblinded[x.b]:
                    assert abs(x.c) <= 3, "a blinded advice query beyond +-3"
                elif big:
                    f.add(("large rotation", "unblinded advice" if x.a == ADVICE else x.a))
        if max(_spine(r, 0), max(_spine(x, 0) for x in G.walk(r))) >= 12:
            f.add("left chain")
        if max(_spine(x, 1) for x in G.walk(r)) >= 12:
            f.add("right chain")
        for x in G.walk(r):
            if x.op in (OP_SUM, OP_PROD) and G.sethi_ullman(x) >= 6 and G.sethi_ullman(x.a) == G.sethi_ullman(x.b):
                f.add("balanced, Sethi-Ullman >= 6")
    # a sub-expression object used twice (the walk meets it twice; leaves do not count)
    seen_twice = [i for i, c in ids.items() if c > 1]
    if any(True for r in rs for x in G.walk(r) if id(x) in seen_twice and x.op in (OP_SUM, OP_PROD)):
        f.add("shared sub-expression")
    if circ.num_constants >= 40:
        f.add(">= 40 constants")
    consts = set(hc.mont_to_ints(circ.constants[: circ.num_constants]))
    f |= {("constant", v) for v in G.EDGE if v in consts}
    if any(len(v) >= 6 for (t, c), v in rots.items() if t == ADVICE and not circ.unblinded[c]):
        assert circ.blinding_factors() >= 8
        f.add("six rotations of a blinded column")
    d = circ.degree()
    ek = (d - 2).bit_length()   # extended_k - k = ceil(log2(degree - 1))
    f.add(("extended_k - k", ek))
    nsets = -(-len(circ.perm_columns) // (d - 2))
    assert {t for t, _ in circ.perm_columns} == {ADVICE, FIXED, INSTANCE} and len(circ.copies) > 0
    if d == 3 and nsets >= 3:
        f.add("nsets >= 3 at degree 3")
    if d >= 6 and nsets >= 2:
        f.add("nsets >= 2 at degree >= 6")
    for a, b in circ.lookups:
        f.add(("lookup expressions", len(a)))
        if any(e.op in (OP_SUM, OP_PROD) for e in b):
            f.add("compound table expression")
        if any(x.op == OP_QUERY and x.a == ADVICE for e in b for x in G.walk(e)):
            f.add("table over advice")
        if any(x.op == OP_CHALLENGE for e in a + b for x in G.walk(e)):
            f.add("challenge in a lookup")
    tabs = [tuple(id(e) for e in b) for _, b in circ.lookups]
    if len(set(tabs)) < len(tabs):
        f.add("two lookups, one table")
    if circ.shuffles:
        f.add("shuffle")
    if any(x.op == OP_CHALLENGE for g in circ.gates for x in G.walk(g)):
        assert list(circ.challenge_phase[: circ.num_challenges]) == [0, 1] and circ.max_phase == 2
        f.add("challenge in a gate")
    if circ.k == 10:
        f.add("k = 10")
    # witness values: about 30 % from the edge list, all canonical
    u = circ.usable_rows()
    vals = [v for c in range(G.NFREE) for v in hc.mont_to_ints(wit.advice[c][:u])] if wit.advice.any() else []
    if vals:
        frac = sum(v in G.EDGE for v in vals) / len(vals)
        assert 0.2 < frac < 0.4, frac
    limbs = np.asarray(wit.advice, dtype=np.uint64).reshape(-1, 4)
    as_int = [sum(int(l[i]) << (64 * i) for i in range(4)) for l in limbs[:: max(len(limbs) // 512, 1)]]
    assert all(v < hc.R_MOD for v in as_int)
    return f


WANTED = (["NEG(NEG x)", "x + NEG(NEG y)", "NEG(x) + y", "left chain", "right chain", "balanced, Sethi-Ullman >= 6",
           "shared sub-expression", "root bare query", "root bare constant", ">= 40 constants",
           "six rotations of a blinded column", "nsets >= 3 at degree 3", "nsets >= 2 at degree >= 6",
           "compound table expression", "table over advice", "two lookups, one table", "shuffle",
           "challenge in a gate", "challenge in a lookup", "k = 10"]
          + [("constant", v) for v in G.EDGE] + [("extended_k - k", j) for j in (1, 2, 3, 4)]
          + [("lookup expressions", m) for m in (1, 2, 3)]
          + [("large rotation", t) for t in (FIXED, INSTANCE, "unblinded advice")])


def test_the_list_covers_every_shape():
    assert 38 <= len(G.CASES) <= 44 and len({c["seed"] for c in G.CASES}) == len(G.CASES)
    have = set()
    for i in range(len(G.CASES)):
        circ, wit, fill = made(i)
        have |= _facts(circ, fill.full([3, 5]) if fill else wit)
    missing = [w for w in WANTED if w not in have]
    assert not missing, missing


# ----------------------------------------------------------------------------- the large cases
@pytest.mark.parametrize("i", range(len(G.LARGE_CASES)), ids=[G.case_id(c) for c in G.LARGE_CASES])
def test_large_case_is_valid(i):
    """G.LARGE_CASES: one phase, satisfied, deterministic, and an extended domain above 2^10 of
    which h(X) fills a part that is no power of two"""
    circ, wit, fill = G.generate(**G.LARGE_CASES[i])
    assert fill is None
    d = circ.degree()
    ek = circ.k + (d - 2).bit_length()
    assert d == G.LARGE_CASES[i]["degree"] and 13 <= ek <= 16
    assert (d - 1) & (d - 2) and (d - 1) << circ.k < 1 << ek
    assert CR.check(circ, wit, []) == set()
    assert _same((circ, wit, None), G.generate(**G.LARGE_CASES[i]))


def test_the_large_list_splits_h_unevenly_at_every_extension():
    assert len({c["seed"] for c in G.LARGE_CASES + G.CASES}) == len(G.LARGE_CASES) + len(G.CASES)
    kept = set()
    for c in G.LARGE_CASES:
        e = (c["degree"] - 2).bit_length()
        kept.add((c["degree"] - 1, 1 << e))
    assert kept == {(3, 4), (6, 8), (5, 8), (7, 8), (11, 16), (15, 16)}


# ----------------------------------------------------------------------------- refused proofs
@pytest.mark.parametrize("make", [G.zero_table_lookup, G.unblinded_boolean], ids=lambda f: f.__name__)
def test_oracle_refuses_an_identity_commitment(make):
    """a commitment at infinity (the top piece of h(X) under an all-zero table, an all-zero
    unblinded advice column) is what the reference's transcript refuses to write: the
    restatement fails with -5 although the witness satisfies the circuit; the sibling proves"""
    circ, wit = make(6, zero=True)
    s, g, gl = O.srs(circ.k)
    assert CR.check(circ, wit) == set()
    with pytest.raises(ValueError, match="failed: -5$"):
        O.create_proof(circ, wit, g, gl)
    circ, wit = make(6, zero=False)
    assert V.verify(circ, [], O.create_proof(circ, wit, g, gl), s)
