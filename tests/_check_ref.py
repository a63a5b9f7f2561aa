"""Plain-Python restatement of h2g_check_witness's semantics (include/h2g.h), itself a
restatement of MockProver::verify (halo2_frontend/src/dev.rs:742-1166) for a complete
witness -- the yardstick of tests/test_gpu_check_witness.py, pinned by
tests/test_check_witness_cpu.py.

Exact where the device is probabilistic: lookup and shuffle tuples are compared as tuples.
Rows [u, n) of the advice (u = usable_rows()) are filled as the prover will fill them: zero
for unblinded columns, random field elements (Python's own generator) for the others.
"""
import random

import numpy as np

import h2g_circuit as hc

GATE, GATE_BLINDING, LOOKUP, SHUFFLE, COPY = 1, 2, 3, 4, 5
NO_ROW = 0xFFFFFFFF


CH6 = [12345, 2**200 + 7]   # challenge_circuit's two challenges in the anchors
CH_MY = [987654321]         # my_circuit's challenge


def set_cell(wit, col, row, value):
    """a copy of wit with advice[col][row] := value (canonical int)"""
    adv = wit.advice.copy()
    adv[col, row] = hc.fr_to_limbs(value)
    return hc.Witness(adv, wit.instance, wit.instance_lens)


def valid_cases():
    """[(name, circuit, witness, challenges)]: valid witnesses, no failures"""
    out = [("simple_example", *hc.simple_example(6), []), ("mixed", *hc.mixed_circuit(7), []),
           ("lookup", *hc.lookup_circuit(7), [])]
    c, _, fill = hc.challenge_circuit(6)
    out.append(("challenge", c, fill.full(CH6), CH6))
    c, _, fill = hc.challenge_circuit(6, extended=True)
    out.append(("challenge+", c, fill.full(CH6), CH6))
    c, _, fill = hc.my_circuit(6)
    out.append(("my_circuit", c, fill.full(CH_MY), CH_MY))
    return out


def corrupted_cases():
    """[(name, circuit, witness, challenges, expected failure set)]"""
    out = []
    c, w = hc.mixed_circuit(7)
    d10 = hc.fr_from_limbs(w.advice[3, 10])
    out.append(("mixed D[9]:=D[10]", c, set_cell(w, 3, 9, d10), [], {(1, 0, 9), (1, 3, 9)}))
    c, w = hc.lookup_circuit(7)
    out.append(("lookup A[5]:=300", c, set_cell(w, 0, 5, 300), [],
                {(1, 0, 5), (3, 0, 5), (3, 1, 5), (3, 2, 4), (5, 2, 5)}))
    out.append(("lookup D[2]:=1", c, set_cell(w, 3, 2, 1), [], {(4, 0, NO_ROW)}))
    c, _, fill = hc.my_circuit(6)
    out.append(("my_circuit other challenge", c, fill.full(CH_MY), [5],
                {(1, g, r) for g in (1, 2) for r in (29, 31, 33)}))
    c, w = hc.simple_example(6)   # u = 58: the selector live in the last usable row and in a blinding row
    c.fixed_values[1, 57] = c.fixed_values[1, 60] = hc.fr_to_limbs(1)
    out.append(("simple_example s_mul rows 57, 60", c, w, [], {(1, 0, 57), (2, 0, 60)}))
    return out


def columns(circ, wit, seed=0):
    """(advice, fixed, instance) as lists of n canonical ints per column, the advice with its
    rows [u, n) filled as the prover fills them"""
    n, u = circ.n, circ.usable_rows()
    rng = random.Random(seed)
    adv = [hc.mont_to_ints(wit.advice[c]) for c in range(circ.num_advice)]
    for c in range(circ.num_advice):
        for r in range(u, n):
            adv[c][r] = 0 if circ.unblinded[c] else rng.randrange(hc.R_MOD)
    fix = [hc.mont_to_ints(circ.fixed_values[c]) for c in range(circ.num_fixed)]
    ins = [hc.mont_to_ints(wit.instance[c]) for c in range(circ.num_instance)]
    return adv, fix, ins


def check(circ, wit, challenges=(), seed=0, copies=True):
    """-> set of (kind, index, row)"""
    n, u = circ.n, circ.usable_rows()
    adv, fix, ins = columns(circ, wit, seed)
    cols = {hc.ADVICE: adv, hc.FIXED: fix, hc.INSTANCE: ins}
    ch = [int(c) % hc.R_MOD for c in challenges]

    def at(e, row):  # (an Expr constant carries its value, not an index into circ.constants)
        return e.evaluate(lambda v: v, lambda t, i, rot: cols[t][i][(row + rot) % n], challenge=lambda i: ch[i])

    out = set()
    for g, e in enumerate(circ.gates):
        for row in range(n):
            if at(e, row):
                out.add((GATE if row < u else GATE_BLINDING, g, row))
    for l, (inputs, table) in enumerate(circ.lookups):
        have = {tuple(at(e, row) for e in table) for row in range(u)}
        for row in range(u):
            if tuple(at(e, row) for e in inputs) not in have:
                out.add((LOOKUP, l, row))
    for s, (inputs, shuffle) in enumerate(circ.shuffles):
        a = sorted(tuple(at(e, row) for e in inputs) for row in range(u))
        b = sorted(tuple(at(e, row) for e in shuffle) for row in range(u))
        if a != b:
            out.add((SHUFFLE, s, NO_ROW))
    if copies:
        for i, (lt, li, lr, rt, ri, rr) in enumerate(np.asarray(circ.copies).reshape(-1, 6).tolist()):
            if cols[lt][li][lr] != cols[rt][ri][rr]:
                out.add((COPY, i, lr))
    return out
