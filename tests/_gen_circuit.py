"""Seeded generator of circuits with satisfying witnesses (test helper, not a conftest).

generate(seed, k, **shape) -> (circuit, witness, fill or None), deterministic from `seed`
(the circuit) and `witness_seed` (the witness; default: the seed).  The cases a test proves
are pinned on the CPU first (tests/test_generated_circuits_cpu.py: the oracle proves them,
oracle/py/verifier.py accepts the proof, tests/_check_ref.py finds no failure) and only then
compared with the device.

Witnesses satisfy the constraints by "solve one cell":
  gate g     q_g (E_g - advice(out_g)),   out_g[row] = E_g(row) where the selector q_g is 1
  lookup     input i = q (advice(cell_i) + F_i) + (1 - q) d_i against table expression T_i,
             cell_i[row] = T_i(a chosen table row) - F_i(row); d = the table's tuple on one row
  shuffle    q (advice(cell) + F) ~ q S,  cell[row] = S(pi(row)) - F(row), pi a permutation
with E, F, T and S random trees over the free columns.  Selectors are 1 on [R, u - R), R the
largest rotation of a blinded advice query, so no active row reads a blinding row; fixed,
instance and unblinded advice columns are deterministic on every row and are also queried at
large rotations.  u comes from a probe Circuit holding the final expressions and permutation.

With challenges=True the circuit has two challenges (phases 0 and 1) as leaves of gate and
lookup expressions; a solved column sits in the phase after the last challenge it depends on
and the witness comes back as fill(phase, challenges) with fill.full(challenges).
"""
import numpy as np

import h2g_circuit as hc
from h2g_circuit import ADVICE, FIXED, INSTANCE, OP_CHALLENGE, OP_NEG, OP_PROD, OP_QUERY, OP_SUM

R = hc.R_MOD
EDGE = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, 2**29, 2**29 - 1, 2**64, 2**253 + 5]
SPECIALS = ("negneg", "sub_nbrs", "left", "right", "balanced", "shared", "many_rot", "bare")
NFREE = 3   # free (blinded) advice columns 0..2; column 3 is the free unblinded one
UNB = 3


def _uniform(rng):
    return int.from_bytes(rng.bytes(32), "little") % R


def _value(rng):
    """~30 % from the edge list, the rest uniform"""
    return EDGE[int(rng.integers(len(EDGE)))] if rng.random() < 0.3 else _uniform(rng)


# ----------------------------------------------------------------------------- tree shape facts
def sethi_ullman(e):
    """registers the tree needs (leaf 1, NEG its child, binary max or equal + 1)"""
    if e.op == OP_NEG:
        return sethi_ullman(e.a)
    if e.op in (OP_SUM, OP_PROD):
        a, b = sethi_ullman(e.a), sethi_ullman(e.b)
        return a + 1 if a == b else max(a, b)
    return 1


def walk(e):
    """every node of the tree, parents first"""
    stack = [e]
    while stack:
        x = stack.pop()
        yield x
        if x.op == OP_NEG:
            stack.append(x.a)
        elif x.op in (OP_SUM, OP_PROD):
            stack += [x.b, x.a]


def roots(circ):
    """every expression root of the circuit: gates, lookup and shuffle expressions"""
    return list(circ.gates) + [e for a, b in circ.lookups + circ.shuffles for e in a + b]


# ----------------------------------------------------------------------------- random trees
class _Trees:
    def __init__(self, rng, n, challenges=(), arots=(-1, 0, 1, 2)):
        self.rng, self.n, self.challenges, self.arots = rng, n, list(challenges), list(arots)
        big = [37 % n, n // 2, -(n // 2), n - 1, -(n - 1)]
        self.big = [0, 0, 1, -1, 2] + big
        self.unb_rots = [0, big[int(rng.integers(len(big)))], big[int(rng.integers(len(big)))]]

    def query(self):
        rng = self.rng
        t = rng.random()
        if t < 0.5:
            return hc.advice(int(rng.integers(NFREE)), self.arots[int(rng.integers(len(self.arots)))])
        if t < 0.7:
            return hc.fixed(int(rng.integers(2)), self.big[int(rng.integers(len(self.big)))])
        if t < 0.85:
            return hc.instance(0, self.big[int(rng.integers(len(self.big)))])
        return hc.advice(UNB, self.unb_rots[int(rng.integers(3))])

    def const(self):
        rng = self.rng
        if self.challenges and rng.random() < 0.35:
            return hc.challenge(self.challenges[int(rng.integers(len(self.challenges)))])
        return hc.const(EDGE[int(rng.integers(len(EDGE)))] if rng.random() < 0.5 else _uniform(rng))

    def leaf(self, d):
        return self.query() if d >= 1 and self.rng.random() < 0.75 else self.const()

    def tree(self, d, size):
        """a random tree of about `size` nodes and degree <= d"""
        rng = self.rng
        if size <= 1:
            return self.leaf(d)
        r = rng.random()
        if r < 0.12:
            return -self.tree(d, size - 1)
        ls = int(rng.integers(1, size - 1)) if size > 2 else 1
        rs = max(size - 1 - ls, 1)
        if r < 0.45:
            return self.tree(d, ls) + self.tree(d, rs)
        if r < 0.6:
            return self.tree(d, ls) - self.tree(d, rs)
        da = int(rng.integers(0, d + 1))
        return self.tree(da, ls) * self.tree(d - da, rs)

    def chain(self, d, ops, left):
        """a chain of `ops` operations leaning to one side"""
        rng = self.rng
        acc = self.query()
        for _ in range(ops):
            r = rng.random()
            if r < 0.3:
                x, mul = self.leaf(1), False
            elif r < 0.55:
                x, mul = -self.leaf(1), False       # a - b as the frontend writes it
            elif r < 0.8 or acc.degree() >= d:
                x, mul = self.const(), True
            else:
                x, mul = self.query(), True
            if left:
                acc = acc * x if mul else acc + x
            else:
                acc = x * acc if mul else x + acc
        return acc

    def balanced(self, depth, d):
        if depth == 0:
            return self.leaf(d) if d < 1 else self.query()
        if d >= 2 and (1 << depth) <= d:
            return self.balanced(depth - 1, d // 2) * self.balanced(depth - 1, d - d // 2)
        a, b = self.balanced(depth - 1, d), self.balanced(depth - 1, d)
        return a + b if self.rng.random() < 0.6 else a - b

    def special(self, name, d):
        small = lambda: self.tree(min(d, 2), int(self.rng.integers(3, 9)))  # noqa: E731
        if name == "negneg":
            return -(-small()) * self.const() + -(-(-self.query()))
        if name == "sub_nbrs":
            return (small() + -(-small())) + ((-small()) + small())
        if name == "left":
            return self.chain(d, 14, True)
        if name == "right":
            return self.chain(d, 14, False)
        if name == "balanced":
            return self.balanced(5, d)
        if name == "shared":
            s = self.tree(max(d // 2, 1), 12)
            return (s + self.const()) * s if d >= 2 else s + s
        if name == "many_rot":   # six rotations of one blinded column: blinding_factors() = 8
            e = self.const() * hc.advice(0, -3)
            for rot in (-2, -1, 0, 1, 2):
                e = e + self.const() * hc.advice(0, rot)
            return e
        raise ValueError(name)


def _max_advice_rot(exprs):
    return max([abs(x.c) for e in exprs for x in walk(e) if x.op == OP_QUERY and x.a == ADVICE and x.b != UNB] + [0])


def _challenges_of(exprs):
    return {x.a for e in exprs for x in walk(e) if x.op == OP_CHALLENGE}


# ----------------------------------------------------------------------------- the generator
def generate(seed, k, degree=5, gates=2, nodes=(30, 120), special=None, lookups=(), twin=False,
             advice_table=False, plain_lookup=False, shuffle=False, challenges=False, copies=6,
             witness_seed=None):
    """degree: the circuit's declared degree (one product-chain gate has exactly it; >= 3);
    gates: random gates of `nodes` nodes; special: names from SPECIALS (None: three drawn from
    the seed, "all": every one); lookups: the expression count of each lookup (a 3-expression
    lookup leads with a constant tag); twin: one more lookup over lookup 0's table expressions;
    advice_table: lookup 0's first table expression reads an advice column; plain_lookup: one
    lookup [advice] in [fixed] with bare queries as roots; shuffle; challenges; copies: how many
    copy constraints of each kind."""
    n = 1 << k
    rng = np.random.default_rng([int(seed), 0x6E6])
    chal = [0, 1] if challenges else []
    T = _Trees(rng, n, chal)
    d = degree - 1                      # the budget of E in q (E - out)
    assert degree >= 3
    if (lookups or twin or plain_lookup or shuffle) and degree < 5:
        raise ValueError("lookups and shuffles here need degree >= 5")
    if special is None:
        special = [SPECIALS[int(i)] for i in rng.choice(len(SPECIALS), size=3, replace=False)]
    elif special == "all":
        special = list(SPECIALS)

    # ---- expressions (none depends on u)
    NFIX_DATA = 2                       # fixed 0, 1: data; then the table columns; then selectors
    E = []                              # gate bodies; gate g's solved column is the g-th out column
    chain = hc.advice(0)
    for i in range(1, d):
        chain = chain * (hc.advice(i % NFREE, T.arots[i % len(T.arots)]) if i % 3 else hc.fixed(i % 2, i % 2))
    E.append(chain)
    for _ in range(gates):
        E.append(T.tree(d, int(rng.integers(nodes[0], nodes[1] + 1))))
    bare = "bare" in special
    for name in special:
        if name != "bare":
            E.append(T.special(name, d))
    gate_chal = []                      # challenges gate g may use: none / c0 / c0 and c1 by g mod 3
    if challenges:
        for g in range(len(E)):
            allowed = [[], [0], [0, 1]][g % 3]
            E[g] = _restrict_challenges(E[g], allowed, T)
            gate_chal.append(allowed)
        if 1 not in _challenges_of(E) and len(E) > 2:
            E[2] = E[2] + hc.challenge(1) * hc.challenge(0)
        if 0 not in _challenges_of(E[1:2]) and len(E) > 1:
            E[1] = E[1] + hc.challenge(0)
    lk_chal = [0] if challenges else []
    TL = _Trees(rng, n, lk_chal)
    TL.unb_rots = T.unb_rots

    tab_cols = 0

    def table_expr(adv):
        """a compound table expression over fixed table columns (one of them may be advice)"""
        nonlocal tab_cols
        a, b = NFIX_DATA + tab_cols, NFIX_DATA + tab_cols + 1
        tab_cols += 2
        first = hc.advice(1, 1) if adv else hc.fixed(a)
        e = TL.const() * first + hc.fixed(b, int(rng.integers(-1, 2)))
        if rng.random() < 0.5 and not challenges:   # (a challenge circuit's table holds the zero tuple)
            e = e - TL.const()
        return e

    lk = []      # (F list or None (plain), table expressions, tag constant or None)
    for li, m in enumerate(lookups):
        assert 1 <= m <= 3 and not (m == 3 and challenges), "a tagged lookup's table has no zero tuple"
        tag = hc.const(_value(rng)) if m == 3 else None
        tabs = [table_expr(advice_table and li == 0 and i == 0) for i in range(m - (tag is not None))]
        lk.append(([TL.tree(1, int(rng.integers(1, 8))) for _ in tabs], tabs, tag))
    if twin:
        assert lk, "twin needs a lookup"
        lk.append(([TL.tree(1, int(rng.integers(1, 8))) for _ in lk[0][1]], lk[0][1], lk[0][2]))
    if plain_lookup:
        lk.append((None, [hc.fixed(NFIX_DATA + tab_cols)], None))
        tab_cols += 1
    sh = (TL.tree(1, 5), TL.tree(2, 9)) if shuffle else None

    # ---- columns
    nout = len(E)
    out0 = NFREE + 1
    cell0 = out0 + nout
    ncell = sum(len(f[1]) for f in lk) + (1 if sh else 0)
    num_advice = cell0 + ncell
    q_gate0 = NFIX_DATA + tab_cols      # one selector per gate, then q_lookup, q_shuffle
    q_lk = q_gate0 + nout
    q_sh = q_lk + 1
    num_fixed = q_sh + 1
    gate_list = [hc.fixed(q_gate0 + g) * (E[g] - hc.advice(out0 + g)) for g in range(nout)]
    if bare:
        gate_list += [hc.const(0), hc.instance(1)]      # roots that are a bare constant / a bare query
    ql = hc.fixed(q_lk)

    def make_lookups(d_of):
        """d_of(table expression) -> the constant d_i; challenge circuits drop the (1 - q) d
        arm (d would depend on a challenge): their tables hold the zero tuple instead"""
        out, cell = [], cell0
        for F, tabs, tag in lk:
            ins = [tag] if tag is not None else []
            for i, t in enumerate(tabs):
                if F is None:
                    ins.append(hc.advice(cell))
                elif challenges:
                    ins.append(ql * (hc.advice(cell) + F[i]))
                else:
                    ins.append(ql * (hc.advice(cell) + F[i]) + (1 - ql) * hc.const(d_of(t)))
                cell += 1
            out.append((ins, ([tag] if tag is not None else []) + list(tabs)))
        return out

    shuffles_x = []
    if sh:
        qs = hc.fixed(q_sh)
        shuffles_x.append(([qs * (hc.advice(num_advice - 1) + sh[0])], [qs * sh[1]]))
    # the permutation: all three column types, more columns than chunk_len at degree <= 9
    perm = [(ADVICE, 0), (FIXED, 0), (INSTANCE, 0), (ADVICE, 1), (ADVICE, 2), (ADVICE, UNB)]
    perm += [(ADVICE, out0 + g) for g in range(nout)]
    adv_phase = [0] * num_advice
    if challenges:
        for g in range(nout):
            adv_phase[out0 + g] = len(gate_chal[g])
        for c in range(cell0, num_advice):
            adv_phase[c] = 1
    kw = dict(unblinded=[UNB], advice_phase=adv_phase if challenges else None,
              challenge_phase=[0, 1] if challenges else None)

    def build(fixed_vals, copies_, lookups_):
        return hc.Circuit(k, num_advice, num_fixed, 2, gate_list, perm, copies_, fixed_vals,
                          name=f"generated seed={seed} k={k}", lookups=lookups_, shuffles=shuffles_x, **kw)

    probe = build(np.zeros((num_fixed, n, 4), np.uint64), [], make_lookups(lambda t: 0))
    u = probe.usable_rows()
    lo = max(_max_advice_rot(roots(probe)), 1)
    hi = u - lo
    assert hi - lo >= 8, "too few active rows"
    active = list(range(lo, hi))

    # ---- fixed columns: data and tables (random on every row), the selectors
    fixed_cols = [[_value(rng) for _ in range(n)] for _ in range(NFIX_DATA + tab_cols)]
    for _ in range(nout + 2):
        fixed_cols.append([1 if lo <= r < hi else 0 for r in range(n)])
    # d is the table's tuple on row lo.  It is circuit data, so the one advice cell a table
    # expression reads there (column 1, row lo + 1) holds a circuit-seeded value in every witness.
    adv_tab_val = 0 if challenges else _value(rng)
    if challenges:   # the zero tuple on row lo: zero what the table expressions read there
        for F, tabs, tag in lk:
            for t in tabs:
                for x in walk(t):
                    if x.op == OP_QUERY and x.a == FIXED:
                        fixed_cols[x.b][(lo + x.c) % n] = 0

    def d_of(t):
        def q(ty, c, rot):
            if ty == FIXED:
                return fixed_cols[c][(lo + rot) % n]
            assert (ty, c, rot) == (ADVICE, 1, 1)
            return adv_tab_val
        return t.evaluate(lambda v: v, q)

    # ---- copies between cells of the free columns, from a fixed cell and from an instance cell;
    # no cell takes part in two of them
    crng = np.random.default_rng([int(seed), 0xC0])
    copy_list, seen = [], {(ADVICE, 1, lo + 1)}
    for _ in range(copies):
        a, b = int(crng.integers(NFREE)), int(crng.integers(NFREE))
        ra, rb, rc = (int(crng.integers(u)) for _ in range(3))
        for c in ((ADVICE, a, ra, ADVICE, b, rb), (FIXED, 0, rc, ADVICE, UNB, rc),
                  (INSTANCE, 0, rb, ADVICE, (a + 1) % NFREE, rc)):
            src, dst = c[:3], c[3:]
            if src != dst and src not in seen and dst not in seen:
                seen |= {src, dst}
                copy_list.append(c)

    circ = build(np.stack([hc.ints_to_mont(c) for c in fixed_cols]), copy_list, make_lookups(d_of))
    assert circ.usable_rows() == u and circ.degree() == probe.degree()
    # where the solved cells are (a test corrupts one): gate g's output column out0 + g on
    # `active`; last_phase: the gates whose column no challenge depends on (a changed cell there
    # leaves the challenges, and so every other solved column, as they were)
    circ.gen = dict(out0=out0, nout=nout, cell0=cell0, active=(lo, hi), u=u,
                    last_phase=[g for g in range(nout) if adv_phase[out0 + g] == max(adv_phase)])

    # ---- the witness
    wseed = seed if witness_seed is None else witness_seed
    wrng = np.random.default_rng([int(wseed), 0x717])
    free = [[_value(wrng) if r < u else 0 for r in range(n)] for _ in range(NFREE + 1)]
    free[1][lo + 1] = adv_tab_val
    inst0 = [_value(wrng) if r < u else 0 for r in range(n)]
    for lt, li, lr, rt, ri, rr in copy_list:
        src = fixed_cols[li][lr] if lt == FIXED else inst0[lr] if lt == INSTANCE else free[li][lr]
        free[ri][rr] = src
    filler = [[_value(wrng) if r < u else 0 for r in range(n)] for _ in range(nout + ncell)]
    pick = [[int(wrng.integers(lo, hi)) for _ in range(n)] for _ in lk]
    pick_plain = [int(wrng.integers(0, u)) for _ in range(n)]
    pi = [active[int(i)] for i in wrng.permutation(len(active))]

    def solve(chs):
        """every advice column (canonical ints) for the challenge values chs"""
        chs = list(chs) + [0] * (2 - len(chs))
        adv = [c[:] for c in free] + [c[:] for c in filler]
        cols = {ADVICE: adv, FIXED: fixed_cols, INSTANCE: [inst0, [0] * n]}

        def at(e, row):
            return e.evaluate(lambda v: v, lambda t, i, rot: cols[t][i][(row + rot) % n], challenge=lambda i: chs[i])

        for g in range(nout):
            col = adv[out0 + g]
            for row in active:
                col[row] = at(E[g], row)
        ci = cell0
        for j, (F, tabs, tag) in enumerate(lk):
            for i, t in enumerate(tabs):
                col = adv[ci]
                if F is None:
                    for row in range(u):
                        col[row] = at(t, pick_plain[row])
                else:
                    for row in active:
                        col[row] = (at(t, pick[j][row]) - at(F[i], row)) % R
                ci += 1
        if sh:
            col = adv[ci]
            for idx, row in enumerate(active):
                col[row] = (at(sh[1], pi[idx]) - at(sh[0], row)) % R
        return adv

    instance = np.stack([hc.ints_to_mont(inst0), np.zeros((n, 4), np.uint64)])
    lens = [u, 0]
    if not challenges:
        wit = hc.Witness(np.stack([hc.ints_to_mont(c) for c in solve([])]), instance, lens)
        return circ, wit, None

    wit = hc.Witness(np.zeros((num_advice, n, 4), np.uint64), instance, lens)

    def fill(phase, chs):
        adv = solve(chs)
        return {c: hc.ints_to_mont(adv[c]) for c in range(num_advice) if adv_phase[c] == phase}

    def full(chs):
        return hc.Witness(np.stack([hc.ints_to_mont(c) for c in solve(chs)]), instance, lens)

    fill.full = full
    return circ, wit, fill


def _restrict_challenges(e, allowed, T, memo=None):
    """the tree with every challenge leaf outside `allowed` replaced (by an allowed one, or by
    a constant); a sub-expression object used twice stays one object"""
    memo = {} if memo is None else memo
    if id(e) in memo:
        return memo[id(e)]
    out = e
    if e.op == OP_CHALLENGE and e.a not in allowed:
        out = hc.challenge(allowed[e.a % len(allowed)]) if allowed else hc.const(_uniform(T.rng))
    elif e.op == OP_NEG:
        out = hc.Expr(OP_NEG, _restrict_challenges(e.a, allowed, T, memo))
    elif e.op in (OP_SUM, OP_PROD):
        out = hc.Expr(e.op, _restrict_challenges(e.a, allowed, T, memo), _restrict_challenges(e.b, allowed, T, memo))
    memo[id(e)] = out
    return out


# ----------------------------------------------------------------------------- the pinned cases
# Every case is proved by the oracle, verified and checked on the CPU
# (tests/test_generated_circuits_cpu.py, which also asserts what the list covers) before the
# device is compared with it.  A seed the oracle refuses is replaced here by hand.
_FULL = dict(lookups=(1, 2, 3), twin=True, advice_table=True, plain_lookup=True, shuffle=True)
CASES = [
    # degree 3: extended domain 2n, one permutation column per set
    dict(seed=101, k=6, degree=3, special="all"),
    dict(seed=102, k=7, degree=3),
    dict(seed=103, k=6, degree=3, gates=4),
    dict(seed=104, k=7, degree=3, special=("right", "left")),
    dict(seed=105, k=6, degree=3, gates=1, special=("balanced", "bare")),
    # degree 4..5: extended domain 4n; lookups and shuffles from degree 5 on
    dict(seed=201, k=6, degree=4),
    dict(seed=202, k=7, degree=4, special="all"),
    dict(seed=203, k=7, degree=5, special="all", **_FULL),
    dict(seed=204, k=6, degree=5, lookups=(1,)),
    dict(seed=205, k=6, degree=5, lookups=(2,), twin=True),
    dict(seed=206, k=7, degree=5, lookups=(3, 1), advice_table=False, shuffle=True),
    dict(seed=207, k=7, degree=5, lookups=(1, 1), advice_table=True),
    dict(seed=208, k=6, degree=5, plain_lookup=True, shuffle=True),
    dict(seed=209, k=7, degree=5, gates=6, nodes=(100, 120)),
    dict(seed=210, k=7, degree=5, lookups=(2, 3), twin=True, special=("many_rot",)),
    # degree 6..9: extended domain 8n
    dict(seed=301, k=6, degree=6),
    dict(seed=302, k=7, degree=6, special="all", **_FULL),
    dict(seed=303, k=6, degree=7, lookups=(1, 2)),
    dict(seed=304, k=7, degree=7, shuffle=True),
    dict(seed=305, k=6, degree=8, special=("shared", "negneg", "sub_nbrs")),
    dict(seed=306, k=7, degree=8, lookups=(3,), twin=True),
    dict(seed=307, k=6, degree=9, special="all"),
    dict(seed=308, k=7, degree=9, gates=4, lookups=(1,), advice_table=True),
    dict(seed=309, k=6, degree=9, gates=1, special=("left", "right")),
    # degree 10..17: extended domain 16n
    dict(seed=401, k=6, degree=10),
    dict(seed=402, k=6, degree=12, special=("balanced", "many_rot")),
    dict(seed=403, k=6, degree=13, lookups=(1,)),
    dict(seed=404, k=6, degree=15, gates=1, special=()),
    dict(seed=405, k=6, degree=17, gates=1),
    dict(seed=406, k=6, degree=17, gates=1, special=("shared",), shuffle=True),
    # challenges in gates and lookups, solved columns over three phases
    dict(seed=501, k=6, degree=5, challenges=True, lookups=(1,)),
    dict(seed=502, k=7, degree=5, challenges=True, lookups=(1, 2), twin=True, shuffle=True, special="all"),
    dict(seed=503, k=6, degree=3, challenges=True),
    dict(seed=504, k=7, degree=6, challenges=True, lookups=(2,), advice_table=True, plain_lookup=True),
    dict(seed=505, k=6, degree=9, challenges=True, shuffle=True),
    dict(seed=506, k=6, degree=11, challenges=True, gates=1),
    # more of the common shape, and one larger domain
    dict(seed=601, k=7, degree=5, **_FULL),
    dict(seed=602, k=6, degree=5, **_FULL),
    dict(seed=603, k=7, degree=7, **_FULL),
    dict(seed=604, k=10, degree=5, special=("many_rot", "balanced"), lookups=(1, 2), twin=True, shuffle=True),
]


# Circuits whose h(X) splits unevenly (degree - 1 no power of two) at a multi-pass size: the
# extended domain is 2^13 .. 2^16, so extended_to_coeff ends in the truncated last pass and keeps
# 3/4, 6/8, 5/8, 7/8, 11/16 and 15/16 of it, where every case above with such a degree sits at
# k <= 7 and is served by the one-block kernel.  Pinned valid by tests/test_generated_circuits_cpu.py,
# compared on the device by tests/test_gpu_generated_large.py.
LARGE_CASES = [
    dict(seed=701, k=11, degree=4),
    dict(seed=702, k=11, degree=7, lookups=(1,), shuffle=True),
    dict(seed=703, k=12, degree=6),
    dict(seed=704, k=11, degree=8),
    dict(seed=705, k=11, degree=12, gates=1),
    dict(seed=706, k=12, degree=16, gates=1),
]


def case_id(case):
    return "-".join(f"{k[0]}{v}" if k in ("seed", "k", "degree") else k for k, v in case.items()
                    if k in ("seed", "k", "degree") or (k == "challenges" and v))


# ----------------------------------------------------------------------------- refused proofs
def zero_table_lookup(k=6, zero=True):
    """[q advice(a)] in [fixed(t)] with the gate q b (b - 1).  zero: t and a identically zero --
    the lookup declares degree 5, h(X) then has a lower one, its top piece is the zero
    polynomial and its commitment the point at infinity, which the reference refuses to write.
    zero=False: the sibling with t = 0, 1, 2, .. and a drawn from it."""
    n = 1 << k
    u = n - 6
    rng = np.random.default_rng(k)
    q = hc.fixed(0)
    t = [0 if zero or r >= u else r for r in range(n)]
    a = [0 if zero or r >= u else int(rng.integers(u)) for r in range(n)]
    b = [int(rng.integers(2)) if r < u else 0 for r in range(n)]
    fixed_vals = np.stack([hc.ints_to_mont([1 if r < u else 0 for r in range(n)]), hc.ints_to_mont(t)])
    circ = hc.Circuit(k, 2, 2, 0, [q * hc.advice(1) * (hc.advice(1) - 1)], [(ADVICE, 0)], [], fixed_vals,
                      name=f"zero table k={k}" if zero else f"range table k={k}",
                      lookups=[([q * hc.advice(0)], [hc.fixed(1)])])
    assert circ.usable_rows() == u
    return circ, hc.Witness(np.stack([hc.ints_to_mont(a), hc.ints_to_mont(b)]), np.zeros((0, n, 4), np.uint64), [])


def unblinded_boolean(k=6, zero=True):
    """an unblinded advice column z under the gate q z (z - 1), next to a blinded column with a
    copy.  zero: z identically zero -- its commitment is the point at infinity; else random bits
    (the same circuit: one key proves both)."""
    n = 1 << k
    u = n - 6
    rng = np.random.default_rng(k + 100)
    q = hc.fixed(0)
    z = [0 if zero or r >= u else int(rng.integers(2)) for r in range(n)]
    a = [_value(rng) if r < u else 0 for r in range(n)]
    a[5] = a[2]
    gates = [q * hc.advice(0) * (hc.advice(0) - 1)]
    circ = hc.Circuit(k, 2, 1, 0, gates, [(ADVICE, 1)], [(ADVICE, 1, 2, ADVICE, 1, 5)],
                      hc.ints_to_mont([1 if r < u else 0 for r in range(n)])[None], unblinded=[0],
                      name=f"unblinded boolean k={k}")
    assert circ.usable_rows() == u
    return circ, hc.Witness(np.stack([hc.ints_to_mont(z), hc.ints_to_mont(a)]), np.zeros((0, n, 4), np.uint64), [])
