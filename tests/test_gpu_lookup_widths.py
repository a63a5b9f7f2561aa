"""The lookup sort's adaptive strategy (create_proof's permute_expression_pair, prover.cpp)
driven through every regime and transition, with proof bytes against the C restatement prover
after every step and the per-lookup sort hints read back through h2g_pk_lookup_sort_hints.

The rule, restated in `step` below from prover.cpp: a lookup whose hint is `used` keys both
columns on bits [max(used - 48, 0), +48) of the canonical values and sorts stably; hb is the
bit width of the OR of the values it keyed, tie says a gathered column came out unsorted; the
next hint is 0 when tie and hb == used, else hb; a hint of 0 (full sort) stays.  Lookups with
identical table expressions key the table once, for the first of them, while no hint is 0.

The lookups are [q advice(a)] in [advice(t)], so both sides change between witnesses of one key.
k = 7 is one radix tile; k = 13 has u > 4096: several tiles and the cross-tile scan, also
inside the full sort."""
import numpy as np
import pytest

import _oracle as O
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

R = hc.R_MOD
_PARAMS = {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for _, _, p in _PARAMS.values():
        p.close()
    _PARAMS.clear()


def _params(k):
    if k not in _PARAMS:
        _, g, gl = O.srs(k)
        _PARAMS[k] = (g, gl, h2g.Params(k, g, gl))
    return _PARAMS[k]


# ----------------------------------------------------------------------------- circuit and witnesses
def width_circuit(k, lookups):
    """lookups: [(input columns, table columns)] over advice columns 1..; advice 0 is a
    boolean column b with the gate q b (b - 1) and a few copies.  q = 1 on every usable row."""
    n = 1 << k
    na = 1 + max(c for a, t in lookups for c in a + t)
    q = hc.fixed(0)
    lks = [([q * hc.advice(c) for c in a], [hc.advice(c) for c in t]) for a, t in lookups]
    gates = [q * hc.advice(0) * (hc.advice(0) - 1)]
    u = n - 6
    bits = [int(x) for x in np.random.default_rng(k).integers(0, 2, size=n)]
    bits[0], bits[1] = 1, 0
    copies = [(hc.ADVICE, 0, 0, hc.ADVICE, 0, r) for r in range(2, 40) if bits[r] == 1][:5]
    fixed = hc.ints_to_mont([1 if r < u else 0 for r in range(n)])[None]
    circ = hc.Circuit(k, na, 1, 0, gates, [(hc.ADVICE, 0)], copies, fixed, name=f"lookup widths k={k}",
                      lookups=lks)
    assert circ.usable_rows() == u and circ.degree() == 5
    circ.bits = bits
    return circ


def witness(circ, columns):
    """columns: {advice column: u canonical values}"""
    n, u = circ.n, circ.usable_rows()
    adv = np.zeros((circ.num_advice, n, 4), np.uint64)
    adv[0] = hc.ints_to_mont([b if r < u else 0 for r, b in enumerate(circ.bits)])
    for c, vals in columns.items():
        assert len(vals) == u and all(0 <= v < R for v in vals)
        adv[c, :u] = O.fr_from_canonical(np.asarray(
            [[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64))
    return hc.Witness(adv, np.zeros((0, n, 4), np.uint64), [])


def _uniform(rng, m):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(m)]


def _below(rng, bits, m):
    return [int.from_bytes(rng.bytes(32), "little") >> (256 - bits) for _ in range(m)]


def family(name, u, seed=0):
    """-> (table values, input values), u canonical ints each; the input is drawn from the table"""
    rng = np.random.default_rng([seed, sum(name.encode())])
    draw = lambda t: [t[int(i)] for i in rng.integers(0, u, size=u)]  # noqa: E731
    if name == "below 2^8":
        t = _below(rng, 8, u)
    elif name == "top bit 47":
        t = [(1 << 47) + v for v in _below(rng, 47, u)]
    elif name == "top bit 48":
        t = [(1 << 48) + v for v in _below(rng, 48, u)]
    elif name == "64 bit":
        t = [(1 << 63) + v for v in _below(rng, 63, u)]
    elif name == "2^64 + small":
        t = [(1 << 64) + v for v in _below(rng, 16, u)]
    elif name == "2^100 + small":
        t = [(1 << 100) + v for v in _below(rng, 16, u)]
    elif name == "uniform":
        t = _uniform(rng, u)
    elif name == "r - 1 - small":
        t = [R - 1 - v for v in _below(rng, 16, u)]
    elif name == "one value":
        t = [(1 << 200) + 12345] * u
    elif name == "distinct, input a permutation":
        t = _uniform(rng, u)
        assert len(set(t)) == u
        return t, [t[int(i)] for i in rng.permutation(u)]
    elif name == "ascending":       # the window ties every row, yet both columns come out in order
        t = sorted((1 << 100) + v for v in _below(rng, 30, u))
        return t, list(t)
    elif name == "descending":
        t = sorted(((1 << 100) + v for v in _below(rng, 30, u)), reverse=True)
    else:
        raise ValueError(name)
    return t, draw(t)


# the hints after each of three proofs of one witness on a fresh key (64 before the first),
# written out from the rule
FAMILIES = {
    "below 2^8": [8, 8, 8],                    # width redo down (a tie at the wrong width), then value keys
    "top bit 47": [48, 48, 48],                # the widest value key
    "top bit 48": [49, 49, 49],                # the narrowest window: bits [1, 49)
    "64 bit": [64, 64, 64],                    # the first guess holds
    "2^64 + small": [65, 0, 0],                # width redo, tie at the right width, full sort
    "2^100 + small": [101, 0, 0],
    "uniform": [254, 254, 254],
    "r - 1 - small": [254, 0, 0],              # the top 48 bits tie
    "one value": [201, 201, 201],              # equal values are no tie
    "distinct, input a permutation": [254, 254, 254],
    "ascending": [101, 101, 101],              # every key ties; the stable sort keeps the order
    "descending": [101, 0, 0],
}


def _unsorted(vals, shift):
    order = sorted(range(len(vals)), key=lambda i: (vals[i] >> shift) & ((1 << 48) - 1))   # stable
    return any(vals[order[i + 1]] < vals[order[i]] for i in range(len(vals) - 1))


def step(hints, cols, trep):
    """the hints after one proof.  hints: per circuit x lookup, before; cols[j] = (input, table)
    canonical values of lookup j of this proof (len(cols) <= len(hints)); trep[l]: the first
    lookup with lookup l's table expressions.  -> (hints after, {what the proof went through})"""
    nl, nlt = len(trep), len(cols)
    share = all(h != 0 for h in hints[:nlt])
    shift = [max(h - 48, 0) for h in hints]
    out, went = list(hints), set()
    if any(trep[l] != l for l in range(nl)):
        went.add("shared table" if share else "sharing off")
    for j in range(nlt):
        used = hints[j]
        if used == 0:
            went.add("full sort from the start")
            continue
        src = (j // nl) * nl + trep[j % nl] if share else j
        a, t = cols[j]
        acc = 0
        for v in a + (t if src == j else []):
            acc |= v
        hb = max(acc.bit_length(), 1)
        tie = _unsorted(a, shift[j]) or _unsorted(t, shift[src])
        out[j] = 0 if tie and hb == used else hb
        went.add("value keys" if used <= 48 else "window")
        if hb > used:
            went.add("width redo")
        if tie and hb == used:
            went.add("tie redo")
        if not tie and hb <= used:
            went.add("value keys held" if used <= 48 else "window held")
    return out, went


def test_the_rule_gives_the_written_sequences():
    """(no device work) the table above follows from the rule, and the module's cases go
    through every regime and transition"""
    went = set()
    for k in (7, 13):
        u = (1 << k) - 6
        for name, want in FAMILIES.items():
            h, seq = [64], []
            for _ in range(3):
                h, w = step(h, [family(name, u)[::-1]], [0])
                went |= w
                seq.append(h[0])
            assert seq == want, (k, name, seq)
    assert went >= {"value keys", "window", "width redo", "tie redo", "full sort from the start", "value keys held",
                    "window held"}
    hints = {h for seq in FAMILIES.values() for h in seq}
    assert any(0 < h <= 48 for h in hints) and any(h > 48 for h in hints) and 0 in hints


class Key:
    """a device key and the oracle's for one circuit, with the hints followed by the rule"""

    def __init__(self, circ, trep=None):
        self.circ = circ
        self.g, self.gl, params = _params(circ.k)
        self.pk = h2g.ProvingKey(params, circ)
        self.kg = None
        self.nl = len(circ.lookups)
        self.trep = trep or list(range(self.nl))
        self.want = [64] * self.nl
        self.went = set()
        assert self.pk.lookup_sort_hints() == self.want

    def prove(self, wits, cols):
        """one proof of the witnesses `wits` (one per circuit); cols: per circuit x lookup
        (input values, table values), None where the values are not known to the test"""
        if self.kg is None:
            self.kg = O.Keygen(self.circ, wits[0], self.g, self.gl)
        if len(wits) == 1:
            want = O.create_proof(self.circ, wits[0], self.g, self.gl, keygen=self.kg)
            got = self.pk.create_proof(wits[0])
        else:
            want = O.create_proof(self.circ, wits[0], self.g, self.gl, keygen=self.kg, wits=wits)
            got = self.pk.create_proof_multi(wits)
        assert got == want
        hints = self.pk.lookup_sort_hints()
        if cols is not None:
            self.want += [64] * (len(cols) - len(self.want))
            self.want, went = step(self.want, cols, self.trep)
            self.went |= went
            assert hints == self.want
        return hints

    def close(self):
        if self.kg:
            self.kg.close()
        self.pk.close()


def _single(k):
    circ = width_circuit(k, [((1,), (2,))])
    u = circ.usable_rows()

    def wit(name, seed=0):
        t, a = family(name, u, seed)
        return witness(circ, {1: a, 2: t}), [(a, t)]

    return circ, wit


@pytest.mark.parametrize("k,name", [(k, f) for k in (7, 13) for f in FAMILIES])
def test_family_three_proofs(k, name):
    circ, wit = _single(k)
    key = Key(circ)
    w, cols = wit(name)
    seq = [key.prove([w], cols)[0] for _ in range(3)]
    assert seq == FAMILIES[name]
    key.close()


def test_sequences_on_one_key():
    """grow, shrink, tie, the full sort that sticks; and a window that starts tying"""
    circ, wit = _single(7)
    key = Key(circ)
    seq = []
    for i, name in enumerate(["below 2^8", "uniform", "below 2^8"] + ["2^100 + small"] * 3 + ["below 2^8", "uniform"]):
        w, cols = wit(name, seed=i)
        seq.append(key.prove([w], cols)[0])
    assert seq == [8, 254, 8, 101, 0, 0, 0, 0]
    assert key.went >= {"value keys", "window", "width redo", "tie redo", "full sort from the start"}
    key.close()
    key = Key(circ)
    seq = []
    for i, name in enumerate(["uniform"] + ["r - 1 - small"] * 3):
        w, cols = wit(name, seed=i)
        seq.append(key.prove([w], cols)[0])
    assert seq == [254, 0, 0, 0]
    key.close()


def _shared(k, first_input_sorted, third):
    """lookups 0 and 1 over one table expression, lookup 2 over another.  The shared table
    holds uniform and 2^100 + small values (these ascending down the column, so that the
    table's own window never ties out of order); lookup 0 draws from the uniform part, lookup
    1 only from the other: its own width is 101 while the table's is 254."""
    circ = width_circuit(k, [((1,), (4,)), ((2,), (4,)), ((3,), (5,))])
    u = circ.usable_rows()
    rng = np.random.default_rng(k)
    uni, packed = family("uniform", u)[0][: u // 2], sorted(family("2^100 + small", u)[0][: u - u // 2])
    t0 = [uni[i // 2] if i % 2 == 0 else packed[i // 2] for i in range(u)]
    a0 = [uni[int(i)] for i in rng.integers(0, len(uni), size=u)]
    a1 = [packed[int(i)] for i in rng.integers(0, len(packed), size=u)]
    if first_input_sorted:
        a1.sort()
    t1, a2 = family(third, u, seed=1)
    cols = [(a0, t0), (a1, t0), (a2, t1)]
    return circ, witness(circ, {1: a0, 2: a1, 3: a2, 4: t0, 5: t1}), cols


@pytest.mark.parametrize("k", [7, 13])
def test_shared_tables_until_one_lookup_sorts_in_full(k):
    """lookup 1's window ties its input: from the third proof on it sorts in full and the
    lookups stop sharing the table, lookups 0 and 2 still keyed on their windows"""
    circ, w, cols = _shared(k, False, "uniform")
    u = circ.usable_rows()
    key = Key(circ, trep=[0, 0, 2])
    assert key.prove([w], cols) == [254, 101, 254]   # lookup 1's OR saw its input only: the table was keyed for lookup 0
    assert key.prove([w], cols) == [254, 0, 254]
    assert key.went >= {"shared table", "tie redo"} and "sharing off" not in key.went
    for _ in range(2):                               # every lookup sorts its own copy of the table
        assert key.prove([w], cols) == [254, 0, 254]
    assert key.went >= {"sharing off", "full sort from the start", "window held"}
    small = {c: family("below 2^8", u, seed=c) for c in (4, 5)}
    ws = witness(circ, {1: small[4][1], 2: small[4][1][::-1], 3: small[5][1], 4: small[4][0], 5: small[5][0]})
    cs = [(small[4][1], small[4][0]), (small[4][1][::-1], small[4][0]), (small[5][1], small[5][0])]
    assert key.prove([ws], cs) == [8, 0, 8]          # the full sort sticks
    assert key.prove([w], cols) == [254, 0, 254]
    key.close()


def test_shared_tables_width_learnt_without_the_table():
    """lookup 2 is the one that ties; lookup 1, whose hint (101) never saw the shared table
    (254), then keys its own copy of it, finds it too wide and redoes"""
    circ, w, cols = _shared(7, True, "r - 1 - small")
    key = Key(circ, trep=[0, 0, 2])
    seq = [key.prove([w], cols) for _ in range(4)]
    assert seq == [[254, 101, 254], [254, 101, 0], [254, 254, 0], [254, 254, 0]]
    assert key.went >= {"shared table", "sharing off", "width redo", "window held", "full sort from the start"}
    key.close()


def test_several_circuits_in_one_proof():
    circ, wit = _single(7)
    key = Key(circ)
    parts = [wit("below 2^8"), wit("2^100 + small"), wit("uniform")]
    wits, cols = [p[0] for p in parts], [p[1][0] for p in parts]
    seq = [key.prove(wits, cols) for _ in range(3)]
    assert seq == [[8, 101, 254], [8, 0, 254], [8, 0, 254]]
    w, c = wit("below 2^8", seed=5)
    assert key.prove([w], c) == [8, 0, 254]     # one circuit: the other circuits' hints wait
    key.close()


def test_check_witness_leaves_the_hints_alone():
    circ, wit = _single(7)
    key = Key(circ)
    w, cols = wit("2^100 + small")
    key.prove([w], cols)
    before = key.pk.lookup_sort_hints()
    assert before == [101]
    other, _ = wit("below 2^8")
    assert key.pk.check_witness(other) == (0, [])
    assert key.pk.check_witness(w) == (0, [])
    assert key.pk.lookup_sort_hints() == before
    assert key.prove([w], cols) == [0]          # as without the checks: the tie at the right width
    key.close()


@pytest.mark.parametrize("tuples", ["all equal", "all distinct"])
def test_multi_column_lookup(tuples):
    """theta-compressed tuples (their values are the transcript's to know): one run over the
    whole permuted column, and u runs of one row, for the prefix-basis commitment"""
    circ = width_circuit(7, [((1, 2), (3, 4))])
    u = circ.usable_rows()
    rng = np.random.default_rng(3)
    if tuples == "all equal":
        x, y = 2**100 + 7, R - 5
        cols = {1: [x] * u, 2: [y] * u, 3: [x] * u, 4: [y] * u}
    else:
        t0, t1 = _uniform(rng, u), [2**100 + i for i in range(u)]
        p = [int(i) for i in rng.permutation(u)]
        cols = {1: [t0[i] for i in p], 2: [t1[i] for i in p], 3: t0, 4: t1}
    w = witness(circ, cols)
    key = Key(circ)
    for _ in range(3):
        hints = key.prove([w], None)
        assert len(hints) == 1 and (hints[0] == 0 or hints[0] > 200)
    key.close()
