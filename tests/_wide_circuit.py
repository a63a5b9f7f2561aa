"""Circuits whose column, lookup and permutation counts sit at the prover's per-launch
capacities (h2g.debug_limits): what tests/test_wide_circuits_cpu.py pins on the CPU and
tests/test_gpu_wide_circuits.py proves on the device.

wide_circuit lays its cells out directly, in the manner of width_circuit
(tests/test_gpu_lookup_widths.py).  Fixed column 0 is q = 1 on every usable row.  Of the A
advice columns the last two are derived: a_sum by the linear gate

    q (a_0 + 2 a_1 + ... + (A - 2) a_{A-3} - a_sum),

which queries every column but the last, and a_pad by the padding gate q (a_0^(d-1) - a_pad),
which sets the degree d.  Lookup l is [q a_(l mod m)] in [fixed t_l] over the first m free
columns; every table holds one common set of values (the inputs are drawn from it) and fillers
of its own, in an order of its own, so the tables differ while any input column fits any table.
shared_table: every lookup names the one table t_0.  Shuffle s is [q a_x] ~ [q a_y] over a pair
of the last free columns.  The permutation covers the first perm_cols free columns -- and, where
there are fewer, fixed columns of its own beyond them, so that the number of sets does not bind
the number of advice columns -- with a few copies between neighbouring advice columns."""
import numpy as np

import h2g_circuit as hc

R = hc.R_MOD
K = 7


def _rand(rng, m):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(m)]


def wide_circuit(k=K, advice=5, phases=None, lookups=0, shared_table=False, perm_cols=3, degree=None, shuffles=0,
                 seed=0):
    """-> (circuit, witness).  phases: advice columns per phase (default: all in phase 0);
    degree: the circuit's degree (default: what the arguments alone give, at least 3)."""
    n = 1 << k
    u = n - 6   # every advice column is queried at one rotation: 5 blinding factors
    A = advice
    free = A - 2
    s_col, p_col = A - 2, A - 1
    sh_cols = list(range(free - 2 * shuffles, free))
    m = min(lookups, free - 2 * shuffles)
    assert free >= 1 and perm_cols >= 1 and (lookups == 0 or m >= 1) and free - 2 * shuffles >= 0
    pa = min(perm_cols, free)   # the permutation's advice columns; beyond them it takes fixed columns of its own
    arg_degree = max(3, 5 if lookups else 0, 4 if shuffles else 0)
    degree = degree or arg_degree
    assert degree >= arg_degree
    q = hc.fixed(0)

    lin = hc.advice(0)
    for i in range(1, free):
        lin = lin + (i + 1) * hc.advice(i)
    gates = [q * (lin - hc.advice(s_col))]
    pw = hc.advice(0)
    for _ in range(degree - 2):
        pw = pw * hc.advice(0)
    gates.append(q * (pw - hc.advice(p_col)))

    ntab = 0 if not lookups else (1 if shared_table else lookups)
    tab = [hc.fixed(1 + (0 if shared_table else l)) for l in range(lookups)]
    lks = [([q * hc.advice(l % m)], [tab[l]]) for l in range(lookups)]
    shs = [([q * hc.advice(sh_cols[2 * s])], [q * hc.advice(sh_cols[2 * s + 1])]) for s in range(shuffles)]

    # ---- fixed columns
    common = [1000 + 3 * j for j in range(u // 2)]
    fixed = [[1 if r < u else 0 for r in range(n)]]
    for t in range(ntab):
        vals = common + [1000000 * (t + 1) + j for j in range(u - len(common))]
        rot = (7 * t) % u
        fixed.append(vals[rot:] + vals[:rot] + [0] * (n - u))
    rng = np.random.default_rng([k, A, lookups, shuffles, perm_cols])
    for _ in range(perm_cols - pa):
        fixed.append(_rand(rng, n))

    # ---- advice
    rng = np.random.default_rng([k, A, lookups, shuffles, seed])
    cols = [[0] * n for _ in range(A)]
    for c in range(free):
        if c < m:
            cols[c][:u] = [common[int(i)] for i in rng.integers(0, len(common), size=u)]
        else:
            cols[c][:u] = _rand(rng, u)
    copies = []
    for j in range(min(pa, 6)):
        x, y = j, (j + 1) % pa
        if x in sh_cols or y in sh_cols:
            continue
        if y < m <= x:   # a lookup column takes no foreign value
            x, y = y, x
        rx, ry = 3 + j, 20 + 2 * j
        cols[y][ry] = cols[x][rx]
        copies.append((hc.ADVICE, x, rx, hc.ADVICE, y, ry))
    for s in range(shuffles):
        x, y = sh_cols[2 * s], sh_cols[2 * s + 1]
        cols[y][:u] = [cols[x][int(i)] for i in rng.permutation(u)]
    for r in range(u):
        cols[s_col][r] = sum((i + 1) * cols[i][r] for i in range(free)) % R
        cols[p_col][r] = pow(cols[0][r], degree - 1, R)

    ph = list(phases) if phases else [A]
    assert sum(ph) == A
    advice_phase = [p for p, cnt in enumerate(ph) for _ in range(cnt)]
    perm = [(hc.ADVICE, c) for c in range(pa)] + [(hc.FIXED, 1 + ntab + j) for j in range(perm_cols - pa)]
    circ = hc.Circuit(k, A, len(fixed), 0, gates, perm, copies,
                      np.stack([hc.ints_to_mont(f) for f in fixed]), name=f"wide A={A} NL={lookups} P={perm_cols}",
                      lookups=lks, shuffles=shs, advice_phase=advice_phase if len(ph) > 1 else None)
    assert circ.usable_rows() == u and circ.degree() == degree
    wit = hc.Witness(np.stack([hc.ints_to_mont(c) for c in cols]), np.zeros((0, n, 4), np.uint64), [])
    return circ, wit


def counts(circ):
    """(advice per phase, NL, NS, P, nsets, degree)"""
    d = circ.degree()
    per_phase = [int((circ.advice_phase[:circ.num_advice] == p).sum()) for p in range(circ.max_phase + 1)]
    P = len(circ.perm_columns)
    return per_phase, len(circ.lookups), len(circ.shuffles), P, -(-P // (d - 2)), d


def shapes(lim):
    """{name: (wide_circuit arguments, the counts the case claims)} from the capacities `lim`
    (h2g.debug_limits()); today's values in the comments"""
    copy, ring, batch = lim["copy_cols"], lim["msm_ring"], lim["msm_batch"]
    comp, keys, perm, inv = lim["compress_batch"], lim["lookup_keys_batch"], lim["perm_cols"], lim["poly_inv_batch"]
    assert comp == keys and lim["prefix_diff"] == copy and ring == batch   # the shapes below lean on these
    out = {}

    def add(name, claim, **kw):
        assert name not in out
        out[name] = (kw, claim)

    # advice columns per copy launch: 15, 16, 17, 32, 33
    for a in (copy - 1, copy, copy + 1, 2 * copy, 2 * copy + 1):
        add(f"advice-{a}", dict(phase=[a], NL=0, NS=0, P=3, nsets=3, d=3), advice=a)
    # commitments per stage against the ring and the batch: 63, 64, 65, 129
    for a in (ring - 1, ring, ring + 1, 2 * ring + 1):
        add(f"advice-{a}", dict(phase=[a], NL=0, NS=0, P=3, nsets=3, d=3), advice=a)
    h = (ring + copy) // 2   # 40 + 40: each phase below the ring, the proof above it
    add(f"phases-{h}-{h}", dict(phase=[h, h], NL=0, NS=0, P=3, nsets=3, d=3), advice=2 * h, phases=(h, h))
    # lookups with distinct tables, two compress / key items each: 16, 17, 32, 33
    for nl in (comp // 2, comp // 2 + 1, comp, comp + 1):
        add(f"lookups-{nl}", dict(phase=[nl + 3], NL=nl, NS=0, P=3, nsets=1, d=5), advice=nl + 3, lookups=nl)
    nl = keys + 1   # one shared table: 33 inputs + 1 table = 34 key items
    add(f"lookups-{nl}-shared", dict(phase=[nl + 3], NL=nl, NS=0, P=3, nsets=1, d=5), advice=nl + 3, lookups=nl,
        shared_table=True)
    # permutation sets against the ring (degree 3: one column a set): 63, 64
    for p in (ring - 1, ring):
        add(f"perm-d3-{p}", dict(phase=[5], NL=0, NS=0, P=p, nsets=p, d=3), advice=5, perm_cols=p)
    # columns of one set against the launch capacity: 8, 9 in one set; 10 = 9 + 1; 17 = 8 + 8 + 1 in one
    d = perm + 3   # 11: sets of 9
    for p in (perm, perm + 1, perm + 2):
        add(f"perm-d{d}-{p}", dict(phase=[p + 2], NL=0, NS=0, P=p, nsets=-(-p // (d - 2)), d=d), advice=p + 2,
            perm_cols=p, degree=d)
    d = 2 * perm + 3   # 19: sets of 17
    add(f"perm-d{d}-{d - 2}", dict(phase=[d], NL=0, NS=0, P=d - 2, nsets=1, d=d), advice=d, perm_cols=d - 2, degree=d)
    # grand products per batched inversion: 1 set + lookups + 1 shuffle = 16, 17
    for nl in (inv - 2, inv - 1):
        add(f"products-{nl + 2}", dict(phase=[nl + 5], NL=nl, NS=1, P=3, nsets=1, d=5), advice=nl + 5, lookups=nl,
            shuffles=1)
    # copy launches and compress / key batches crossed in one circuit: 17 columns, 17 lookups
    a = copy + 1
    add(f"advice-{a}-lookups-{a}", dict(phase=[a], NL=a, NS=0, P=3, nsets=1, d=5), advice=a, lookups=a)
    return out
