"""Python restatement of the KZG multi-open argument on its own, the yardstick of
h2g_multiopen_prove / h2g_multiopen_verify (TEST INFRASTRUCTURE ONLY).

Restated reference code (paths relative to the reference root):
  ProverSHPLONK::create_proof      halo2_backend/src/poly/kzg/multiopen/shplonk/prover.rs:121-305
  VerifierSHPLONK::verify_proof    halo2_backend/src/poly/kzg/multiopen/shplonk/verifier.rs:45-140
  construct_intermediate_sets      halo2_backend/src/poly/kzg/multiopen/shplonk.rs:48-140
  ProverGWC::create_proof          halo2_backend/src/poly/kzg/multiopen/gwc/prover.rs:40-90, gwc.rs:25-50
  VerifierGWC::verify_proof        oracle/py/verifier.py _verify_gwc, reused as it is
  the round trip                   halo2_backend/src/poly/multiopen_test.rs:140-304

The params come from a known secret s (h2g_params_setup), and commit is a homomorphism, so a
commitment is [p(s)] G: every polynomial the provers build (h, the GWC witnesses, the
linearisation quotient) is followed through its value at s instead of its coefficients -- the
quotient N / Z at s is N(s) / Z(s).  No MSM, no polynomial division; s must not be one of the
opening points or challenges (probability ~ 2^-250).

Values are canonical Python ints; points are (x, y) or None; polynomials lists of ints.
"""
from bn254_ref import G1_GEN, R, eval_polynomial, fr_to_repr, g1_mul, g1_to_bytes
import verifier as V


class _Write:
    """TranscriptWrite over the oracle's read classes (transcript.rs:353-463): write_* absorbs
    what common_* does and appends the encoding"""

    def write_point(self, pt):
        self.common_point(pt)  # VerifyError for the identity, before anything is written
        self.out += g1_to_bytes(pt)

    def write_scalar(self, s):
        self.common_scalar(s)
        self.out += fr_to_repr(s % R)

    def finalize(self):
        return bytes(self.out)


def writer(kind):
    t = type("Write_" + kind, (_Write, V.TRANSCRIPTS[kind]), {})(b"")
    t.out = bytearray()
    return t


def reader(kind, proof):
    return V.TRANSCRIPTS[kind](proof)


def commit(poly, s):
    """[p(s)] G; None for the identity"""
    return g1_mul(G1_GEN, eval_polynomial(poly, s))


def _inv(a):
    return pow(a % R, -1, R)


def _rotation_sets(queries):
    """construct_intermediate_sets (shplonk.rs:48-140) over (key, point) pairs: the keys in
    first-appearance order with their point sets; keys with equal sets share a rotation set
    (sets in first-appearance order, points sorted as the BTreeSet iterates)"""
    order, pts_of = [], {}
    for key, pt in queries:
        if key not in pts_of:
            order.append(key)
            pts_of[key] = set()
        pts_of[key].add(pt)
    sets = []
    for key in order:
        pts = sorted(pts_of[key])
        for rs in sets:
            if rs[0] == pts:
                rs[1].append(key)
                break
        else:
            sets.append((pts, [key]))
    return sets, sorted({pt for _, pt in queries})


def prove_shplonk(T, s, polys, queries):
    """queries: [(poly index, point)] in the argument's order; writes h and h' into T"""
    y = T.squeeze()
    sets, super_pts = _rotation_sets(queries)
    at_s = {i: eval_polynomial(polys[i], s) for i, _ in queries}
    low = {}  # (poly, set index) -> r(X), the interpolation through the evaluations
    for si, (pts, ids) in enumerate(sets):
        for i in ids:
            low[(i, si)] = V.lagrange_interpolate(pts, [eval_polynomial(polys[i], p) for p in pts])
    v = T.squeeze()
    h_s, vpow = 0, 1
    for si, (pts, ids) in enumerate(sets):
        n_s, ypow = 0, 1
        for i in ids:  # N(X) = sum_j y^j (P_j(X) - R_j(X))
            n_s = (n_s + ypow * (at_s[i] - eval_polynomial(low[(i, si)], s))) % R
            ypow = ypow * y % R
        h_s = (h_s + vpow * n_s % R * _inv(V.vanishing_poly_eval(pts, s))) % R
        vpow = vpow * v % R
    T.write_point(g1_mul(G1_GEN, h_s))
    u = T.squeeze()
    l_s, vpow, z_diffs = 0, 1, []
    for si, (pts, ids) in enumerate(sets):
        z_i = V.vanishing_poly_eval([p for p in super_pts if p not in pts], u)
        inner, ypow = 0, 1
        for i in ids:  # L(X) = sum_j y^j (P_j(X) - R_j(u))
            inner = (inner + ypow * (at_s[i] - eval_polynomial(low[(i, si)], u))) % R
            ypow = ypow * y % R
        l_s = (l_s + vpow * inner % R * z_i) % R
        z_diffs.append(z_i)
        vpow = vpow * v % R
    l_s = (l_s - V.vanishing_poly_eval(super_pts, u) * h_s) % R
    T.write_point(g1_mul(G1_GEN, l_s * _inv(s - u) % R * _inv(z_diffs[0]) % R))


def prove_gwc(T, s, polys, queries):
    v = T.squeeze()
    groups = []  # [(point, [poly index])], first appearance; a repeated pair stays twice
    for i, pt in queries:
        for g in groups:
            if g[0] == pt:
                g[1].append(i)
                break
        else:
            groups.append((pt, [i]))
    for z, ids in groups:
        pb, eb, vpow = 0, 0, 1
        for i in ids:
            pb = (pb + vpow * eval_polynomial(polys[i], s)) % R
            eb = (eb + vpow * eval_polynomial(polys[i], z)) % R
            vpow = vpow * v % R
        T.write_point(g1_mul(G1_GEN, (pb - eb) * _inv(s - z) % R))  # kate_division at s


def prove(scheme, T, s, polys, queries):
    return (prove_gwc if scheme == "gwc" else prove_shplonk)(T, s, polys, queries)


def verify_shplonk(T, s, commitments, queries, proof):
    """queries: [(commitment index, point, eval)]; returns (accepted, left, right).
    Raises VerifyError as the oracle's transcript does."""
    sets, super_pts = _rotation_sets([(c, pt) for c, pt, _ in queries])
    evals = {}
    for c, pt, ev in queries:
        evals.setdefault((c, pt), ev)  # get_eval: the first query of the pair (shplonk.rs:57-63)
    y = T.squeeze()
    v = T.squeeze()
    h1 = T.read_point()
    u = T.squeeze()
    h2 = T.read_point()
    if T.pos != len(proof):
        raise V.VerifyError("trailing proof bytes")
    outer = V.Msm()
    r_outer, vpow, z0, z0_diff_inv = 0, 1, 0, 0
    for si, (pts, ids) in enumerate(sets):
        z_diff = V.vanishing_poly_eval([p for p in super_pts if p not in pts], u)
        if si == 0:
            z0 = V.vanishing_poly_eval(pts, u)
            z0_diff_inv = _inv(z_diff)
            z_diff = 1
        else:
            z_diff = z_diff * z0_diff_inv % R
        r_inner, ypow = 0, 1
        for c in ids:
            r_x = V.lagrange_interpolate(pts, [evals[(c, p)] for p in pts])
            r_inner = (r_inner + ypow * eval_polynomial(r_x, u)) % R
            outer.add(ypow * vpow % R * z_diff, commitments[c])
            ypow = ypow * y % R
        r_outer = (r_outer + vpow * r_inner % R * z_diff) % R
        vpow = vpow * v % R
    outer.add(-r_outer, G1_GEN)
    outer.add(-z0, h1)
    outer.add(u, h2)
    right = outer.eval()
    return g1_mul(h2, s) == right, h2, right


def verify(scheme, T, s, commitments, queries, proof):
    """True / False; VerifyError for a malformed argument"""
    if scheme == "gwc":
        return V._verify_gwc(T, [(c, commitments[c], pt, ev) for c, pt, ev in queries], proof, s)
    return verify_shplonk(T, s, commitments, queries, proof)[0]


# ----------------------------------------------------------------------------- the reference's round trip
def round_trip_polys(k):
    """multiopen_test.rs:240-255: a_i = 10 + i, b_i = c_i = 100 + i"""
    n = 1 << k
    return [[10 + i for i in range(n)], [100 + i for i in range(n)], [100 + i for i in range(n)]]


def round_trip_prove(scheme, kind, k, s):
    """create_proof of multiopen_test.rs:227-304 -> the proof bytes"""
    polys = round_trip_polys(k)
    T = writer(kind)
    for p in polys:
        T.write_point(commit(p, s))
    x = T.squeeze()
    y = T.squeeze()
    for p, pt in zip(polys, (x, x, y)):
        T.write_scalar(eval_polynomial(p, pt))
    queries = [(0, x), (1, x), (2, y)]
    prove(scheme, T, s, polys, queries)
    return T.finalize()


def round_trip_open(kind, proof):
    """verify's head (multiopen_test.rs:180-205): the transcript after the evaluations, the
    commitments, and the valid and the invalid queries (b's evaluation replaced by a's)"""
    T = reader(kind, proof)
    cms = [T.read_point() for _ in range(3)]
    x = T.squeeze()
    y = T.squeeze()
    avx, bvx, cvy = T.read_scalar(), T.read_scalar(), T.read_scalar()
    return T, cms, [(0, x, avx), (1, x, bvx), (2, y, cvy)], [(0, x, avx), (1, x, avx), (2, y, cvy)]
