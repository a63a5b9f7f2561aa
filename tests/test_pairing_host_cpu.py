"""csrc/pairing.h (the verifier's host pairing) against oracle/py/pairing_ref.py.

A host program (tests/native/pairing_host.cpp, built from the library's own header with
hipcc for the host side only) runs the Fq12 operations, the pairing and pairing_check on
values this test picks; every result is compared with the Python restatement value for
value: the same tower (Fq12 = Fq2[w] / (w^6 - xi), six Fq2 coefficients), the same affine
line functions, so the Miller loop's output and the final exponentiation agree exactly.
"""
import os
import random
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "yet-another-halo2-fork_amd", "csrc")
sys.path.insert(0, os.path.join(REPO, "oracle", "py"))
import bn254_ref as B  # noqa: E402
import pairing_ref as PR  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("pairinghost") / "pairing_host"
    subprocess.run([HIPCC, "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC,
                    os.path.join(REPO, "tests", "native", "pairing_host.cpp"), "-o", str(exe)],
                   check=True, cwd=str(exe.parent))

    def go(cmds):
        text = "\n".join(op + " " + " ".join(format(x, "x") for x in args) for op, args in cmds) + "\n"
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout
        rows = out.splitlines()
        assert len(rows) == len(cmds)
        for r in rows:
            assert not r.startswith("ERR"), r
        return rows
    return go


def flat12(a):
    return [v for c in a for v in c]


def parse12(row):
    v = [int(x, 16) for x in row.split()]
    assert len(v) == 12
    return [(v[2 * i], v[2 * i + 1]) for i in range(6)]


def g1(pt):
    return [0, 0] if pt is None else [pt[0], pt[1]]


def g2(pt):
    return [pt[0][0], pt[0][1], pt[1][0], pt[1][1]]


def rand12(rng):
    return [(rng.randrange(B.P), rng.randrange(B.P)) for _ in range(6)]


def test_fq12_mul_inverse_frobenius(run):
    rng = random.Random(1201)
    xs = [rand12(rng) for _ in range(6)]
    # sparse operands too: a line's shape, one coefficient, one
    xs.append([(rng.randrange(B.P), 0), (rng.randrange(B.P), rng.randrange(B.P)), (0, 0),
               (rng.randrange(B.P), rng.randrange(B.P)), (0, 0), (0, 0)])
    xs.append([(0, 0)] * 5 + [(rng.randrange(B.P), rng.randrange(B.P))])
    xs.append(list(PR.ONE12))
    cmds, want = [], []
    for i, a in enumerate(xs):
        b = xs[(i + 3) % len(xs)]
        cmds.append(("f12mul", flat12(a) + flat12(b)))
        want.append(PR.f12_mul(a, b))
        cmds.append(("f12frob", flat12(a)))
        want.append(PR.f12_pow(a, B.P))
    rows = run(cmds)
    for r, w in zip(rows, want):
        assert parse12(r) == [tuple(c) for c in w]
    inv = [parse12(r) for r in run([("f12inv", flat12(a)) for a in xs])]
    for a, ai in zip(xs, inv):
        assert PR.f12_is_one(PR.f12_mul(a, ai))


def test_pairing_matches_reference_limb_for_limb(run):
    cases = [(1, 1), (0x1234567890ABCDEF1234, 0xFEDCBA0987654321), (B.R - 1, 7)]
    pts = [(B.g1_mul(B.G1_GEN, a), B.g2_mul(B.G2_GEN, b)) for a, b in cases]
    rows = run([("pairing", g1(p) + g2(q)) for p, q in pts])
    for r, (p, q) in zip(rows, pts):
        assert parse12(r) == [tuple(c) for c in PR.pairing(p, q)]


def test_bilinearity_and_identity(run):
    a, b = 0x51A7F00D5EED, 0xC0FFEE1234567
    P, Q = B.G1_GEN, B.G2_GEN
    rows = run([("pairing", g1(B.g1_mul(P, a)) + g2(B.g2_mul(Q, b))),
                ("pairing", g1(B.g1_mul(P, a * b % B.R)) + g2(Q)),
                ("pairing", g1(P) + g2(B.g2_mul(Q, a * b % B.R))),
                ("pairing", g1(None) + g2(Q)),
                ("pairing", g1(P) + g2(Q))])
    assert rows[0] == rows[1] == rows[2]
    assert parse12(rows[3]) == [tuple(c) for c in PR.ONE12]
    e = parse12(rows[4])
    assert e != [tuple(c) for c in PR.ONE12]   # non-degenerate
    assert parse12(rows[0]) == [tuple(c) for c in PR.f12_pow(e, a * b % B.R)]


def test_pairing_check(run):
    a = 0x1F2E3D4C5B6A79880123456789
    P, Q = B.g1_mul(B.G1_GEN, 5), B.g2_mul(B.G2_GEN, 11)
    aP, aQ, nP = B.g1_mul(P, a), B.g2_mul(Q, a), B.g1_neg(P)
    rows = run([
        ("check", [2] + g1(aP) + g2(Q) + g1(nP) + g2(aQ)),                          # e(aP, Q) e(-P, aQ) = 1
        ("check", [2] + g1(B.g1_mul(P, a + 1)) + g2(Q) + g1(nP) + g2(aQ)),          # one scalar off by one
        ("check", [2] + g1(aP) + g2(Q) + g1(nP) + g2(B.g2_mul(Q, a - 1))),
        ("check", [2] + g1(None) + g2(Q) + g1(None) + g2(aQ)),                      # identities pair to one
        ("check", [3] + g1(aP) + g2(Q) + g1(nP) + g2(aQ) + g1(None) + g2(Q)),
        ("check", [1] + g1(P) + g2(Q)),
        ("check", [0]),
    ])
    assert rows == ["1", "0", "0", "1", "1", "0", "1"]
