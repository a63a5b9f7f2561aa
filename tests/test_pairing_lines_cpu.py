"""csrc/pairing.h's line tables (what the device pairing reads) against oracle/py/pairing_ref.py.

g2_line_table walks the Miller loop for one fixed G2 point and keeps each line's (lam, c);
miller_from_lines assembles f_{6u+2, Q}(P) from such a table in the order the device kernel
follows.  A host program (tests/native/pairing_lines_host.cpp, built from the library's own
header with hipcc for the host side only) does both, and every value is compared with the
Python restatement's Miller loop value for value.
"""
import os
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
ATE_LINES = 64 + bin(PR.ATE_LOOP & ((1 << 64) - 1)).count("1") + 2


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("pairinglines") / "pairing_lines_host"
    subprocess.run([HIPCC, "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC,
                    os.path.join(REPO, "tests", "native", "pairing_lines_host.cpp"), "-o", str(exe)],
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


def parse12(row):
    v = [int(x, 16) for x in row.split()]
    assert len(v) == 12
    return [(v[2 * i], v[2 * i + 1]) for i in range(6)]


def g1(pt):
    return [0, 0] if pt is None else [pt[0], pt[1]]


def g2(pt):
    return [0, 0, 0, 0] if pt is None else [pt[0][0], pt[0][1], pt[1][0], pt[1][1]]


S_VALUES = (0x1234567, 0x2B5C9A1E77D3F0468ACE13579BDF02468ACE1357)
G2_POINTS = [B.G2_GEN] + [B.g2_mul(B.G2_GEN, s) for s in S_VALUES]
G1_POINTS = [B.G1_GEN, B.g1_mul(B.G1_GEN, 0xC0FFEE1234567890ABCD), B.g1_mul(B.G1_GEN, B.R - 1), None]


def test_table_length_and_identity(run):
    rows = run([("lines", g2(q)) for q in G2_POINTS] + [("lines", g2(None))])
    assert rows == [str(ATE_LINES)] * len(G2_POINTS) + ["VERT"]


def test_miller_value_from_lines_matches_reference(run):
    cases = [(p, q) for q in G2_POINTS for p in G1_POINTS]
    rows = run([("miller", g1(p) + g2(q)) for p, q in cases])
    for r, (p, q) in zip(rows, cases):
        assert parse12(r) == [tuple(c) for c in PR.miller_loop(p, q)]
    # the identity gives 1
    assert parse12(rows[3]) == [tuple(c) for c in PR.ONE12]


def test_miller_loop_unchanged_by_the_split(run):
    cases = [(G1_POINTS[1], G2_POINTS[1]), (G1_POINTS[2], G2_POINTS[2])]
    rows = run([(op, g1(p) + g2(q)) for p, q in cases for op in ("loop", "miller")])
    for i, (p, q) in enumerate(cases):
        assert rows[2 * i] == rows[2 * i + 1]
        assert parse12(rows[2 * i]) == [tuple(c) for c in PR.miller_loop(p, q)]
