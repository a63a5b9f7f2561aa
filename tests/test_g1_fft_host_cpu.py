"""The G1 group FFT of csrc/g1_fft.h (g_to_lagrange) run on the host.

tests/native/g1_fft_host.cpp compiles the kernels' own header for the host side only and runs
the whole transform through its H2G_HD index functions and butterfly, stage by stage, in the
order and mapping the kernels use (bit-reversal swaps, butterfly t of stage s with the
twiddle of its wave's first butterfly where the stage is wave-uniform, the n^-1 scaling).  It
is built twice -- plainly, and with the address and undefined-behaviour sanitisers -- and run
directly; every test runs against both.  Expected values: tests/_g1_fft_ref.py (a field FFT in
Python integers and one oracle g1_mul per output).

k = 1 .. 6 never reaches a wave-uniform stage (those need 2^(k-s) >= 64 butterflies per
twiddle, k >= 7), so k = 7 and 8 are run as well: stages 1 and 1..2 there read the twiddle
through the wave's first butterfly.
"""
import os
import subprocess

import numpy as np
import pytest

import _g1_fft_ref as G
import bn254_ref as B

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "yet-another-halo2-fork_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
R = B.R


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("g1fft_" + request.param) / "g1_fft_host"
    flags = ["-O2"] if request.param == "plain" else [
        "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([HIPCC, "--offload-host-only", "-std=c++17", "-I", CSRC] + flags +
                   [os.path.join(REPO, "tests", "native", "g1_fft_host.cpp"), "-o", str(exe)],
                   check=True, cwd=str(exe.parent))

    def go(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = r.stdout.splitlines()
        assert len(rows) == len(lines)
        for row in rows:
            assert not row.startswith("ERR"), row
        return [[int(x) for x in row.split()] for row in rows]
    return go


def fft_line(ms):
    k = len(ms).bit_length() - 1
    head = B.fr_mont_limbs(pow(B.omega_for(k), -1, R)) + B.to_limbs(pow(1 << k, -1, R))
    return "fft %d %s" % (k, " ".join(str(int(x)) for x in head + G.points(ms).reshape(-1).tolist()))


def check(run, cases):
    """cases: name -> m_j"""
    names = list(cases)
    got = run([fft_line(cases[nm]) for nm in names])
    for nm, row in zip(names, got):
        want = G.points(G.lagrange_scalars(cases[nm]))
        have = np.array(row, dtype=np.uint64).reshape(-1, 8)
        assert have.shape == want.shape, nm
        bad = np.nonzero((have != want).any(axis=1))[0]
        assert bad.size == 0, f"{nm}: outputs {bad[:8].tolist()} differ"


def test_index_functions(run):
    """every stage of k = 1 .. 9: the butterflies' (lo, hi) pairs partition the points, hi - lo
    is half the block, the twiddle index is (lo mod half) * n / m, and in a wave-uniform stage
    the 64 butterflies of a wave do share it"""
    lines, keys = [], []
    for k in range(1, 10):
        for s in range(1, k + 1):
            for t in range(1 << (k - 1)):
                lines.append(f"map {k} {s} {t}")
                keys.append((k, s, t))
    seen, tws = {}, {}
    for (k, s, t), (tw, lo, hi, uni) in zip(keys, run(lines)):
        n, m = 1 << k, 1 << s
        assert hi - lo == m // 2 and hi < n and lo // m == hi // m
        assert tw == (lo % (m // 2)) * (n // m) and tw < n // 2
        assert uni == int(k - s >= 6)
        seen.setdefault((k, s), set()).update((lo, hi))
        tws.setdefault((k, s, t // 64), set()).add(tw)
    for (k, s), pts in seen.items():
        assert pts == set(range(1 << k))
    for (k, s, _), tw in tws.items():
        if k - s >= 6:
            assert len(tw) == 1


@pytest.mark.parametrize("k", range(1, 9))
def test_random_multiples(run, k):
    check(run, {f"k{k}": G.random_ms(k, 100 + k)})


@pytest.mark.parametrize("k", [3, 6])
def test_edge_vectors(run, k):
    check(run, G.edge_vectors(k))


def test_edge_vectors_in_a_wave_uniform_stage(run):
    """k = 7: stage 1 is wave-uniform; the cancelling inputs meet in it"""
    ev = G.edge_vectors(7)
    check(run, {nm: ev[nm] for nm in ("all_equal", "negation_at_half_sparse", "negation_at_half_dense",
                                      "zero_one_minus_one")})
