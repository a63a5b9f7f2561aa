"""GPU parity of the MSM accumulation's run handling (csrc/msm_acc.hip), bit-exact against
the C oracle.

The accumulation walks the bucket-sorted entries in chunks of L, one thread per chunk; a
run is one bucket's entries inside one chunk.  Its hot loop starts a run from the run's
first point, keeps "the sum is the identity" in a flag and leaves p == q to a repair
launch, so the cases here are shaped by where runs start and end and by what a run's sum
meets on the way, not by the values (tests/test_gpu_adversarial.py has those):
  * every scalar equal: one bucket per window, its run crossing every chunk boundary;
  * every digit distinct: every run has length 1, a run ends on every step;
  * only positive digits, and negative digits in every window but the one that takes the
    last carry;
  * buckets holding P, -P, P, ...: the identity in the middle of a run, then a restart;
  * the same followed by P, P: the doubling, hence the repair launch;
  * buckets of exactly 1, 2, 3, L - 1, L and L + 1 entries (L = 8 at these sizes:
    msm.hip msm_chunk_len);
  * zero scalars mixed in, and identity bases.
Scalars are built from signed digits for window widths 8 and 13 (the low windows have that
width in the uniform and in the balanced layout); every case runs through h2g.msm,
h2g.msm_with_cached_base and h2g.msm_dev at both widths.  All sizes are at most 2^12 points.
"""
import os
import sys

import numpy as np
import pytest

import _oracle as O
import h2g

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "py"))
import bn254_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu

N = 1 << 12
L = 8  # the chunk length msm_chunk_len picks for at most 2^12 points
WIDTHS = (8, 13)


@pytest.fixture(scope="module", autouse=True)
def engine():
    h2g.init()
    yield
    h2g.shutdown()


@pytest.fixture(scope="module")
def points():
    """2^12 distinct points (an SRS), as the (n, 8) limb array and never changed"""
    buf = h2g.DevBuf(N * 64)
    try:
        h2g.srs_setup_dev(O.random_fr(np.random.default_rng(5), 1)[0], N, buf.ptr)
        return buf.download((N, 8))
    finally:
        buf.close()


def _fr(ints):
    can = np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in ints], dtype=np.uint64)
    return O.fr_from_canonical(can)


def _scalar(digits, wb):
    """the scalar with the given signed digits in windows 0, 1, ... of width wb; the top
    digit given is positive, so the value is positive and its signed decomposition is this"""
    half = 1 << (wb - 1)
    assert all(-half < d <= half for d in digits) and digits[-1] > 0
    return sum(d << (wb * w) for w, d in enumerate(digits))


def _neg_row(row):
    """-P for an affine point given as its limb row: the stored y -> p - y"""
    r = row.copy()
    y_st = sum(int(row[4 + i]) << (64 * i) for i in range(4))  # the stored (Montgomery) y
    ny = (B.P - y_st) % B.P                                  # -y in the same form
    for i in range(4):
        r[4 + i] = (ny >> (64 * i)) & 0xFFFFFFFFFFFFFFFF
    return r


def _check(sc, bases):
    want = O.msm_best(sc, bases, 8)
    n = len(bases)
    assert np.array_equal(h2g.msm(sc, bases), want), "msm"
    hb = h2g.base_descriptor(bases)
    try:
        assert np.array_equal(h2g.msm_with_cached_base(sc, hb), want), "msm_with_cached_base"
    finally:
        h2g.descriptor_free(hb)
    dsc, dbs, dout = h2g.DevBuf.from_array(sc), h2g.DevBuf.from_array(bases), h2g.DevBuf(64)
    try:
        for wb in WIDTHS:
            h2g.msm_dev(dsc.ptr, dbs.ptr, n, dout.ptr, window_bits=wb)
            assert np.array_equal(dout.download(8), want), ("msm_dev", wb)
    finally:
        for b in (dsc, dbs, dout):
            b.close()


@pytest.mark.parametrize("wb", WIDTHS)
def test_every_scalar_equal_one_run_across_every_chunk(points, wb):
    n = 1024
    s = _scalar([5, -3, 7], wb)
    _check(_fr([s] * n), points[:n])


@pytest.mark.parametrize("wb", WIDTHS)
def test_every_digit_distinct_runs_of_length_one(points, wb):
    half = 1 << (wb - 1)
    n = min(half - 1, N - 1)
    r = np.random.default_rng(wb)
    perms = [r.permutation(n) + 1 for _ in range(3)]
    sc = [_scalar([int(p[i]) for p in perms], wb) for i in range(n)]
    _check(_fr(sc), points[:n])


@pytest.mark.parametrize("sign", [1, -1], ids=["positive", "negative"])
@pytest.mark.parametrize("wb", WIDTHS)
def test_digits_of_one_sign(points, wb, sign):
    """negative: windows 0..2 hold negative digits, window 3 the closing carry (digit 1)"""
    half = 1 << (wb - 1)
    n = 1024
    r = np.random.default_rng(10 * wb + (sign > 0))
    d = r.integers(1, half, size=(n, 3))
    sc = [_scalar([sign * int(x) for x in row] + [1], wb) for row in d]
    _check(_fr(sc), points[:n])


def _groups(points, wb, tail):
    """bucket g + 1 of window 0 (and of window 1, by the second digit) holds P_g, -P_g
    repeated m_g times, then `tail` more copies of P_g; P_g distinct per group"""
    rows, sc = [], []
    for g in range(48):
        p = points[g:g + 1]
        pair = np.concatenate([p, _neg_row(p[0])[None, :]])
        m = 1 + g % 5
        rows += [pair] * m + [p] * tail
        sc += [_scalar([g + 1, 2 * g + 1], wb)] * (2 * m + tail)
    return _fr(sc), np.concatenate(rows)


@pytest.mark.parametrize("wb", WIDTHS)
def test_identity_in_the_middle_of_a_run(points, wb):
    """P, -P, P, -P, ...: every bucket's sum is the identity, met m_g times on the way"""
    _check(*_groups(points, wb, 0))


@pytest.mark.parametrize("wb", WIDTHS)
def test_identity_then_the_doubling(points, wb):
    """... then P, P: the run restarts from P and meets p == q (the repair launch)"""
    _check(*_groups(points, wb, 2))


@pytest.mark.parametrize("wb", WIDTHS)
def test_identity_then_one_more_point(points, wb):
    """... then one P: the restart alone"""
    _check(*_groups(points, wb, 1))


@pytest.mark.parametrize("wb", WIDTHS)
def test_run_lengths_around_the_chunk_length(points, wb):
    """buckets of exactly 1, 2, 3, L - 1, L, L + 1 entries, in that order and again"""
    lens = [1, 2, 3, L - 1, L, L + 1]
    half = 1 << (wb - 1)
    sc, digit = [], 1
    while digit < min(half, 600) and len(sc) + L + 1 <= N:
        sc += [_scalar([digit, (digit % 7) + 1], wb)] * lens[digit % len(lens)]
        digit += 1
    _check(_fr(sc), points[:len(sc)])


@pytest.mark.parametrize("wb", WIDTHS)
def test_zero_scalars_and_identity_bases_mixed_in(points, wb):
    n = 2048
    r = np.random.default_rng(40 + wb)
    sc = O.random_fr(r, n)
    sc[r.random(n) < 0.5] = 0
    small = r.random(n) < 0.2   # short scalars: two windows, the rest of the digits zero
    sc[small] = _fr([_scalar([int(a), int(b)], wb) for a, b in r.integers(1, 1 << (wb - 1), size=(int(small.sum()), 2))])
    bases = points[:n].copy()
    bases[r.random(n) < 0.1] = 0  # the identity: (0, 0)
    _check(sc, bases)
