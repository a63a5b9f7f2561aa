"""The batched fixed-base MSM pipeline and the commitment schedule around it, on their own:
h2g_debug_msm_batches_dev launches MSMs against a base descriptor exactly as a proof stage
does -- batches of up to `chunk` back to back, every result collected after the last launch --
so the batch size and the window are the test's to choose, not a circuit's.

Every case first asserts with h2g.debug_msm_plan that its shape still selects the kernels it is
here for (tests/test_msm_plan_cpu.py pins the rule itself), then compares every MSM of the
batch with the oracle's best_multiexp of that column alone, exactly.  The columns of one batch
differ in kind, cycled by their index -- uniform, ones, zeros (the identity), r - 1, sparse,
small, a copy of column 0 -- so a bucket set that leaks into its neighbour shows.

The ring cases launch more MSMs than one block of result slots holds before any is collected
(h2g.debug_limits()["msm_ring"]): what a stage with that many commitments does, batched
(chunk = 64) and one pipeline per commitment (chunk = 1, the schedule of commitments too large
to batch)."""
import numpy as np
import pytest

import _oracle as O
import h2g

pytestmark = pytest.mark.gpu

N = 3000
N_DESC = 4000   # the offset case's descriptor
OFFSET = 517
GEN = np.array([0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f,
                0xa6ba871b8b1e1b3a, 0x14f1d651eb8e167b, 0xccdd46def0f28c58, 0x1c14ef83340fbe5e], dtype=np.uint64)
R_MINUS_1 = np.array([0x43e1f593f0000000, 0x2833e84879b97091, 0xb85045b68181585d, 0x30644e72e131a029],
                     dtype=np.uint64)
KINDS = ("uniform", "ones", "zeros", "r - 1", "sparse", "small", "copy of column 0")
LIM = h2g.debug_limits()
RING, BATCH = LIM["msm_ring"], LIM["msm_batch"]
POOL = 2 * RING + 1


def column(i, n, first=None):
    """column i of a batch, n scalars: its kind is KINDS[i % 7]"""
    r = np.random.default_rng([i, n])
    kind = KINDS[i % len(KINDS)]
    if kind == "uniform":
        return O.random_fr(r, n)
    if kind == "ones":
        return O.fr_from_canonical(np.tile(np.array([1, 0, 0, 0], dtype=np.uint64), (n, 1)))
    if kind == "zeros":
        return np.zeros((n, 4), dtype=np.uint64)
    if kind == "r - 1":
        return np.tile(O.fr_from_canonical(R_MINUS_1), (n, 1))
    if kind == "sparse":   # 1 in 64 non-zero
        sc = O.random_fr(r, n)
        sc[r.integers(0, 64, size=n) != 0] = 0
        return sc
    if kind == "small":
        c = np.zeros((n, 4), dtype=np.uint64)
        c[:, 0] = r.integers(0, 1 << 16, size=n).astype(np.uint64)
        return O.fr_from_canonical(c)
    return first.copy()


def columns(count, n):
    cols = []
    for i in range(count):
        cols.append(column(i, n, cols[0] if cols else None))
    return cols


class Inputs:
    """an SRS of N_DESC points, POOL columns of N scalars on the device, and the oracle's MSM of
    each against the first N points -- computed once for the module"""

    def __init__(self):
        r = np.random.default_rng(2024)
        self.s = O.random_fr(r, 1)[0]
        self.d_bases = h2g.DevBuf(N_DESC * 64)
        h2g.srs_setup_dev(self.s, N_DESC, self.d_bases.ptr)
        self.bases = self.d_bases.download((N_DESC, 8))
        self.cols = columns(POOL, N)
        self.d_cols = h2g.DevBuf.from_array(np.stack(self.cols))
        self.ptrs = [self.d_cols.ptr + i * N * 32 for i in range(POOL)]
        self.want = {}
        self._desc = {}

    def expected(self, i, offset=0):
        if (i, offset) not in self.want:
            j = 0 if i % len(KINDS) == 6 else i
            if (j, offset) not in self.want:
                self.want[(j, offset)] = O.msm_best(self.cols[j], self.bases[offset:offset + N], 8)
            self.want[(i, offset)] = self.want[(j, offset)]
        return self.want[(i, offset)]

    def desc(self, c, n=N):
        if (c, n) not in self._desc:
            self._desc[(c, n)] = h2g.base_descriptor_dev(self.d_bases.ptr, n, c)
        return self._desc[(c, n)]

    def drop_descs(self):
        for h in self._desc.values():
            h2g.descriptor_free(h)
        self._desc.clear()

    def close(self):
        self.drop_descs()
        self.d_cols.close()
        self.d_bases.close()


@pytest.fixture(scope="module")
def inp():
    h2g.init()
    x = Inputs()
    yield x
    x.close()


def run_and_compare(inp, c, nb_total, chunk, offset=0, n_desc=N):
    got, ids = h2g.debug_msm_batches_dev(inp.desc(c, n_desc), inp.ptrs[:nb_total], N, chunk, offset)
    assert got.shape == (nb_total, 8)
    for i in range(nb_total):
        assert np.array_equal(got[i], inp.expected(i, offset)), (c, nb_total, chunk, i, KINDS[i % 7])
        zero = i % len(KINDS) == 2
        assert ids[i] == (1 if zero else 0), (c, nb_total, i)
        if zero:
            assert not got[i].any()
        if i % len(KINDS) == 6:
            assert np.array_equal(got[i], got[0])
    inp.drop_descs()


# (c, nbatch): what the shape must select in h2g.debug_msm_plan
CASES = {
    (11, 32): dict(nbt=32768, fixup_q=4),
    (11, 33): dict(nbt=33792, fixup_q=1),
    (16, 2): dict(red="plane", plane_q=4, rgp=1),
    (16, 4): dict(red="plane", plane_q=4, rgp=2),
    (16, 5): dict(red="plane", plane_q=4, rgp=4),
    (11, 64): dict(red="plane", plane_q=4, rgp=1, nbt=1 << 16),
    (12, 64): dict(red="plane", plane_q=4, rgp=2, nbt=1 << 17),
    (13, 64): dict(red="plane", plane_q=4, rgp=4, nbt=1 << 18),
    (14, 33): dict(red="plane", plane_q=1, rgp=8, nbt=33 << 13),
    (19, 2): dict(red="plane", plane_q=1, rgp=8, nbt=1 << 19, WB=2),
    (17, 32): dict(red="plane", plane_q=1, nbt=1 << 21, fb=10, ncoarse=2048),
    (17, 64): dict(red="plane", plane_q=1, nbt=1 << 22, fb=11, ncoarse=2048),
    (22, 2): dict(red="rscale", WB=2, nbt=1 << 22, m1=1 << 18),
}


@pytest.mark.parametrize("c,nbatch", sorted(CASES), ids=[f"c{c}-b{b}" for c, b in sorted(CASES)])
def test_batched_variant(inp, c, nbatch):
    want_plan = CASES[(c, nbatch)]
    pl = h2g.debug_msm_plan(N, c, fixed=True, nbatch=nbatch)
    assert {k: pl[k] for k in want_plan} == want_plan
    assert pl["staged"] == 1 and pl["nbatch"] == nbatch
    run_and_compare(inp, c, nbatch, BATCH)


def test_refused_batch_launches_nothing_and_the_next_is_right(inp):
    """33 sets of 2^17 buckets are past the partition's 2^22 keys: the argument error, before
    any launch -- no result slot stays taken, and the device goes on"""
    with pytest.raises(h2g.H2GError):
        h2g.debug_msm_plan(N, 18, fixed=True, nbatch=33)
    h2g.debug_msm_plan(N, 18, fixed=True, nbatch=32)
    with pytest.raises(h2g.H2GError, match="^h2g error 1: .*refuses"):
        h2g.debug_msm_batches_dev(inp.desc(18), inp.ptrs[:33], N, BATCH)
    inp.drop_descs()
    run_and_compare(inp, 13, 64, BATCH)


def test_base_offset_into_a_longer_table(inp):
    """the slab path's table offset: points [517, 3517) of a table over 4000"""
    for c, nb in ((13, 9), (16, 2)):
        pl = h2g.debug_msm_plan(N, c, fixed=True, nbatch=nb)
        assert pl["WB"] == nb
        run_and_compare(inp, c, nb, BATCH, offset=OFFSET, n_desc=N_DESC)
    with pytest.raises(h2g.H2GError, match="bases.len"):
        h2g.debug_msm_batches_dev(inp.desc(13, N_DESC), inp.ptrs[:2], N, BATCH, N_DESC - N + 1)
    inp.drop_descs()


def test_unstaged_fine_pass(inp):
    """2^25 entries take the fine pass without its LDS staging.  16 columns of 2^17 scalars,
    checked by the SRS identity sum_i c_i [s^i]G = [c(s)]G"""
    n, c, nb = 1 << 17, 16, 16
    pl = h2g.debug_msm_plan(n, c, fixed=True, nbatch=nb)
    assert (pl["total"], pl["staged"], pl["WB"]) == (1 << 25, 0, nb)
    assert h2g.debug_msm_plan(n, c, fixed=True, nbatch=nb - 1)["staged"] == 1
    d_bases = h2g.DevBuf(n * 64)
    h2g.srs_setup_dev(inp.s, n, d_bases.ptr)
    cols = columns(nb, n)
    d_cols = h2g.DevBuf.from_array(np.stack(cols))
    h = h2g.base_descriptor_dev(d_bases.ptr, n, c)
    try:
        got, ids = h2g.debug_msm_batches_dev(h, [d_cols.ptr + i * n * 32 for i in range(nb)], n, BATCH)
    finally:
        h2g.descriptor_free(h)
        d_cols.close()
        d_bases.close()
    for i in range(nb):
        if i % len(KINDS) == 2:
            assert ids[i] == 1 and not got[i].any()
            continue
        want = O.g1_mul(GEN, O.eval_poly(cols[i], inp.s))
        assert ids[i] == 0 and np.array_equal(got[i], want), (i, KINDS[i % 7])
    assert np.array_equal(got[7 - 1], got[0]) and np.array_equal(got[14 - 1], got[0])


RING_CASES = [(RING, BATCH), (RING + 1, BATCH), (2 * RING + 1, BATCH), (RING + 1, 1), (RING + 6, 7)]


@pytest.mark.parametrize("nb_total,chunk", RING_CASES, ids=[f"{a}-by-{b}" for a, b in RING_CASES])
def test_more_msms_outstanding_than_result_slots(inp, nb_total, chunk):
    """every batch is launched before the first result is collected, as in a proof stage: with
    more MSMs than one block of result slots the ring grows, and each result is still its own"""
    pl =h2g.debug_msm_plan(N, 13, fixed=True, nbatch=min(chunk, nb_total))
    assert pl["red"] == "plane" and pl["WB"] == min(chunk, nb_total)
    run_and_compare(inp, 13, nb_total, chunk)
    run_and_compare(inp, 13, min(nb_total, 9), chunk)   # and the slots are all free again
