"""h2g_assigned_to_fr on the device against _assigned_ref (batch_invert_assigned restated on the
oracle and, for the edge values, on Python integers), bit for bit: every list length around the
block and thread boundaries, every elements-per-thread variant at the sizes where its split
changes shape, the edge values, both the in-place and the out-of-place form, and the device
entry's contract for indices out of range and misaligned pointers.

The variants are reached through h2g_debug_assigned_to_fr_dev, so the largest case but one is
256 * 16 * 16 + 1 denominators; the size rule itself runs once, at 2^18 + 3."""
import numpy as np
import pytest

import _assigned_ref as AR
import _oracle as O
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

PERS = (2, 4, 8, 16)
NCELLS = 4099
PT, INV_REG = 256, 16  # threads per block; elements a middle-level thread holds (csrc/poly.hip)


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()


def run_dev(num, idx, den, per=None, in_place=False, pad_cells=0):
    """the device entry (the override when per is given) on fresh buffers -> (out, num afterwards,
    den afterwards, idx afterwards); pad_cells more cells of 0xEE bytes follow num and out"""
    ncells, nden = len(num), len(idx)
    pad = np.full((pad_cells, 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    d_num = h2g.DevBuf.from_array(np.concatenate([num, pad]))
    d_out = d_num if in_place else h2g.DevBuf.from_array(np.concatenate([np.full_like(num, 0xDD), pad]))
    d_idx = h2g.DevBuf.from_array(idx if nden else np.zeros(2, dtype=np.uint64))
    d_den = h2g.DevBuf.from_array(den if nden else np.zeros((1, 4), dtype=np.uint64))
    try:
        if per is None:
            h2g.assigned_to_fr_dev(d_num.ptr, ncells, d_idx.ptr, d_den.ptr, nden, d_out.ptr)
        else:
            h2g.debug_assigned_to_fr_dev(d_num.ptr, ncells, d_idx.ptr, d_den.ptr, nden, d_out.ptr, per=per)
        h2g.check(h2g.lib().h2g_synchronize())
        out = d_out.download((ncells + pad_cells, 4))
        num_after = d_num.download((ncells + pad_cells, 4))
        den_after = d_den.download((nden, 4)) if nden else den
        idx_after = d_idx.download((nden,)) if nden else idx
    finally:
        for b in {d_num, d_out, d_idx, d_den}:
            b.close()
    assert np.array_equal(out[ncells:], pad) and np.array_equal(num_after[ncells:], pad)
    return out[:ncells], num_after[:ncells], den_after, idx_after


def check_both_forms(num, idx, den, per=None, want=None):
    want = AR.convert(num, idx, den) if want is None else want
    out, num_after, den_after, idx_after = run_dev(num, idx, den, per, in_place=False)
    assert np.array_equal(out, want)
    assert np.array_equal(num_after, num), "num was modified out of place"
    assert np.array_equal(den_after, den), "den was modified"
    assert np.array_equal(idx_after, idx)
    listed = np.zeros(len(num), dtype=bool)
    listed[idx.astype(np.int64)] = True
    assert np.array_equal(out[~listed], num[~listed]), "unlisted cells were not copied"
    out, _, den_after, _ = run_dev(num, idx, den, per, in_place=True)
    assert np.array_equal(out, want)
    assert np.array_equal(den_after, den), "den was modified in place"
    return want


@pytest.mark.parametrize("nden", [0, 1, 2, 3, 255, 256, 257, NCELLS])
def test_list_lengths(nden):
    """4099 cells, random Rational cells that always include cell 0 and the last cell (4099:
    every cell), by the size rule"""
    rng = np.random.default_rng(1000 + nden)
    num, idx, den = AR.random_case(rng, NCELLS, nden)
    assert len(idx) == nden and (nden < 2 or (idx[0] == 0 and idx[-1] == NCELLS - 1))
    check_both_forms(num, idx, den)


@pytest.mark.parametrize("per", PERS)
def test_every_variant_at_its_boundaries(per):
    """a thread with one element, a ragged last thread, one block less one, exactly one block,
    and more first-level threads (256 * 16 + 1) than one middle-level block inverts"""
    for nden in (per, per + 1, PT * per - 1, PT * per, PT * per * INV_REG + 1):
        rng = np.random.default_rng(per * 1000003 + nden)
        num, idx, den = AR.random_case(rng, nden + 37, nden)
        check_both_forms(num, idx, den, per=per)


def test_rule_answers_are_accepted_and_others_refused():
    for nden in (1, 4099, 1 << 20, 1 << 24):
        assert h2g.debug_assigned_per(nden) in PERS
    d = h2g.DevBuf(4096)
    try:
        for per in (1, 3, 32, -1):
            with pytest.raises(h2g.H2GError, match="per must be"):
                h2g.debug_assigned_to_fr_dev(d.ptr, 4, d.ptr + 1024, d.ptr + 2048, 2, d.ptr, per=per)
    finally:
        d.close()


def test_edge_values_against_python_integers():
    """denominators 0, 1, r - 1, 2 under numerators 0, r - 1 and a random one: the pin that does
    not rest on the oracle's inversion"""
    num, index, den = AR.edge_case()
    want = hc.ints_to_mont(AR.convert_int(num, index, den))
    idx = np.asarray(index, dtype=np.uint64)
    for per in (None,) + PERS:
        check_both_forms(hc.ints_to_mont(num), idx, hc.ints_to_mont(den), per=per, want=want)
    got = h2g.assigned_to_fr(hc.ints_to_mont(num), idx, hc.ints_to_mont(den))  # the host entry
    assert np.array_equal(got, want)


def _edge_dens(rng, nden):
    den = O.random_fr(rng, nden)
    edges = hc.ints_to_mont(list(AR.EDGE_DENS))
    for j in range(0, nden, 7):
        den[j] = edges[(j // 7) % len(edges)]
    return den


@pytest.mark.parametrize("per", PERS)
def test_zero_patterns(per):
    """zero denominators give 0 and leave their neighbours' inverses right: edge denominators
    scattered through the list, a run of 300 consecutive zeros, every element of some threads
    zero (thread t of T holds t, t + T, ...: zeros at every j = t mod T for a fifth of the t),
    and all denominators zero; numerators 0 and r - 1 among the random ones"""
    nden = PT * per + 2 * per + 1
    T = (nden + per - 1) // per
    rng = np.random.default_rng(4242 + per)
    num, idx, _ = AR.random_case(rng, nden + 11, nden)
    num[3::9] = 0
    num[4::9] = hc.ints_to_mont([AR.R - 1])[0]
    zero = np.zeros(4, dtype=np.uint64)

    scattered = _edge_dens(rng, nden)
    want = check_both_forms(num, idx, scattered, per=per)
    zc = idx[np.all(scattered == 0, axis=1)].astype(np.int64)
    assert len(zc) and not want[zc].any()

    run = _edge_dens(rng, nden)
    run[100:400] = zero
    check_both_forms(num, idx, run, per=per)

    threads = O.random_fr(rng, nden)
    threads[np.arange(nden) % T % 5 == 0] = zero
    assert all(not threads[t::T].any() for t in range(0, T, 5))
    check_both_forms(num, idx, threads, per=per)

    want = check_both_forms(num, idx, np.zeros((nden, 4), dtype=np.uint64), per=per)
    assert not want[idx.astype(np.int64)].any()


def test_host_entry_both_forms():
    rng = np.random.default_rng(9)
    num, idx, den = AR.random_case(rng, NCELLS, 1500)
    den[::11] = 0
    want = AR.convert(num, idx, den)
    keep_num, keep_den = num.copy(), den.copy()
    got = h2g.assigned_to_fr(num, idx, den)
    assert np.array_equal(got, want) and np.array_equal(num, keep_num) and np.array_equal(den, keep_den)
    same = num.copy()
    assert h2g.assigned_to_fr(same, idx, den, out=same) is same
    assert np.array_equal(same, want) and np.array_equal(den, keep_den)


@pytest.mark.parametrize("per", (None, 2, 16))
def test_out_of_range_index_is_skipped(per):
    """the device entry's index contract is the caller's: an index >= ncells in the middle of the
    list is skipped -- its neighbours come out right, nothing at or past ncells is written, no
    error is left on the device.  The buffers hold 600 cells past ncells, so the entry's address
    is in owned memory either way; those cells keep their fill."""
    rng = np.random.default_rng(31)
    ncells, nden, pad = 2000, 700, 600
    num, idx, den = AR.random_case(rng, ncells, nden)
    good = np.ones(nden, dtype=bool)
    for j, beyond in ((0, ncells), (350, ncells + 5), (351, ncells + pad - 1), (nden - 1, ncells + 17)):
        idx[j] = beyond
        good[j] = False
    want = AR.convert(num, idx[good], den[good])
    for in_place in (False, True):
        out, _, den_after, _ = run_dev(num, idx, den, per, in_place=in_place, pad_cells=pad)
        assert np.array_equal(out, want)
        assert np.array_equal(den_after, den)
    assert h2g.lib().h2g_synchronize() == 0


def test_repeated_index_does_not_fault():
    """a repeated index: that cell's value is unspecified, every other cell is right"""
    rng = np.random.default_rng(32)
    num, idx, den = AR.random_case(rng, 1000, 400)
    idx[200] = idx[199]
    keep = np.ones(400, dtype=bool)
    keep[200] = False
    want = AR.convert(num, idx[keep], den[keep])
    out, _, _, _ = run_dev(num, idx, den, in_place=True)
    others = np.ones(1000, dtype=bool)
    others[int(idx[199])] = False
    assert np.array_equal(out[others], want[others])
    assert h2g.lib().h2g_synchronize() == 0


def test_misaligned_pointers_are_refused():
    d = h2g.DevBuf(1 << 16)
    base = d.ptr
    try:
        ok = (base, 16, base + 8192, base + 16384, 4, base + 32768)
        for k in (0, 2, 3, 5):
            args = list(ok)
            args[k] += 8
            with pytest.raises(h2g.H2GError, match="16-byte aligned"):
                h2g.assigned_to_fr_dev(*args)
    finally:
        d.close()


def test_size_rule_path():
    """no override, 2^18 + 3 denominators among 2^18 + 1003 cells, in place"""
    rng = np.random.default_rng(18)
    nden = (1 << 18) + 3
    num, idx, den = AR.random_case(rng, nden + 1000, nden)
    den[5::1001] = 0
    want = AR.convert(num, idx, den)
    out, _, den_after, _ = run_dev(num, idx, den, in_place=True)
    assert np.array_equal(out, want)
    assert np.array_equal(den_after, den)
