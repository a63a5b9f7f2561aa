"""The Assigned-witness additions to the C ABI are declared, bound and additive; the size rule
answers without a device; the host entry validates its list before it asks for one; and the two
restatements of batch_invert_assigned in _assigned_ref.py agree (no GPU)."""
import ctypes

import numpy as np
import pytest

import _assigned_ref as AR
import h2g
import h2g_circuit as hc

NEW = ["h2g_assigned_to_fr", "h2g_assigned_to_fr_dev", "h2g_debug_assigned_per", "h2g_debug_assigned_to_fr_dev",
       "h2g_create_proof_assigned"]
H2G_OK, H2G_ERR_ARG, H2G_ERR_STATE = 0, 1, 4
PERS = (2, 4, 8, 16)  # what h2g_debug_assigned_to_fr_dev accepts (include/h2g.h)


def test_new_symbols_declared_and_bound():
    declared = h2g.header_symbols()
    L = h2g.lib()
    for name in NEW:
        assert name in declared, name
        assert name in h2g._SIGS, name
        assert hasattr(L, name), name
    for name in ("h2g_create_proof_multi", "h2g_fr_batch_invert_dev"):  # what they extend stays
        assert name in declared and name in h2g._SIGS


def test_struct_sizes_and_header_text():
    assert ctypes.sizeof(h2g.AssignedDens) == 24
    assert ctypes.sizeof(h2g.AssignedSource) == 16
    text = open(h2g.HEADER).read()
    assert "typedef struct { const uint64_t* index; const uint64_t* den; size_t count; } h2g_assigned_dens;" in text
    assert "circuit.rs:363-404" in text and "assigned.rs:280-295" in text and "assigned.rs:352-364" in text


def test_abi_version_unchanged():
    assert h2g.lib().h2g_abi_version() == 1


def test_size_rule_without_a_device():
    """h2g_debug_assigned_per needs no h2g_init, never decreases with nden, and answers only
    with values the override takes"""
    sizes = [0, 1, 2, 3, 255, 4096, 4097] + [(1 << s) + d for s in range(13, 27) for d in (-1, 0, 1)] + [1 << 40]
    got = [h2g.debug_assigned_per(n) for n in sorted(sizes)]
    assert all(p in PERS for p in got), got
    assert got == sorted(got), got
    assert got[0] == PERS[0] and got[-1] == PERS[-1]  # both ends of the rule are reached
    assert h2g.lib().h2g_debug_assigned_per(5, None) == H2G_ERR_ARG


def _host_call(num, index, den, out, nden=None):
    L = h2g.lib()
    return L.h2g_assigned_to_fr(h2g.p64(num), len(num), h2g.p64(index), h2g.p64(den),
                                len(index) if nden is None else nden, h2g.p64(out))


def test_host_entry_validates_before_any_device_use():
    """no h2g_init in this process: a call that reached the device would answer H2G_ERR_STATE
    (test_abi_cpu.py); the list's errors come first, name the entry, and leave out alone"""
    L = h2g.lib()
    num = hc.ints_to_mont([3, 4, 5, 6, 7, 8])
    den = hc.ints_to_mont([2, 2, 2])
    mark = np.full((6, 4), 0xABCD, dtype=np.uint64)

    def bad(index, d=den, nden=None):
        out = mark.copy()
        rc = _host_call(num, np.asarray(index, dtype=np.uint64), d, out, nden)
        assert np.array_equal(out, mark)
        return rc, L.h2g_last_error().decode()

    rc, msg = bad([1, 3, 6])  # an index equal to ncells
    assert rc == H2G_ERR_ARG and "index[2]" in msg and "6" in msg, msg
    rc, msg = bad([1, 3, 3])  # an equal pair
    assert rc == H2G_ERR_ARG and "index[2]" in msg and "strictly increasing" in msg, msg
    rc, msg = bad([1, 4, 2])  # a decreasing pair
    assert rc == H2G_ERR_ARG and "index[2]" in msg and "strictly increasing" in msg, msg
    rc, msg = bad([1, 3, 5], d=None, nden=3)  # no denominators for three entries
    assert rc == H2G_ERR_ARG and "null" in msg, msg
    # and a valid list does go on to the device: refused there without h2g_init (or, where an
    # earlier test of the same process has initialised one, converted)
    out = mark.copy()
    rc = _host_call(num, np.asarray([1, 3, 5], dtype=np.uint64), den, out)
    if rc == H2G_ERR_STATE:
        assert b"h2g_init" in L.h2g_last_error()
        assert np.array_equal(out, mark)
    else:
        assert rc == H2G_OK
        assert np.array_equal(out, AR.convert(num, [1, 3, 5], den))


def test_host_entry_without_divisions_needs_no_device():
    """ncells == 0 is H2G_OK; nden == 0 is a copy out of place and nothing in place"""
    num = hc.ints_to_mont([3, 4, 5])
    empty = np.zeros(0, dtype=np.uint64)
    assert h2g.lib().h2g_assigned_to_fr(None, 0, None, None, 0, None) == H2G_OK
    got = h2g.assigned_to_fr(num, empty, np.zeros((0, 4), dtype=np.uint64))
    assert np.array_equal(got, num) and got is not num
    same = num.copy()
    assert h2g.assigned_to_fr(same, empty, np.zeros((0, 4), dtype=np.uint64), out=same) is same
    assert np.array_equal(same, num)


def test_dev_entries_check_their_arguments_first():
    """a misaligned pointer and an unsupported per are H2G_ERR_ARG whatever the device's state"""
    L = h2g.lib()
    for per in (1, 3, 5, 32, -2):
        assert L.h2g_debug_assigned_to_fr_dev(4096, 4, 8192, 12288, 2, 4096, per, None) == H2G_ERR_ARG
        assert b"per" in L.h2g_last_error()
    for args in ((4104, 4, 8192, 12288, 2, 4096), (4096, 4, 8200, 12288, 2, 4096), (4096, 4, 8192, 12296, 2, 4096),
                 (4096, 4, 8192, 12288, 2, 4104)):
        assert L.h2g_assigned_to_fr_dev(*args, None) == H2G_ERR_ARG
        assert b"16-byte aligned" in L.h2g_last_error()


def test_the_two_references_agree_on_the_edge_values():
    """_assigned_ref.convert (the oracle's batch inversion and product) against convert_int
    (Python integers) on denominators 0, 1, r - 1, 2 under numerators 0, r - 1 and a random one"""
    num, index, den = AR.edge_case()
    assert len(num) <= 300
    want = AR.convert_int(num, index, den)
    got = AR.convert(hc.ints_to_mont(num), np.asarray(index, dtype=np.uint64), hc.ints_to_mont(den))
    assert hc.mont_to_ints(got) == want
    # spot values: x / 0 = 0, x / 1 = x, (r - 1) / (r - 1) = 1, unlisted cells keep their numerator
    by_cell = dict(zip(index, den))
    for c, d in by_cell.items():
        if d == 0:
            assert want[c] == 0
        if d == 1:
            assert want[c] == num[c]
        if d == AR.R - 1:
            assert want[c] == (AR.R - num[c]) % AR.R
    assert all(want[c] == num[c] for c in range(len(num)) if c not in by_cell)


def test_python_option_errors():
    with pytest.raises(AssertionError):
        h2g.assigned_to_fr(hc.ints_to_mont([1, 2]), np.asarray([0, 1], dtype=np.uint64), hc.ints_to_mont([1]))
