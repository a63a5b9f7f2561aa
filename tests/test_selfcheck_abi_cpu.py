"""The prover's self-checks in the C ABI: the new entries are declared, bound and exported
beside the ones they extend, the ABI version stays, the error code and record kinds have the
values the header gives them, and the calls that need a device say so before h2g_init.  No GPU."""
import ctypes
import re

import pytest

import h2g

ERR_ARG, ERR_STATE, ERR_HANDLE, ERR_UNSATISFIED = 1, 4, 5, 6
NEW = ["h2g_pk_set_self_check", "h2g_last_self_check", "h2g_debug_selfcheck_product_dev",
       "h2g_debug_selfcheck_permuted_dev", "h2g_debug_selfcheck_permutation_dev"]


def test_new_symbols_declared_bound_and_exported():
    declared = h2g.header_symbols()
    L = h2g.lib()
    for name in NEW:
        assert name in declared, name
        assert name in h2g._SIGS, name
        assert hasattr(L, name), name
    for name in ("h2g_create_proof", "h2g_create_proof_phased", "h2g_create_proof_multi",
                 "h2g_create_proof_assigned", "h2g_check_witness", "h2g_pk_set_multiopen", "h2g_last_challenges"):
        assert name in declared and name in h2g._SIGS and hasattr(L, name)
    assert L.h2g_abi_version() == 1


def test_header_values():
    text = open(h2g.HEADER).read()
    assert "H2G_ERR_UNSATISFIED = 6" in text and "H2G_ERR_HANDLE = 5," in text
    assert "H2G_SELFCHECK_OFF = 0, H2G_SELFCHECK_VERDICT = 1, H2G_SELFCHECK_ARGUMENTS = 2" in text
    kinds = dict(re.findall(r"H2G_CHECK_(\w+) = (\d+)", text))
    assert {k: int(v) for k, v in kinds.items()} == {
        "GATE": 1, "GATE_BLINDING": 2, "LOOKUP": 3, "SHUFFLE": 4, "COPY": 5, "PERMUTATION": 6, "PRODUCT": 7,
        "PERMUTED_PAIR": 8, "UNUSABLE_ROW": 9, "IDENTITY": 10}
    assert (h2g.CHECK_PERMUTATION, h2g.CHECK_PRODUCT, h2g.CHECK_PERMUTED_PAIR, h2g.CHECK_UNUSABLE_ROW,
            h2g.CHECK_IDENTITY) == (6, 7, 8, 9, 10)
    assert h2g.ERR_UNSATISFIED == ERR_UNSATISFIED and h2g.SELF_CHECK_MODES == {"off": 0, "verdict": 1, "arguments": 2}
    assert ctypes.sizeof(h2g.CheckFailure) == 16   # the records of h2g_check_witness, `reserved` = the circuit


def test_set_self_check_arguments():
    """host state only: an unknown mode is H2G_ERR_ARG, an unknown key H2G_ERR_HANDLE"""
    L = h2g.lib()
    for mode in (3, -1, 100):
        assert L.h2g_pk_set_self_check(0xDEAD, mode) == ERR_ARG
        assert b"mode must be" in L.h2g_last_error()
    for mode in (0, 1, 2):
        assert L.h2g_pk_set_self_check(0xDEAD, mode) == ERR_HANDLE
    with pytest.raises(h2g.H2GError) as e:
        h2g.check(L.h2g_pk_set_self_check(0xDEAD, 1))
    assert e.value.code == ERR_HANDLE and e.value.failures == [] and e.value.total == 0


_BEFORE_INIT = r"""
import ctypes, sys
sys.path[:0] = %r
import h2g
L = h2g.lib()
total = h2g.U64(7)
out = (h2g.CheckFailure * 4)()
assert L.h2g_last_self_check(ctypes.cast(out, h2g.VP), 4, ctypes.byref(total)) == 4
assert b"h2g_init" in L.h2g_last_error() and total.value == 7
one = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
buf = ctypes.create_string_buffer(32 * 8)
p = ctypes.cast(buf, h2g.VP)
assert L.h2g_debug_selfcheck_product_dev(p, p, p, p, p, one, one, 8, 5, 0, ctypes.cast(out, h2g.VP), 4,
                                         ctypes.byref(total)) == 4
assert L.h2g_debug_selfcheck_permuted_dev(p, p, 5, 0, ctypes.cast(out, h2g.VP), 4, ctypes.byref(total)) == 4
try:
    h2g.last_self_check()
except h2g.H2GError as e:
    assert e.code == 4 and "h2g_init" in str(e)
else:
    raise AssertionError("last_self_check before h2g_init did not raise")
print("before-init ok")
"""


def test_device_calls_before_init_fail_loudly():
    """H2G_ERR_STATE naming h2g_init, nothing written -- in a process of its own, which never
    initialises the library (this one may have, in a GPU run of the whole suite)"""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, "-c", _BEFORE_INIT % (sys.path,)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "before-init ok" in r.stdout, r.stdout + r.stderr


def test_error_classes():
    assert issubclass(h2g.UnsatisfiedError, h2g.H2GError)
    e = h2g.UnsatisfiedError("m", code=6, failures=[(1, 0, 3, 0)], total=5)
    assert (e.code, e.failures, e.total) == (6, [(1, 0, 3, 0)], 5)
    assert h2g.H2GError("plain").failures == []
