"""CPU-side checks of the C ABI library: it loads, exports every symbol that
include/h2g.h declares, and fails loudly (no CPU fallback) without a device."""
import ctypes

import numpy as np
import pytest

import h2g


def test_library_exports_every_header_symbol():
    L = h2g.lib()
    syms = h2g.header_symbols()
    assert len(syms) >= 40
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing
    # and the Python binding covers all of them
    assert set(syms) == set(h2g._SIGS), set(syms) ^ set(h2g._SIGS)


def test_abi_version():
    assert h2g.lib().h2g_abi_version() == 1


def test_calls_before_init_fail_loudly():
    a = np.zeros((4, 4), dtype=np.uint64)
    rc = h2g.lib().h2g_fr_batch_invert(h2g.p64(a), 4)
    assert rc == 4  # H2G_ERR_STATE
    assert b"h2g_init" in h2g.lib().h2g_last_error()


def test_host_point_add_matches_oracle(golden):
    import _oracle as O
    g = golden["msm"]
    pts = g["srs_random_k3__bases"]
    for i in range(len(pts) - 1):
        assert np.array_equal(h2g.g1_add_affine(pts[i], pts[i + 1]), O.g1_add(pts[i], pts[i + 1]))
    # doubling and identity handling
    assert np.array_equal(h2g.g1_add_affine(pts[1], pts[1]), O.g1_add(pts[1], pts[1]))
    z = np.zeros(8, dtype=np.uint64)
    assert np.array_equal(h2g.g1_add_affine(pts[2], z), pts[2])


def test_capacity_and_commit_schedule_seams_are_exported_and_host_only():
    """h2g_debug_limits and h2g_debug_commit_batch_chunk answer without h2g_init; the device
    seam h2g_debug_msm_batches_dev is declared, bound, exported and refuses to run without one"""
    L = h2g.lib()
    for name in ("h2g_debug_limits", "h2g_debug_commit_batch_chunk", "h2g_debug_msm_batches_dev"):
        assert name in h2g.header_symbols() and name in h2g._SIGS and hasattr(L, name), name
    n = ctypes.c_int(0)
    assert L.h2g_debug_limits(None, 0, ctypes.byref(n)) == 0 and n.value == len(h2g.LIMITS) == 10
    out = (ctypes.c_int32 * 12)(*([-1] * 12))
    assert L.h2g_debug_limits(out, 3, ctypes.byref(n)) == 0 and list(out)[:4] == [16, 16, 32, -1]
    assert L.h2g_debug_limits(out, 12, ctypes.byref(n)) == 0 and n.value == 10 and list(out)[10:] == [-1, -1]
    assert list(out)[:10] == list(h2g.debug_limits().values())
    assert L.h2g_debug_limits(out, 10, None) == 1 and L.h2g_debug_limits(None, 10, ctypes.byref(n)) == 1
    assert L.h2g_debug_limits(out, -1, ctypes.byref(n)) == 1   # H2G_ERR_ARG
    ch = ctypes.c_int(0)
    assert L.h2g_debug_commit_batch_chunk(17, 1 << 18, ctypes.byref(ch)) == 0 and ch.value == 34
    assert L.h2g_debug_commit_batch_chunk(20, 1 << 22, ctypes.byref(ch)) == 0 and ch.value == 1
    assert L.h2g_debug_commit_batch_chunk(17, 1 << 18, None) == 1
    assert L.h2g_debug_commit_batch_chunk(0, 1 << 18, ctypes.byref(ch)) == 1
    assert L.h2g_debug_commit_batch_chunk(32, 1 << 18, ctypes.byref(ch)) == 1
    with pytest.raises(h2g.H2GError, match="h2g_init"):
        h2g.debug_msm_batches_dev(1, [], 0, 1)
