"""kate_division's size rule (kate_tile_s in csrc/prover_kernels.hip) through its host-only
seam, h2g_debug_kate_tile_s: which compiled variant (coefficients per thread, 8 / 16 / 32)
serves which length.  No GPU: the rule is host code and needs no h2g_init.

The rule doubles S from 8 while S < 32 and ceil((len - 1) / (256 S 2)) >= 512, so
  S = 8   for len - 1 <= 511 * 4096  = 2 093 056,
  S = 16  for len - 1 <= 511 * 8192  = 4 186 112,
  S = 32  above.
tests/test_gpu_scan_variants.py runs the kernels at these lengths."""
import ctypes

import pytest

import h2g

ERR_ARG = 1
SEAM = ["h2g_debug_kate_division_dev", "h2g_debug_kate_tile_s"]


def test_seam_declared_bound_and_exported():
    declared = h2g.header_symbols()
    L = h2g.lib()
    for name in SEAM:
        assert name in declared, name
        assert name in h2g._SIGS, name
        assert hasattr(L, name), name
    assert h2g._SIGS["h2g_debug_kate_division_dev"][0][4:6] == [h2g.I32, h2g.I32]  # accumulate, tile_s
    # the entries they stand beside stay, and the ABI version with them
    for name in ("h2g_kate_division", "h2g_kate_division_dev"):
        assert name in declared and name in h2g._SIGS
    assert L.h2g_abi_version() == 1


@pytest.mark.parametrize("length,want", [(2050, 8), (2_093_057, 8), (2_093_058, 16), (4_186_113, 16),
                                         (4_186_114, 32)])
def test_rule_at_its_thresholds(length, want):
    assert h2g.debug_kate_tile_s(length) == want


@pytest.mark.parametrize("k,want", [(20, 8), (21, 16), (22, 32), (24, 32)])
def test_rule_at_circuit_sizes(k, want):
    """which proof size depends on which variant: k <= 20 on S = 8, k = 21 alone on S = 16,
    k >= 22 on S = 32"""
    assert h2g.debug_kate_tile_s(1 << k) == want


def test_rule_is_monotone_and_short_lengths_keep_the_shortest_tile():
    assert [h2g.debug_kate_tile_s(n) for n in (1, 2, 3, 2048, 2049)] == [8] * 5
    seen = [h2g.debug_kate_tile_s(n) for n in range(1 << 20, (1 << 23) + 1, 1 << 18)]
    assert seen == sorted(seen) and set(seen) == {8, 16, 32}
    assert h2g.debug_kate_tile_s(1 << 40) == 32  # never the default: arm (64)


def test_rule_argument_errors_need_no_device():
    s = ctypes.c_int(-1)
    assert h2g.lib().h2g_debug_kate_tile_s(0, ctypes.byref(s)) == ERR_ARG
    assert h2g.lib().h2g_debug_kate_tile_s(5, None) == ERR_ARG
    assert s.value == -1
