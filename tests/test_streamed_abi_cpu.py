"""The streamed-coset key's additions to the C ABI are declared, bound and additive, and the
Python option is checked before the library is touched (no GPU, no library call)."""
import pytest

import h2g

NEW = ["h2g_keygen_opts", "h2g_pk_read_opts", "h2g_pk_memory", "h2g_coeff_to_subcoset"]


def test_new_symbols_declared_and_bound():
    declared = h2g.header_symbols()
    for name in NEW + ["h2g_coeff_to_subcoset_dev"]:
        assert name in declared, name
        assert name in h2g._SIGS, name
    # the functions they extend stay
    for name in ("h2g_keygen", "h2g_pk_read", "h2g_coeff_to_extended"):
        assert name in declared and name in h2g._SIGS


def test_options_struct_and_modes():
    import ctypes

    assert ctypes.sizeof(h2g.KeyOptions) == 8  # { uint32_t size; uint32_t cosets; }
    assert h2g.COSETS == {"resident": 0, "streamed": 1}
    text = open(h2g.HEADER).read()
    assert "H2G_COSETS_RESIDENT = 0" in text and "H2G_COSETS_STREAMED = 1" in text
    assert "typedef struct { uint32_t size; uint32_t cosets; } h2g_key_options;" in text


def test_abi_version_unchanged():
    L = h2g.lib()
    assert L.h2g_abi_version() == 1
    for name in NEW + ["h2g_coeff_to_subcoset_dev"]:
        assert hasattr(L, name), name


def test_unknown_coset_mode_raises_before_any_library_call(monkeypatch):
    def no_lib():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(h2g, "lib", no_lib)
    for bad in ("x", "", None, 1, "Streamed"):
        with pytest.raises(ValueError):
            h2g.ProvingKey(None, None, cosets=bad)
