"""The entry points of the params' downsizing (h2g_g1_to_lagrange*, h2g_params_from_parts,
h2g_params_downsize) without a GPU: they are exported and bound, and before h2g_init each
refuses with H2G_ERR_STATE and names h2g_init in h2g_last_error()."""
import ctypes

import numpy as np
import pytest

import h2g

H2G_ERR_STATE = 4


def _calls():
    L = h2g.lib()
    g = np.zeros((4, 8), dtype=np.uint64)
    out = np.zeros((4, 8), dtype=np.uint64)
    h = ctypes.c_uint64()
    return {
        "h2g_g1_to_lagrange_dev": lambda: L.h2g_g1_to_lagrange_dev(g.ctypes.data, 2, out.ctypes.data, None),
        "h2g_g1_to_lagrange": lambda: L.h2g_g1_to_lagrange(h2g.p64(g), 2, h2g.p64(out)),
        "h2g_params_from_parts": lambda: L.h2g_params_from_parts(2, h2g.p64(g), None, None, None, ctypes.byref(h)),
        "h2g_params_downsize": lambda: L.h2g_params_downsize(1, 2, ctypes.byref(h)),
    }


@pytest.mark.parametrize("name", ["h2g_g1_to_lagrange_dev", "h2g_g1_to_lagrange", "h2g_params_from_parts",
                                  "h2g_params_downsize"])
def test_refused_before_init(name):
    assert not h2g._inited
    assert name in h2g._SIGS and name in h2g.header_symbols()
    assert _calls()[name]() == H2G_ERR_STATE
    assert "h2g_init" in h2g.lib().h2g_last_error().decode()


def test_python_surface():
    assert callable(h2g.Params.downsize) and callable(h2g.Params.from_parts)
    assert callable(h2g.g1_to_lagrange) and callable(h2g.g1_to_lagrange_dev)
    # from_parts is a constructor: bound to the class, not to an instance
    assert h2g.Params.from_parts.__self__ is h2g.Params
    for name in ("h2g_g1_to_lagrange_dev", "h2g_g1_to_lagrange", "h2g_params_from_parts", "h2g_params_downsize"):
        f = getattr(h2g.lib(), name)
        assert f.argtypes == h2g._SIGS[name][0] and f.restype is h2g._SIGS[name][1]
