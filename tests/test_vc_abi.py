"""The variable-coefficient entry points of the C ABI (CPU): declared, exported, bound by ctypes and by hip.lua, and a
NULL context is MGP_ERR_ARG.  The ABI version and the size of mgp_opts are what they were."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mgp_set_coefficients", "mgp_clear_coefficients", "mgp_has_coefficients", "mgp_get_coefficients")
ERR_ARG = -1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_them():
    h = _read("include", "mgpoisson.h")
    for name in NAMES:
        assert re.search(r"^int\s+%s\(" % name, h, re.M), name
    assert re.search(r"^#define MGP_API_VERSION 3\b", h, re.M)
    assert "coefficient not positive and finite" in h


def test_library_exports_and_ctypes_binds_them():
    from mgpoisson import _lib as L

    for name in NAMES:
        fn = getattr(L.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, name
    assert L.lib.mgp_set_coefficients(None, None, None, None, L.MEM_HOST) == ERR_ARG
    assert L.lib.mgp_clear_coefficients(None) == ERR_ARG
    assert L.lib.mgp_has_coefficients(None) == ERR_ARG
    assert L.lib.mgp_get_coefficients(None, 0, 0, None, 0, L.MEM_HOST) == ERR_ARG
    assert L.lib.mgp_version() == 3
    assert ctypes.sizeof(L.MGPOpts) == 232 and L.default_opts().struct_size == 232


def test_python_layers_have_the_methods():
    import mgpoisson as mg

    for name in ("set_coefficients", "set_coefficients_ptr", "clear_coefficients", "has_coefficients", "get_coefficients"):
        assert callable(getattr(mg.Context, name)), name
    for name in ("setCoefficients", "clearCoefficients"):
        assert callable(getattr(mg.MultigridHIP, name)), name


def test_hip_lua_binds_and_calls_them():
    lua = _read("lua-multigrid-poisson_amd", "lua", "multigrid-poisson", "hip.lua")
    cdef = lua[lua.index("ffi.cdef"):]
    for name in NAMES:
        assert re.search(r"^int\s+%s\(" % name, cdef, re.M), name
        assert "lib.%s(" % name in lua, name
    for method in ("setCoefficients", "clearCoefficients", "getCoefficients"):
        assert "function MultigridHIP:%s(" % method in lua, method
