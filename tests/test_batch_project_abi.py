"""CPU: the entry points of the batched MAC-grid projection are in the header, the library, the ctypes binding, the
classes and hip.lua's cdef; a NULL batch is MGP_ERR_ARG; the ABI version and sizeof(mgp_opts) are unchanged."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgpoisson.h")
LIB = os.path.join(ROOT, "lua-multigrid-poisson_amd", "mgpoisson", "libmgpoisson.so")
LUA = os.path.join(ROOT, "lua-multigrid-poisson_amd", "lua", "multigrid-poisson", "hip.lua")
NAMES = ("mgp_batch_divergence", "mgp_batch_gradient", "mgp_batch_project")


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_declared_in_the_header(name):
    assert re.search(rf"\bint\s+{name}\s*\(\s*mgp_batch\s*\*", _code(HEADER)), name


def test_header_documents_the_scope():
    text = open(HEADER).read()
    assert "Limits: no batches" in text  # still true of mgp_divergence / mgp_gradient / mgp_project themselves
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+mgp_batch_divergence\s*\(", text, flags=re.S).group(1)
    for phrase in ("member slowest", "Out of scope", "per-member stop", "variable density", "cell-centred", "wall",
                   "debug scan", "div_before", "NULL face array", "unknown mem", "unknown op"):
        assert phrase in comment, phrase


def test_exported_by_the_library():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mgp_[a-z_0-9]+)$", out, flags=re.M))
    assert set(NAMES) <= exported, set(NAMES) - exported


def test_bound_in_ctypes_and_on_the_classes():
    import mgpoisson
    from mgpoisson import _lib

    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name).restype is _lib.SIGNATURES[name][0]
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [6, 7, 9]
    for meth in ("face_shapes", "divergence", "gradient", "project", "divergence_ptr", "gradient_ptr", "project_ptr"):
        assert callable(getattr(mgpoisson.BatchContext, meth)), meth
    for meth in ("divergence", "gradient", "project"):
        assert callable(getattr(mgpoisson.MultigridHIPBatch, meth)), meth


def test_declared_and_used_in_hip_lua():
    text = open(LUA).read()
    cdef = re.search(r"ffi\.cdef\s*\[\[(.*?)\]\]", text, flags=re.S).group(1)
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(\s*mgp_batch\s*\*", cdef), name
        assert f"lib.{name}(" in text, name
    assert "function MGBatch:divergence(vx, vy, vz, member)" in text
    assert "function MGBatch:gradient(vx, vy, vz, subtract, member)" in text
    assert "function MGBatch:project(vx, vy, vz, fmg, cycles)" in text


def test_null_batch_is_err_arg():
    from mgpoisson import _lib

    assert _lib.lib.mgp_batch_divergence(None, -1, None, None, None, 0) == -1
    assert _lib.lib.mgp_batch_gradient(None, -1, 1, None, None, None, 0) == -1
    assert _lib.lib.mgp_batch_project(None, None, None, None, 0, 1, 1, None, None) == -1


def test_abi_version_and_opts_size_unchanged():
    from mgpoisson import _lib

    hdr = open(HEADER).read()
    assert re.search(r"#define\s+MGP_API_VERSION\s+3\b", hdr)
    assert "_Static_assert(sizeof(mgp_opts) == 232" in hdr
    assert _lib.lib.mgp_version() == 3 and _lib.API_VERSION == 3
