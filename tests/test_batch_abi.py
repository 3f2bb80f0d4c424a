"""Batched solves (mgp_batch_*): the C ABI, the host-only plan and the refusals.  No GPU needed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgpoisson.h")

ENTRY_POINTS = ["mgp_batch_create", "mgp_batch_destroy", "mgp_batch_last_error", "mgp_batch_size", "mgp_batch_plan",
                "mgp_batch_init_point_charge", "mgp_batch_set_field", "mgp_batch_get_field", "mgp_batch_cycles",
                "mgp_batch_solve", "mgp_batch_residual_norm", "mgp_batch_launches"]


def _mg():
    import mgpoisson

    return mgpoisson


def test_header_declares_and_library_exports():
    from mgpoisson import _lib

    text = open(HEADER).read()
    assert "typedef struct mgp_batch mgp_batch;" in text
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, text), f"{name} is not declared in mgpoisson.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libmgpoisson.so"
        assert name in _lib.SIGNATURES


def test_abi_version_and_opts_size_unchanged():
    from mgpoisson import _lib

    assert hasattr(_lib.lib, "mgp_batch_create")
    text = open(HEADER).read()
    assert re.search(r"#define MGP_API_VERSION 3\b", text)
    assert _lib.lib.mgp_version() == 3
    assert ctypes.sizeof(_lib.MGPOpts) == 232
    assert _lib.default_opts().struct_size == 232


def test_batch_plan_shapes():
    mg = _mg()
    o = mg.make_opts(dim=2, n=(256, 256))
    ref = mg.plan(o)
    p1 = mg.plan_batch(o, 1)
    p7 = mg.plan_batch(o, 7)
    assert p1 == p7
    assert [(d["nx"], d["ny"], d["nz"]) for d in p7] == [(d["nx"], d["ny"], d["nz_global"]) for d in ref]
    assert len(p7) == 9
    # the LDS engine takes the levels of <= 4096 cells, the ordinary context's coarse tail
    assert [d["engine"] for d in p7] == [d["engine"] if d["engine"] == "tail" else "piece" for d in ref]
    assert [d["engine"] for d in p7] == ["piece"] * 2 + ["tail"] * 7


@pytest.mark.parametrize("kw,batch,field", [
    (dict(), 0, "batch"),
    (dict(dim=3, n=(16, 16, 16), world=2), 2, "world"),
    (dict(smoother="gs_lex"), 2, "smoother"),
    (dict(real="float", arith="double"), 2, "arith"),
    (dict(restriction="full_weighting"), 2, "restriction"),
    (dict(dim=3, n=(512, 512, 512), real="float"), 2, "n"),
    (dict(n=(4096, 4096)), 128, "batch"),  # 2^24 cells x 128 = 2^31
])
def test_refusals_name_the_field(kw, batch, field):
    mg = _mg()
    o = mg.make_opts(**kw)
    for call in (lambda: mg.plan_batch(o, batch), lambda: mg.BatchContext(o, batch)):
        with pytest.raises(mg.MGPError) as ei:
            call()
        assert ei.value.code == -1  # MGP_ERR_ARG, before any device call
        assert re.search(r"\b%s\b" % field, str(ei.value)), str(ei.value)


def test_largest_accepted_member_and_batch():
    mg = _mg()
    assert len(mg.plan_batch(mg.make_opts(n=(4096, 4096)), 127)) == 13
    assert len(mg.plan_batch(mg.make_opts(dim=3, n=(256, 256, 256)), 127)) == 9


def test_batch_create_without_gpu_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    mg = _mg()
    with pytest.raises(mg.MGPError) as ei:
        mg.BatchContext(mg.make_opts(dim=2, n=(8, 8)), 2)
    assert "MGP_ERR_HIP" in str(ei.value)


def test_batch_solver_refuses_error_callback():
    mg = _mg()
    with pytest.raises(TypeError):
        mg.MultigridHIPBatch(size=8, batch=2, errorCallback=lambda it, err: False)
