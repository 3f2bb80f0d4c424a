"""The stage-split PRE kernel (k_zs_split: fp32, cl = 0, 2^3-average restriction) against k_zs and the C oracle.

k_zs_split divides k_zs's stages between two groups of waves and keeps every expression and its order, so the bar
is bit identity: psi and f of every level equal between MGP_ZS_SPLIT=1 (default) and MGP_ZS_SPLIT=0 (k_zs), and the
level-0 psi equal to the oracle's (the oracle exposes level 0 only).  PRE computes no err; the per-cycle err of
the two GPU paths must agree to 1e-12 relative (the existing tests' tolerance for a sum whose order may differ).

Shapes: the smallest at which the kernel can go wrong.  64 x 32 x 16 is one tile whose every face is a box face and
whose chunk is as short as fused_supported allows (warm-up and drain dominate, the extra step included; its 32768
cells lie below the 65536 the other cases force the fused phases down to, so this case forces them down to 32768);
64 x 32 x 64 has four 16-plane chunks (seams run the steady path's warm-up and drain); 128 x 64 x 32 has 2 x 2
tiles (interior tile faces, halo cells recomputed by both neighbours).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle_lib import Oracle  # noqa: E402

SPLIT_NAME = "k_zs_split<float, false>"
PARENT_NAME = "k_zs<float, true, 0, false, true, false>"
BASE = dict(dim=3, real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")


def _mg():
    import mgpoisson

    return mgpoisson


def _ctx(**kw):
    mg = _mg()
    return mg.Context(mg.make_opts(**kw))


def _pair(monkeypatch, kw, min_cells=65536):
    """Contexts on the split kernel and on k_zs (the setting is read once, at creation)."""
    monkeypatch.setenv("MGP_FUSED", "1")
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", str(min_cells))
    monkeypatch.setenv("MGP_ZS_SPLIT", "1")
    a = _ctx(**kw)
    monkeypatch.setenv("MGP_ZS_SPLIT", "0")
    b = _ctx(**kw)
    monkeypatch.delenv("MGP_ZS_SPLIT")
    assert a.levels[0]["engine"] == "zs" and b.levels[0]["engine"] == "zs"
    return a, b


def _run_pair(a, b, cycles):
    """Both contexts from the point charge; returns their errs.  Asserts which PRE kernel each launched."""
    for x in (a, b):
        x.init_point_charge()
        x.timing(True)
    ea = [a.cycle() for _ in range(cycles)]
    eb = [b.cycle() for _ in range(cycles)]
    na, nb = a.timing_kernels()["fused_pre"], b.timing_kernels()["fused_pre"]
    for x in (a, b):
        x.timing(False)
    assert na[0] == SPLIT_NAME and nb[0] == PARENT_NAME, (na, nb)
    assert na[1] // 768 == nb[1] // 448  # the same workgroups, 12 waves against 7
    return ea, eb


def _same_levels(a, b):
    for level in range(len(a.levels)):
        assert np.array_equal(a.get_psi(level), b.get_psi(level)), f"psi level {level}"
        assert np.array_equal(a.get_f(level), b.get_f(level)), f"f level {level}"


CASES = [
    ((64, 32, 16), dict()),
    ((64, 32, 64), dict()),
    ((128, 64, 32), dict()),
    ((64, 64, 64), dict(cycle="F")),
    ((64, 64, 64), dict(coarse_init="warm")),
]


@pytest.mark.parametrize("box,extra", CASES, ids=["one-tile-16", "one-tile-4-chunks", "2x2-tiles", "F-cycle", "warm"])
def test_split_equals_k_zs_and_oracle(box, extra, monkeypatch):
    kw = dict(BASE, n=box, **extra)
    a, b = _pair(monkeypatch, kw, min_cells=min(65536, box[0] * box[1] * box[2]))
    o = Oracle(threads=8, **{k: v for k, v in kw.items()})
    o.init_point_charge()
    ea, eb = _run_pair(a, b, 3)
    for _ in range(3):
        o.step()
    assert np.array_equal(a.get_psi(), o.get(0)), "split psi differs from the oracle"
    assert np.array_equal(b.get_psi(), o.get(0)), "k_zs psi differs from the oracle"
    _same_levels(a, b)
    np.testing.assert_allclose(ea, eb, rtol=1e-12, atol=0)


def test_split_fresh_zero_guess(monkeypatch):
    """coarse_bc = zero gives every level cl = 0, so the fused 64^3 level 1 of a 128^3 box runs the split kernel's
    fresh-zero-guess instantiation (no loads of u; the timing name covers level 0 only)."""
    kw = dict(BASE, n=(128, 128, 128), prolong="pc", coarse_bc="zero")
    a, b = _pair(monkeypatch, kw)
    assert [lv["engine"] for lv in a.levels[:2]] == ["zs", "zs"]
    o = Oracle(threads=8, **kw)
    o.init_point_charge()
    ea, eb = _run_pair(a, b, 2)
    for _ in range(2):
        o.step()
    assert np.array_equal(a.get_psi(), o.get(0))
    _same_levels(a, b)
    np.testing.assert_allclose(ea, eb, rtol=1e-12, atol=0)


def test_split_loopback_slabs(monkeypatch):
    """A world-2 split of 64^3 (ghost planes as the z-halo of every slab's level 0) == the single domain on either
    kernel, bit for bit."""
    from test_gpu_parity import _loopback_run

    kw = {k: v for k, v in BASE.items() if k != "dim"}
    monkeypatch.setenv("MGP_FUSED", "1")
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", "65536")
    psi, _, dist = _loopback_run((64, 64, 64), 2, 4096, kw, cycles=2)
    assert dist[0]
    a, b = _pair(monkeypatch, dict(BASE, n=(64, 64, 64), gather_cells=4096))
    _run_pair(a, b, 2)
    assert np.array_equal(psi, a.get_psi())
    assert np.array_equal(psi, b.get_psi())


def test_split_patch_order(monkeypatch):
    """MGP_ZS_PATCH_PRE: 2 x 2 patches of tiles.  The patch rule needs more than 512 workgroups: 512 x 512 x 128
    in 16-plane chunks has 1024 (MGP_ZS_WGS)."""
    monkeypatch.setenv("MGP_ZS_WGS", "1024")
    kw = dict(BASE, n=(512, 512, 128))
    a, b = _pair(monkeypatch, kw)
    monkeypatch.setenv("MGP_ZS_PATCH_PRE", "2,2")
    c = _ctx(**kw)
    c.init_point_charge()
    c.timing(True)
    c.cycle()
    name, grid = c.timing_kernels()["fused_pre"]
    c.timing(False)
    assert name == SPLIT_NAME and grid == 1024 * 768
    _run_pair(a, b, 1)
    assert np.array_equal(c.get_psi(), a.get_psi())
    _same_levels(a, b)
    assert np.array_equal(c.get_f(1), a.get_f(1))
