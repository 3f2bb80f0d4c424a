"""GPU parity: libmgpoisson.so (HIP, gfx950) against the C oracle on identical inputs.

Bar: the kernels keep the reference's operation order with no fused
multiply-add and IEEE division, so psi must be BIT-IDENTICAL to the oracle in fp64 and fp32
after every piece and every cycle.  The only reduction, err = RMS update, is summed in a
different order on the GPU: tolerance |err_gpu - err_oracle| <= 1e-12 * err_oracle (fp64 sum).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle_lib import Oracle, coarse_coef, prolong_correct_arr, residual_arr, restrict_arr, smooth_arr  # noqa: E402

ERR_RTOL = 1e-12


def _check_err(e_gpu, e_oracle, psi_new, psi_old):
    """err = sqrt(sum (psi - psiOld)^2 / N) in fp64.  The GPU sums in a fixed tree order; the
    oracle sums sequentially, whose rounding grows ~N eps.  So: GPU vs a pairwise (numpy) sum of
    the same arrays at 1e-12, and GPU vs the oracle's own number at its summation bound."""
    d = psi_new.astype(np.float64) - psi_old.astype(np.float64)
    e_pw = float(np.sqrt(np.sum(d * d) / d.size))
    assert abs(e_gpu - e_pw) <= ERR_RTOL * abs(e_pw), (e_gpu, e_pw)
    assert abs(e_gpu - e_oracle) <= max(ERR_RTOL, 4 * d.size * 2.0 ** -53) * abs(e_oracle), (e_gpu, e_oracle)


def _mg():
    import mgpoisson

    return mgpoisson


def _ctx(**kw):
    mg = _mg()
    return mg.Context(mg.make_opts(**kw))


def _rand(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=shape).astype(dtype)


def _n3(dim, n):
    return (n, n, n if dim == 3 else 1)


REAL = {"double": np.float64, "float": np.float32}


@pytest.mark.parametrize("dim,n", [(2, 16), (2, 64), (3, 8), (3, 32)])
@pytest.mark.parametrize("real", ["double", "float"])
def test_init_point_charge(dim, n, real):
    ctx = _ctx(dim=dim, n=_n3(dim, n), real=real)
    ctx.init_point_charge()
    o = Oracle(dim=dim, n=_n3(dim, n), real=real)
    o.init_point_charge()
    assert np.array_equal(ctx.get_f(), o.get(1))
    assert np.array_equal(ctx.get_psi(), o.get(0))


@pytest.mark.parametrize("smoother", ["jacobi", "rbgs"])
@pytest.mark.parametrize("dim,n", [(2, 32), (2, 128), (3, 16), (3, 64)])
@pytest.mark.parametrize("real", ["double", "float"])
@pytest.mark.parametrize("level,bc", [(0, "zero"), (1, "consistent")])
def test_smoother_kernel(smoother, dim, n, real, level, bc):
    ctx = _ctx(dim=dim, n=_n3(dim, n), real=real, smoother=smoother, coarse_bc=bc)
    shp = ctx.shape(level)
    u = _rand(shp, REAL[real], 1)
    f = _rand(shp, REAL[real], 2)
    ctx.set_psi(u, level)
    ctx.set_f(f, level)
    ctx.smooth(level, 3)
    h = (2.0 ** level) / n
    ref = smooth_arr(dim, u, f, smoother, 3, h, coarse_coef(bc, level))
    assert np.array_equal(ctx.get_psi(level), ref)


@pytest.mark.parametrize("box", [(64, 64, 64), (128, 64, 32), (64, 128, 256), (256, 256, 8), (8, 4, 2), (4, 8, 16)])
@pytest.mark.parametrize("real", ["double", "float"])
@pytest.mark.parametrize("sweeps", [1, 2, 3])
@pytest.mark.parametrize("bc", ["zero", "consistent"])
def test_rbgs_sweep_shapes(box, real, sweeps, bc):
    """Red/black half-sweeps on the packed layout (vector and scalar kernels) equal in-place
    red/black sweeps of the oracle bit for bit, on cubes and boxes."""
    ctx = _ctx(dim=3, n=box, real=real, smoother="rbgs", coarse_bc=bc)
    for level in (0, 1):
        shp = ctx.shape(level)
        u = _rand(shp, REAL[real], 11 + level)
        f = _rand(shp, REAL[real], 12 + level)
        ctx.set_psi(u, level)
        ctx.set_f(f, level)
        ctx.smooth(level, sweeps)
        ref = smooth_arr(3, u, f, "rbgs", sweeps, (2.0 ** level) / box[0], coarse_coef(bc, level))
        assert np.array_equal(ctx.get_psi(level), ref), f"level {level}"


@pytest.mark.parametrize("dim,n", [(2, 32), (2, 256), (3, 16), (3, 64)])
@pytest.mark.parametrize("real", ["double", "float"])
@pytest.mark.parametrize("level,bc", [(0, "zero"), (1, "consistent"), (2, "zero")])
def test_residual_restrict_kernel(dim, n, real, level, bc):
    ctx = _ctx(dim=dim, n=_n3(dim, n), real=real, coarse_bc=bc)
    shp = ctx.shape(level)
    u = _rand(shp, REAL[real], 3)
    f = _rand(shp, REAL[real], 4)
    ctx.set_psi(u, level)
    ctx.set_f(f, level)
    ctx.residual_restrict(level)
    h = (2.0 ** level) / n
    ref = restrict_arr(dim, residual_arr(dim, u, f, h, coarse_coef(bc, level)))
    assert np.array_equal(ctx.get_f(level + 1), ref)


@pytest.mark.parametrize("prolong", ["pc", "linear"])
@pytest.mark.parametrize("dim,n", [(2, 8), (2, 16), (2, 32), (2, 128), (3, 16), (3, 32)])
@pytest.mark.parametrize("real", ["double", "float"])
@pytest.mark.parametrize("bc", ["zero", "consistent"])
def test_prolong_correct_kernel(prolong, dim, n, real, bc):
    """u += P V on level 0 == the oracle.  The small 2D levels launch fewer items than one workgroup of
    threads: the surplus threads must not repeat a row (round 3 fix: k_prolong_v let them through in 2D, and
    a repeat in another wave adds P V twice).  Applied three times, so a repeat is seen once it happens."""
    ctx = _ctx(dim=dim, n=_n3(dim, n), real=real, prolong=prolong, coarse_bc=bc)
    u = _rand(ctx.shape(0), REAL[real], 5)
    V = _rand(ctx.shape(1), REAL[real], 6)
    ctx.set_psi(u, 0)
    ctx.set_psi(V, 1)
    ref = u
    for _ in range(3):
        ctx.prolong_correct(0)
        ref = prolong_correct_arr(dim, ref, V, prolong, coarse_coef(bc, 1))
        assert np.array_equal(ctx.get_psi(0), ref)


CYCLE_CONFIGS = [
    # the reference cpu.lua path (config 1 family): 2D Jacobi 7+7 V, injection, ghost 0
    dict(dim=2, n=8, real="double", smoother="jacobi", coarse_init="fresh"),
    dict(dim=2, n=8, real="double", smoother="jacobi", coarse_init="warm"),
    dict(dim=2, n=64, real="double", smoother="jacobi"),
    dict(dim=2, n=256, real="double", smoother="jacobi"),
    dict(dim=2, n=256, real="float", smoother="jacobi"),
    # north-star smoother family (configs 2-5): red/black GS 2+2, linear, consistent coarse bc
    dict(dim=2, n=128, real="double", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent"),
    dict(dim=2, n=128, real="float", smoother="rbgs", nu1=2, nu2=2, cycle="F", prolong="linear", coarse_bc="consistent"),
    dict(dim=3, n=16, real="double", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent"),
    dict(dim=3, n=64, real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent"),
    dict(dim=3, n=32, real="double", smoother="rbgs", nu1=2, nu2=2, cycle="F", prolong="linear", coarse_bc="consistent"),
    dict(dim=3, n=32, real="double", smoother="jacobi", prolong="pc"),
    dict(dim=3, n=128, real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent"),
    dict(dim=3, n=128, real="double", smoother="rbgs", nu1=1, nu2=3, cycle="F", prolong="pc", coarse_bc="consistent"),
    dict(dim=3, n=64, real="float", smoother="rbgs", nu1=3, nu2=1, prolong="linear", coarse_bc="zero", coarse_init="warm"),
]


def _cfg_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


@pytest.mark.parametrize("cfg", CYCLE_CONFIGS, ids=_cfg_id)
def test_cycles_match_oracle(cfg):
    cfg = dict(cfg)
    dim, n = cfg.pop("dim"), cfg.pop("n")
    ctx = _ctx(dim=dim, n=_n3(dim, n), **cfg)
    o = Oracle(dim=dim, n=_n3(dim, n), **cfg)
    ctx.init_point_charge()
    o.init_point_charge()
    for it in range(4):
        old = o.get(0)
        e_gpu = ctx.cycle()
        e_ref = o.step()
        new = o.get(0)
        assert np.array_equal(ctx.get_psi(), new), f"psi differs after cycle {it + 1}"
        _check_err(e_gpu, e_ref, new, old)


@pytest.mark.parametrize("box", [(128, 64, 256), (64, 256, 128), (256, 128, 64)])
def test_cycles_box_match_oracle(box):
    kw = dict(dim=3, n=box, real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
    ctx = _ctx(**kw)
    o = Oracle(threads=8, **kw)
    ctx.init_point_charge()
    o.init_point_charge()
    for it in range(3):
        old = o.get(0)
        e_gpu, e_ref = ctx.cycle(), o.step()
        new = o.get(0)
        assert np.array_equal(ctx.get_psi(), new), f"psi differs after cycle {it + 1}"
        _check_err(e_gpu, e_ref, new, old)


@pytest.mark.parametrize("box", [(64, 16, 2), (64, 64, 64), (128, 32, 64), (256, 256, 32)])
@pytest.mark.parametrize("real", ["double", "float"])
@pytest.mark.parametrize("bc", ["zero", "consistent"])
def test_residual_restrict_tiled3d(box, real, bc):
    """mgp_residual_restrict on 3D levels 0 and 1 vs the oracle.  Every level here has fewer than 2^22 coarse cells
    (the largest, 256 x 256 x 32, has 2^18), so this runs the scalar form k_resrestrict_s (one thread per coarse
    cell); the pair and vector forms are test_gpu_switches.py's.  (The name is from an LDS-tiled kernel that no
    longer exists.)"""
    ctx = _ctx(dim=3, n=box, real=real, coarse_bc=bc)
    for level in (0, 1):
        shp = ctx.shape(level)
        if shp[0] < 2 or len(ctx.levels) <= level + 1:
            continue
        u = _rand(shp, REAL[real], 21 + level)
        f = _rand(shp, REAL[real], 22 + level)
        ctx.set_psi(u, level)
        ctx.set_f(f, level)
        ctx.residual_restrict(level)
        h = (2.0 ** level) / box[0]
        ref = restrict_arr(3, residual_arr(3, u, f, h, coarse_coef(bc, level)))
        assert np.array_equal(ctx.get_f(level + 1), ref), f"level {level}"


def test_cycles_batch_equals_single():
    """mgp_cycles(k) (one sync) == k x mgp_cycle, bit for bit, errs included."""
    kw = dict(dim=3, n=_n3(3, 32), real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
    a, b = _ctx(**kw), _ctx(**kw)
    a.init_point_charge()
    b.init_point_charge()
    ea = a.cycles(5)
    eb = np.array([b.cycle() for _ in range(5)])
    assert np.array_equal(a.get_psi(), b.get_psi())
    assert np.array_equal(ea, eb)


def test_graph_replay_equals_eager(monkeypatch):
    """hipGraph replay (default on one GPU) and eager launches give identical psi and err."""
    kw = dict(dim=3, n=_n3(3, 64), real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
    g = _ctx(**kw)
    monkeypatch.setenv("MGP_GRAPH", "0")
    e = _ctx(**kw)
    g.init_point_charge()
    e.init_point_charge()
    eg = np.concatenate([g.cycles(3), g.cycles(4)])
    ee = np.concatenate([e.cycles(3), e.cycles(4)])
    assert np.array_equal(g.get_psi(), e.get_psi())
    assert np.array_equal(eg, ee)


TAIL_CONFIGS = [
    dict(dim=3, n=64, real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent"),
    dict(dim=3, n=32, real="double", smoother="rbgs", nu1=2, nu2=2, cycle="F", prolong="linear", coarse_bc="consistent"),
    dict(dim=3, n=32, real="double", smoother="jacobi", prolong="pc"),
    dict(dim=3, n=(64, 32, 16), real="float", smoother="jacobi", nu1=3, nu2=2, cycle="F", prolong="linear",
         coarse_bc="consistent", coarse_init="warm"),
    dict(dim=2, n=256, real="double"),
    dict(dim=2, n=128, real="float", smoother="rbgs", nu1=2, nu2=2, cycle="F", prolong="linear", coarse_bc="consistent"),
    dict(dim=2, n=64, real="double", coarse_init="warm"),
]


@pytest.mark.parametrize("cfg", TAIL_CONFIGS, ids=_cfg_id)
def test_tail_equals_launch_per_piece(cfg, monkeypatch):
    """The one-launch LDS coarse tail (k_tail) == one launch per piece, on every level."""
    cfg = dict(cfg)
    dim, n = cfg.pop("dim"), cfg.pop("n")
    box = n if isinstance(n, tuple) else _n3(dim, n)
    a = _ctx(dim=dim, n=box, **cfg)
    monkeypatch.setenv("MGP_TAIL", "0")
    b = _ctx(dim=dim, n=box, **cfg)
    assert any(lv["tail"] for lv in a.levels) and not any(lv["tail"] for lv in b.levels)
    assert not a.levels[0]["tail"]
    a.init_point_charge()
    b.init_point_charge()
    for _ in range(3):
        assert a.cycle() == b.cycle()
    for level in range(len(a.levels)):
        assert np.array_equal(a.get_psi(level), b.get_psi(level)), f"psi level {level}"
        assert np.array_equal(a.get_f(level), b.get_f(level)), f"f level {level}"


# fp32 boxes 128 wide run POST's wide 128 x 16 tile on level 0 (wide="0": the 64 x 32 tile)
FUSED_CONFIGS = [
    dict(n=(128, 128, 128), real="float", prolong="linear", coarse_bc="consistent"),
    dict(n=(128, 128, 128), real="float", prolong="linear", coarse_bc="consistent", wide="0"),
    dict(n=(256, 64, 32), real="float", prolong="pc", coarse_bc="zero", err_mode=0),
    dict(n=(64, 64, 64), real="float", prolong="linear", coarse_bc="consistent", cycle="F"),
    dict(n=(128, 64, 32), real="double", prolong="pc", coarse_bc="zero"),
    dict(n=(64, 128, 64), real="double", prolong="linear", coarse_bc="consistent", coarse_init="warm"),
    dict(n=(64, 32, 128), real="float", prolong="pc", coarse_bc="consistent", err_mode=0),
    # instantiations of k_zs / k_zs_split_post that no other case launches: the narrow POST with injection and err on
    # level 0 and, on the fused cl != 0 level 1, without; the wide linear POST without err on k_zs and (every level
    # size on the stage-split kernel) on k_zs_split_post; fp64 level 1 with cl = 0 (the smoothing-only PRE before the
    # full weighting from a fresh guess, the linear POST without err) and with cl != 0 (POST with injection)
    dict(n=(128, 64, 64), real="float", prolong="pc", coarse_bc="consistent", wide="0"),
    dict(n=(128, 32, 32), real="float", prolong="linear", coarse_bc="consistent", err_mode=0),
    dict(n=(128, 32, 32), real="float", prolong="linear", coarse_bc="consistent", err_mode=0, split_post_min="0"),
    dict(n=(128, 64, 64), real="double", prolong="linear", coarse_bc="zero", restriction="full_weighting"),
    dict(n=(128, 64, 64), real="double", prolong="pc", coarse_bc="consistent"),
]


@pytest.mark.parametrize("cfg", FUSED_CONFIGS, ids=_cfg_id)
def test_fused_phases_match_oracle(cfg, monkeypatch):
    """Temporally blocked RB-GS 2+2 phases (k_fused, forced down to 64^3 here) vs one launch per
    half-sweep vs the C oracle: psi bit-identical on every level; err to summation order."""
    cfg = dict(cfg)
    monkeypatch.setenv("MGP_ZS_WIDE", cfg.pop("wide", "1"))
    if "split_post_min" in cfg:  # the smallest level (cells) that takes k_zs_split_post (default 2^27)
        monkeypatch.setenv("MGP_ZS_SPLIT_POST_MIN_CELLS", cfg.pop("split_post_min"))
    kw = dict(dim=3, smoother="rbgs", nu1=2, nu2=2, **cfg)
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", "65536")
    monkeypatch.setenv("MGP_FUSED", "1")
    a = _ctx(**kw)
    monkeypatch.setenv("MGP_FUSED", "0")
    b = _ctx(**kw)
    o = Oracle(threads=8, **{k: v for k, v in kw.items() if k != "err_mode"})
    for x in (a, b, o):
        x.init_point_charge()
    for it in range(3):
        old = o.get(0)
        ea, eb, eo = a.cycle(), b.cycle(), o.step()
        new = o.get(0)
        assert np.array_equal(a.get_psi(), new), f"fused psi differs after cycle {it + 1}"
        assert np.array_equal(b.get_psi(), new), f"unfused psi differs after cycle {it + 1}"
        if kw.get("err_mode", 1):
            _check_err(ea, eo, new, old)
            assert abs(ea - eb) <= 1e-12 * abs(eb)
    for level in range(len(a.levels)):
        assert np.array_equal(a.get_psi(level), b.get_psi(level)), f"psi level {level}"


@pytest.mark.parametrize("real", ["float", "double"])
def test_fused_level1_chunks_match_per_piece(real, monkeypatch):
    """k_zs on the 256^3 level of a 512^3 box (cl != 0, 32-plane z-chunks whose warm-up and drain steps run the
    steady path), both phases or POST alone (the default: PRE per piece): psi of every level bit-identical to
    one launch per piece after 2 cycles."""
    kw = dict(dim=3, n=(512, 512, 512), real=real, smoother="rbgs", nu1=2, nu2=2, prolong="linear",
              coarse_bc="consistent")
    runs = []
    for fmin, zmin, eng in ((1 << 24, 1 << 24, "zs"), (1 << 25, 1 << 24, "zpost"), (1 << 25, 1 << 40, "piece")):
        monkeypatch.setenv("MGP_FUSED_MIN_CELLS", str(fmin))
        monkeypatch.setenv("MGP_ZPOST_MIN_CELLS", str(zmin))
        a = _ctx(**kw)
        assert [lv["engine"] for lv in a.levels[:3]] == ["zs", eng, "piece"]
        a.init_point_charge()
        e = a.cycles(2)
        runs.append((e, [a.get_psi(l) for l in range(3)]))
        a.close()
    eb, pb = runs[-1]
    for e, p in runs[:-1]:
        for l in range(3):
            assert np.array_equal(p[l], pb[l]), f"level {l}"
        assert np.allclose(e, eb, rtol=1e-12, atol=0)


YS_CONFIGS = [
    dict(n=(1024, 1024, 1), real="float", prolong="linear", coarse_bc="consistent", half="0"),
    dict(n=(2048, 1024, 1), real="double", prolong="linear", coarse_bc="consistent", cycle="F"),
    dict(n=(1024, 2048, 1), real="float", prolong="pc", coarse_bc="zero", coarse_init="warm", half="0"),
    dict(n=(2048, 2048, 1), real="float", prolong="linear", coarse_bc="consistent", cycle="F", rows="16"),
    dict(n=(1024, 512, 1), real="double", prolong="linear", coarse_bc="zero", err_mode=0, half="0"),
    dict(n=(1024, 1024, 1), real="double", prolong="pc", coarse_bc="consistent", half="1"),
    # instantiations of k_ys that no other case launches.  fp32, cl = 0: POST without err on full-width segments
    # (injection; linear, after the smoothing-only PRE before the full weighting); POST with injection on half-width
    # segments, with err (level 0) and without (level 1)
    dict(n=(1024, 512, 1), real="float", prolong="pc", coarse_bc="zero", err_mode=0, half="0"),
    dict(n=(1024, 512, 1), real="float", prolong="linear", coarse_bc="consistent", restriction="full_weighting",
         err_mode=0, half="0"),
    dict(n=(1024, 512, 1), real="float", prolong="pc", coarse_bc="zero", half="1"),
    # fp32, cl != 0 (level 1): full-width segments (1024 of a 2048-wide box) with the average and injection, and with
    # the full weighting and linear prolongation; half-width segments with injection
    dict(n=(2048, 512, 1), real="float", prolong="pc", coarse_bc="consistent", half="0"),
    dict(n=(2048, 512, 1), real="float", prolong="linear", coarse_bc="consistent", restriction="full_weighting", half="0"),
    dict(n=(1024, 512, 1), real="float", prolong="pc", coarse_bc="consistent", half="1"),
    # fp64: POST with injection and no err on full-width (level 0) and half-width (level 1, cl = 0) segments; the
    # full weighting's PRE and the linear POST on full-width segments of level 0 (cl = 0) and level 1 (cl != 0)
    dict(n=(512, 512, 1), real="double", prolong="pc", coarse_bc="zero", err_mode=0, half="0"),
    dict(n=(512, 512, 1), real="double", prolong="pc", coarse_bc="zero", half="1"),
    dict(n=(1024, 512, 1), real="double", prolong="linear", coarse_bc="consistent", restriction="full_weighting", half="0"),
]


@pytest.mark.parametrize("cfg", YS_CONFIGS, ids=_cfg_id)
def test_ys_phases_match_oracle(cfg, monkeypatch):
    """2D temporally blocked RB-GS 2+2 phases (k_ys: rows streamed, forced down to 2^16 cells, full- and
    half-width segments) vs one launch
    per piece vs the C oracle: psi bit-identical on every level (the coarse 2D levels with cl != 0 included);
    err to summation order."""
    cfg = dict(cfg)
    rows = cfg.pop("rows", None)
    if rows:
        monkeypatch.setenv("MGP_YS_ROWS", rows)
    # segment width: full ("0"), half ("1"), or the default rule (half below 256 workgroups: every level of
    # these boxes)
    monkeypatch.setenv("MGP_YS_HALF", cfg.pop("half", "-1"))
    kw = dict(dim=2, smoother="rbgs", nu1=2, nu2=2, **cfg)
    monkeypatch.setenv("MGP_YS_MIN_CELLS", "65536")
    monkeypatch.setenv("MGP_FUSED", "1")
    a = _ctx(**kw)
    monkeypatch.setenv("MGP_FUSED", "0")
    b = _ctx(**kw)
    assert a.levels[0]["engine"] == "zs" and b.levels[0]["engine"] != "zs"
    o = Oracle(threads=8, **{k: v for k, v in kw.items() if k != "err_mode"})
    for x in (a, b, o):
        x.init_point_charge()
    for it in range(3):
        old = o.get(0)
        ea, eb, eo = a.cycle(), b.cycle(), o.step()
        new = o.get(0)
        assert np.array_equal(a.get_psi(), new), f"k_ys psi differs after cycle {it + 1}"
        assert np.array_equal(b.get_psi(), new), f"per-piece psi differs after cycle {it + 1}"
        if kw.get("err_mode", 1):
            _check_err(ea, eo, new, old)
            assert abs(ea - eb) <= 1e-12 * abs(eb)
    for level in range(len(a.levels)):
        assert np.array_equal(a.get_psi(level), b.get_psi(level)), f"psi level {level}"
        assert np.array_equal(a.get_f(level), b.get_f(level)), f"f level {level}"


def test_fused_timing_kinds(monkeypatch):
    """The bench's roofline window sees the fused level-0 kernels with their algorithmic bytes."""
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", "65536")
    monkeypatch.setenv("MGP_FUSED", "1")
    kw = dict(dim=3, n=(64, 64, 64), real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear",
              coarse_bc="consistent")
    a = _ctx(**kw)
    a.init_point_charge()
    a.timing(True)
    a.cycles(3)
    t = a.timing_read()
    a.timing(False)
    cells = 64 ** 3
    assert t["half_sweep"][1] == 0
    assert t["fused_pre"][1] == 3 and t["fused_post"][1] == 3
    # algorithmic reals per cell, as bench.py's roofline counts them: PRE reads u (black) and f and writes u
    # (black) and the 2^-d restricted residual; POST adds the correction (both colours) and reads psiOld for err
    assert t["fused_pre"][2] == 3 * (2.0 + 0.125) * 4 * cells
    assert t["fused_post"][2] == 3 * (2.5 + 0.125 + 1.0) * 4 * cells
    assert t["fused_pre"][0] > 0 and t["fused_post"][0] > 0


@pytest.mark.parametrize("kw", [
    dict(dim=3, n=(64, 64, 64), real="float", prolong="linear", coarse_bc="consistent"),
    dict(dim=3, n=(128, 64, 32), real="double", prolong="pc", cycle="F"),
    dict(dim=2, n=(256, 256, 1), real="float", prolong="linear", coarse_bc="consistent"),
    dict(dim=3, n=(128, 128, 128), real="float", prolong="linear", coarse_bc="consistent", fused=True),
    dict(dim=3, n=(128, 128, 64), real="double", prolong="pc", cycle="F", fused=True),
    dict(dim=3, n=(128, 128, 128), real="float", prolong="linear", coarse_bc="consistent", cycle="F",
         restriction="full_weighting", fused=True),
], ids=["3d-f32", "3d-F-f64", "2d-f32", "3d-fused-f32", "3d-fused-F-f64", "3d-fused-F-fw"])
def test_lazy_zero_equals_memset(kw, monkeypatch):
    """A fresh coarse guess read from the shared zero buffer by the first red half-sweep (no memset)
    == zeroing u with a memset, bit for bit, with the coarse tail on and off.  fused: levels 0 and 1 run
    k_zs, whose PRE on level 1 reads the pending zero as such (no loads) instead of a memset."""
    kw = dict(smoother="rbgs", nu1=2, nu2=2, **kw)
    if kw.pop("fused", False):
        monkeypatch.setenv("MGP_FUSED", "1")
        monkeypatch.setenv("MGP_FUSED_MIN_CELLS", "65536")
        monkeypatch.setenv("MGP_ZPOST_MIN_CELLS", str(1 << 40))
    for tail in ("1", "0"):
        monkeypatch.setenv("MGP_TAIL", tail)
        monkeypatch.setenv("MGP_LAZY_ZERO", "0")
        a = _ctx(**kw)
        monkeypatch.delenv("MGP_LAZY_ZERO")
        b = _ctx(**kw)
        a.init_point_charge()
        b.init_point_charge()
        ea, eb = a.cycles(3), b.cycles(3)
        assert np.array_equal(a.get_psi(), b.get_psi())
        assert list(ea) == list(eb)
        if os.environ.get("MGP_FUSED") == "1":
            assert [lv["engine"] for lv in b.levels][:2] == ["zs", "zs"], b.levels


@pytest.mark.parametrize("kw", [
    dict(real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent"),
    dict(real="double", smoother="jacobi", nu1=2, nu2=2, prolong="pc"),
], ids=["rbgs-f32", "jacobi-f64"])
def test_grid_stride_half_sweep_equals_one_shot(kw, monkeypatch):
    """The grid-stride half-sweep (opt-in, large levels: 256^3 here) == one item per thread."""
    monkeypatch.setenv("MGP_GS", "1")
    a = _ctx(dim=3, n=(256, 256, 256), **kw)
    monkeypatch.setenv("MGP_GS", "0")
    b = _ctx(dim=3, n=(256, 256, 256), **kw)
    a.init_point_charge()
    b.init_point_charge()
    ea, eb = a.cycles(2), b.cycles(2)
    assert np.array_equal(a.get_psi(), b.get_psi())
    np.testing.assert_allclose(ea, eb, rtol=1e-12, atol=0)


LOOPBACK_CASES = [
    # box, world, gather_cells, config
    ((64, 64, 128), 2, 4096, dict(real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")),
    ((64, 64, 128), 4, 4096, dict(real="double", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent",
                                  cycle="F")),
    ((32, 64, 64), 2, 512, dict(real="double", smoother="jacobi", nu1=3, nu2=3, prolong="pc", coarse_init="warm")),
    ((128, 64, 64), 8, 32768, dict(real="float", smoother="rbgs", nu1=2, nu2=2, prolong="pc", coarse_bc="zero")),
]


@pytest.mark.parametrize("box,world,gather,cfg", LOOPBACK_CASES, ids=["w2-rbgs-lin-f32", "w4-F-f64", "w2-jacobi-warm",
                                                                       "w8-rbgs-pc"])
def test_slab_decomposition_loopback(box, world, gather, cfg):
    """The library's multi-GPU code path (slab planes, ghost exchange after every half-sweep, coarse
    ghost planes for linear P, all-gather agglomeration, err all-reduce) with the loopback transport:
    `world` ranks on one GPU, one thread each.  Gathered psi == the single-domain run bit for bit."""
    _loopback_vs_single(box, world, gather, cfg)


FUSED_LOOPBACK_CASES = [
    # box, world, gather_cells, config: level 0 of every slab runs k_zs (>= 16 planes per rank)
    ((64, 64, 128), 2, 4096, dict(real="float", prolong="linear", coarse_bc="consistent")),
    ((64, 64, 128), 4, 65536, dict(real="double", prolong="linear", coarse_bc="consistent", cycle="F")),
    ((128, 64, 64), 2, 32768, dict(real="float", prolong="pc", coarse_bc="zero", coarse_init="warm")),
    ((64, 64, 128), 8, 4096, dict(real="float", prolong="linear", coarse_bc="consistent")),
]


@pytest.mark.parametrize("box,world,gather,cfg", FUSED_LOOPBACK_CASES,
                         ids=["w2-lin-f32", "w4-F-f64-gathered", "w2-pc-warm", "w8-lin-f32"])
def test_fused_slab_decomposition_loopback(box, world, gather, cfg, monkeypatch):
    """k_zs on slab-distributed levels: 5-plane halos of u and f before PRE, 4 before POST, 3 coarse
    planes of V, the restricted residual all-gathered when the coarse level is agglomerated.
    Gathered psi == the single-domain run bit for bit, and the level-0 phases ran fused."""
    monkeypatch.setenv("MGP_FUSED", "1")
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", "65536")
    _loopback_vs_single(box, world, gather, dict(smoother="rbgs", nu1=2, nu2=2, **cfg), expect_fused=True,
                        min_dist=1 if gather >= 65536 else 2)


def _loopback_run(box, world, gather, cfg, cycles=2):
    """Run `world` loopback ranks; returns (gathered psi, per-rank list of per-level exchange counts)."""
    import threading

    mg = _mg()
    lb = mg.Loopback(world)
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(dim=3, n=box, rank=r, world=world, gather_cells=gather, device=0,
                                          comm_id=b"\0" * 128, **cfg), loopback=lb)
            ctx.init_point_charge()
            ctx.cycles(cycles)
            ctx._read_levels()
            out[r] = (ctx.get_psi(), [lv["exchanges"] for lv in ctx.levels], [lv["distributed"] for lv in ctx.levels])
            ctx.close()
        except Exception as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    lb.close()
    assert not errors, errors
    return np.concatenate([out[r][0] for r in range(world)], axis=0), [out[r][1] for r in range(world)], out[0][2]


@pytest.mark.parametrize("world,real,cycle", [(2, "float", "V"), (4, "double", "F"), (8, "float", "V")])
def test_early_post_exchange_loopback(world, real, cycle, monkeypatch):
    """The u halo of a temporally blocked POST on slab levels goes out on the side stream right after PRE
    (overlapping the coarse levels) instead of just before POST.  Same exchanges, same psi bit for bit as the
    exchange-before-POST schedule (MGP_EARLY_X=0) and as the single domain."""
    box, gather = (64, 64, 256), 4096
    cfg = dict(real=real, smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent", cycle=cycle)
    monkeypatch.setenv("MGP_FUSED", "1")
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", "65536")
    monkeypatch.setenv("MGP_EARLY_X", "1")
    psi_e, ex_e, dist = _loopback_run(box, world, gather, cfg, cycles=3)
    monkeypatch.setenv("MGP_EARLY_X", "0")
    psi_l, ex_l, _ = _loopback_run(box, world, gather, cfg, cycles=3)
    assert dist[0]
    assert np.array_equal(psi_e, psi_l)
    assert ex_e == ex_l
    ref = _ctx(dim=3, n=box, gather_cells=gather, **cfg)
    ref.init_point_charge()
    ref.cycles(3)
    assert np.array_equal(psi_e, ref.get_psi())


@pytest.mark.parametrize("world,real", [(2, "float"), (4, "double")])
def test_deep_halo_smoothing_loopback(world, real, monkeypatch):
    """Deep-halo RB-GS on distributed levels below the finest (smooth_deep): one exchange of 2 nu + 1
    planes per smoothing phase instead of one per half-sweep.  psi is bit-identical to the exchanging
    schedule (MGP_DEEP_HALO=0) and to the single domain, with fewer exchanges on every such level."""
    box, gather = (64, 64, 128), 4096
    cfg = dict(real=real, smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
    monkeypatch.setenv("MGP_DEEP_HALO", "1")
    psi_d, ex_d, dist = _loopback_run(box, world, gather, cfg)
    monkeypatch.setenv("MGP_DEEP_HALO", "0")
    psi_s, ex_s, _ = _loopback_run(box, world, gather, cfg)
    assert np.array_equal(psi_d, psi_s)
    ref = _ctx(dim=3, n=box, gather_cells=gather, **cfg)
    ref.init_point_charge()
    ref.cycles(2)
    assert np.array_equal(psi_d, ref.get_psi())
    deep_levels = [l for l in range(1, len(dist)) if dist[l] and box[2] // world >> l >= 5]
    assert deep_levels, dist
    for l in deep_levels:
        assert ex_d[0][l] < ex_s[0][l], (l, ex_d[0], ex_s[0])
    assert sum(ex_d[0]) < sum(ex_s[0])


def _loopback_vs_single(box, world, gather, cfg, expect_fused=False, min_dist=2):
    import threading

    mg = _mg()
    lb = mg.Loopback(world)
    results, errors = [None] * world, []

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(dim=3, n=box, rank=r, world=world, gather_cells=gather, device=0,
                                          comm_id=b"\0" * 128, **cfg), loopback=lb)
            assert sum(lv["distributed"] for lv in ctx.levels) >= min_dist
            if min_dist == 1:  # level 0's coarse level is agglomerated
                assert ctx.levels[0]["distributed"] and not ctx.levels[1]["distributed"]
            ctx.init_point_charge()
            if expect_fused:
                ctx.timing(True)
            errs = ctx.cycles(3)
            if expect_fused:
                t = ctx.timing_read()
                ctx.timing(False)
                assert t["fused_pre"][1] == 3 and t["fused_post"][1] == 3 and t["half_sweep"][1] == 0, t
            # the temporally blocked phases overwrite psiOld, so mgp_metrics is unavailable there
            results[r] = (ctx.get_psi(), errs, None if expect_fused else ctx.metrics())
            ctx.close()
        except Exception as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    lb.close()
    assert not errors, errors
    ref = _ctx(dim=3, n=box, gather_cells=gather, **cfg)
    ref.init_point_charge()
    e_ref = ref.cycles(3)
    psi = np.concatenate([results[r][0] for r in range(world)], axis=0)
    assert np.array_equal(psi, ref.get_psi()), float(np.max(np.abs(psi - ref.get_psi())))
    for r in range(world):
        np.testing.assert_allclose(results[r][1], e_ref, rtol=1e-12, atol=0)
    if expect_fused:
        return
    m_ref = ref.metrics()
    for r in range(world):
        assert results[r][2][1] == m_ref[1]
        np.testing.assert_allclose(results[r][2], m_ref, rtol=1e-12, atol=0)


def _ref_metrics(psi, old):
    """gpu.lua:173-200 / test-gpu-obj.lua:216-247 restated in numpy (errorBuf in real, sums fp64)."""
    dt = psi.dtype.type
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where((old != 0) & (old != psi), np.abs(1.0 - (psi / old).astype(np.float64)).astype(psi.dtype), dt(0))
    nz = e != 0
    d = psi.astype(np.float64) - old.astype(np.float64)
    n = int(nz.sum())
    return float(e[nz].astype(np.float64).sum()) / n, n, float(np.sqrt((d * d).sum() / d.size))


@pytest.mark.parametrize("kw", [
    dict(dim=2, n=(64, 64, 1), real="double"),
    dict(dim=2, n=(128, 128, 1), real="float", smoother="rbgs", nu1=2, nu2=2),
    dict(dim=3, n=(64, 64, 64), real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent"),
], ids=["2d-jacobi-f64", "2d-rbgs-f32", "3d-rbgs-f32"])
def test_metrics_match_reference_formulas(kw):
    ctx = _ctx(**kw)
    ctx.init_point_charge()
    ctx.cycles(2)
    old = ctx.get_psi()
    e = ctx.cycle()
    rel, n, frob = ctx.metrics()
    r_rel, r_n, r_frob = _ref_metrics(ctx.get_psi(), old)
    assert n == r_n
    assert abs(rel - r_rel) <= 1e-12 * abs(r_rel)
    assert abs(frob - r_frob) <= 1e-12 * r_frob and abs(frob - e) <= 1e-12 * e


@pytest.mark.parametrize("real,cycle,dim", [("float", "V", 3), ("double", "F", 3), ("float", "V", 2)])
def test_metrics_under_temporally_blocked_finest_level(real, cycle, dim, monkeypatch):
    """k_zs on level 0 (forced down to 128^3): POST writes a buffer of its own, so psiOld survives the cycle and
    the reference's metrics (gpu.lua:173-200, test-gpu-obj.lua:222-243) and the psiOld / errorBuf fields
    (cpu-raw.lua:148-153) work on the north-star path; psi equals MGP_KEEP_PSI_OLD=0 (in place) bit for bit."""
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", "65536")
    monkeypatch.setenv("MGP_YS_MIN_CELLS", "65536")
    n = (128, 128, 128) if dim == 3 else (1024, 1024, 1)
    kw = dict(dim=dim, n=n, real=real, cycle=cycle, smoother="rbgs", nu1=2, nu2=2, prolong="linear",
              coarse_bc="consistent")
    ctx = _ctx(**kw)
    monkeypatch.setenv("MGP_KEEP_PSI_OLD", "0")
    inplace = _ctx(**kw)
    assert ctx.levels[0]["engine"] == "zs"
    mg = _mg()
    for x in (ctx, inplace):
        x.init_point_charge()
        x.cycles(2)
    old = ctx.get_psi()
    e, e2 = ctx.cycle(), inplace.cycle()
    assert e == e2 and np.array_equal(ctx.get_psi(), inplace.get_psi())
    rel, n, frob = ctx.metrics()
    r_rel, r_n, r_frob = _ref_metrics(ctx.get_psi(), old)
    assert n == r_n
    assert abs(rel - r_rel) <= 1e-12 * abs(r_rel)
    assert abs(frob - r_frob) <= 1e-12 * r_frob and abs(frob - e) <= 1e-12 * e
    assert np.array_equal(ctx.get_field(mg.FIELD_PSI_OLD), old)
    d = ctx.get_psi() - old
    assert np.array_equal(ctx.get_field(mg.FIELD_ERROR), d * d)
    with pytest.raises(mg.MGPError):
        inplace.metrics()
    # graph replay keeps the rotation: two more cycles, psiOld = the iterate before the last one
    ctx.cycles(1)
    old = ctx.get_psi()
    ctx.cycles(1)
    assert np.array_equal(ctx.get_field(mg.FIELD_PSI_OLD), old)


def test_metrics_need_err_mode():
    ctx = _ctx(dim=2, n=(16, 16, 1), err_mode=0)
    ctx.init_point_charge()
    ctx.cycle()
    with pytest.raises(_mg().MGPError):
        ctx.metrics()


def test_harness_bench_tsv(tmp_path):
    """test/test.lua's TSV: '#size<TAB>col' header, one row per size with the best run() time."""
    from mgpoisson import harness

    out = tmp_path / "cpu-vs-gpu.txt"
    rows = harness.bench(5, 7, tries=2, cols=("hip", "hip-rbgs"), out=str(out), quiet=True)
    lines = out.read_text().splitlines()
    assert lines[0] == "#size\thip\thip-rbgs"
    assert [int(l.split("\t")[0]) for l in lines[1:]] == [32, 64, 128]
    assert all(len(r) == 3 and all(t > 0 for t in r[1:]) for r in rows)


def test_harness_cpu_vs_gpu_columns(tmp_path):
    """test/test.lua's cpu-vs-gpu table: the C port of cpu-raw.lua plugged in as the 'cpu-raw' column beside the
    GPU's, both of the positional protocol's run() (two outer iterations)."""
    import harness_columns
    from mgpoisson import harness

    harness.register_column("cpu-raw", harness_columns.CpuRaw)
    out = tmp_path / "cpu-vs-gpu.txt"
    rows = harness.bench(5, 6, tries=1, cols=("cpu-raw", "hip"), out=str(out), quiet=True)
    assert out.read_text().splitlines()[0] == "#size\tcpu-raw\thip"
    assert all(len(r) == 3 and all(t > 0 for t in r[1:]) for r in rows)


def test_harness_converge_matches_cg(tmp_path):
    """converge-multigrid-vs-krylov.lua: multigrid and CG histories of |psi|_inf end at the same
    discrete solution (the converged values agree to 1e-8 relative)."""
    from mgpoisson import harness

    rep = harness.converge((8, 16), epsilon=1e-20, outdir=str(tmp_path), maxiter=200, quiet=True)
    for size, (mgh, cgh) in rep.items():
        assert len(mgh) > 3 and len(cgh) > 3
        assert abs(mgh[-1] - cgh[-1]) <= 1e-8 * abs(cgh[-1])
        assert (tmp_path / f"{size}.txt").exists()


def test_two_grid_host_buffers():
    """cpu-raw.lua:186 twoGrid(h, u, f, L) on caller buffers == the oracle's mgo_two_grid."""
    import ctypes

    from oracle_lib import lib as olib

    n = 32
    ctx = _ctx(dim=2, n=_n3(2, n), real="double", coarse_init="fresh")
    o = Oracle(dim=2, n=_n3(2, n), real="double")
    u = _rand((16, 16), np.float64, 7)
    f = _rand((16, 16), np.float64, 8)
    u_gpu = u.copy()
    ctx.two_grid(2.0 / n, u_gpu, f, 16)
    u_ref = u.copy()
    assert olib.mgo_two_grid(o.h, ctypes.c_double(2.0 / n), u_ref.ctypes.data, f.ctypes.data, 16) == 0
    assert np.array_equal(u_gpu, u_ref)


@pytest.mark.parametrize("kw", [
    dict(dim=2, n=(256, 256, 1), real="double"),
    dict(dim=3, n=(64, 64, 64), real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent"),
], ids=["2d-jacobi", "3d-rbgs"])
def test_coarse_level_switch_is_exact(kw):
    """cpuDepth's MI355X form: moving the coarse-engine switch changes nothing in the results."""
    runs = []
    for size in (0, 16, 8, 4):
        ctx = _ctx(**kw)
        ctx.set_coarse_level(size)
        if size:
            assert [lv["nx"] for lv in ctx.levels if lv["tail"]][0] == size or not any(lv["tail"] for lv in ctx.levels)
        ctx.init_point_charge()
        runs.append((ctx.cycles(3), ctx.get_psi()))
    for e, p in runs[1:]:
        assert np.array_equal(p, runs[0][1]) and np.array_equal(e, runs[0][0])


@pytest.mark.parametrize("real", ["double", "float"])
def test_every_level_per_piece_matches_oracle_on_reused_memory(real):
    """The reference cpu.lua configuration (2D 256^2 Jacobi 7+7, fresh coarse guess, err every cycle) with no
    coarse tail (set_coarse_level(0): every level down to 1x1 one launch per piece), on device memory a previous
    context of the same shape has just released: psi bit-identical to the oracle after every cycle.  (Round 3:
    the 2D prolongation's surplus threads repeated rows of the 4^2 .. 16^2 levels and added P V twice.)"""
    kw = dict(dim=2, n=(256, 256, 1), real=real)
    warm = _ctx(**kw)
    warm.init_point_charge()
    warm.cycles(3)
    warm.close()
    ctx = _ctx(**kw)
    ctx.set_coarse_level(0)
    assert not any(lv["tail"] for lv in ctx.levels)
    o = Oracle(**kw)
    ctx.init_point_charge()
    o.init_point_charge()
    for it in range(4):
        ctx.cycle()
        o.step()
        assert np.array_equal(ctx.get_psi(), o.get(0)), f"psi differs after cycle {it + 1}"


@pytest.mark.parametrize("init", ["fresh", "warm"])
def test_hybrid_handoff_to_reference_engine(init):
    """cpu-gpu.lua:17-52: the GPU runs the fine levels and hands level 16 (u, f) to another engine's
    twoGrid (here the C restatement of cpu-raw.lua's twoGrid) and back; psi == the all-GPU cycle."""
    import ctypes

    from oracle_lib import lib as olib

    kw = dict(dim=2, n=_n3(2, 64), real="double", coarse_init=init)
    a, b = _ctx(**kw), _ctx(**kw)
    o = Oracle(dim=2, n=_n3(2, 64), real="double", coarse_init=init)
    calls = []

    def engine(h, u, f, size):
        calls.append(size)
        assert olib.mgo_two_grid(o.h, ctypes.c_double(h), u.ctypes.data, f.ctypes.data, size) == 0

    a.set_coarse_handoff(16, engine)
    a.init_point_charge()
    b.init_point_charge()
    for _ in range(3):
        ea, eb = a.cycle(), b.cycle()
        assert np.array_equal(a.get_psi(), b.get_psi())
        assert abs(ea - eb) <= 1e-12 * abs(eb)
    assert calls == [16, 16, 16]
    a.set_coarse_handoff(16, None)
    a.cycle()


def test_solver_protocol_cpu_lua():
    """MultigridHIP{size,...}:solve() follows cpu.lua:208-216 and matches the oracle per step."""
    mg = _mg()
    seen = []
    s = mg.MultigridHIP(size=16, maxiter=5, errorCallback=lambda it, err: seen.append((it, err)) and False)
    s.solve()
    o = Oracle(dim=2, n=_n3(2, 16))
    o.init_point_charge()
    ref = [o.step() for _ in range(5)]
    assert [it for it, _ in seen] == [1, 2, 3, 4, 5]
    for (_, e), r in zip(seen, ref):
        assert abs(e - r) <= 1e-13 * r
    assert np.array_equal(s.psi, o.get(0))


def test_solver_protocol_break_rules():
    mg = _mg()
    s = mg.MultigridHIP({"size": 8, "maxiter": 50, "epsilon": 1e3})
    calls = []
    s.errorCallback = lambda it, err: calls.append(it) or (it == 3)
    s.solve()
    assert calls[-1] <= 3


def test_raw_protocol_run(capsys):
    mg = _mg()
    r = mg.MultigridHIPRaw(8)
    errs = r.run()
    out = capsys.readouterr().out.splitlines()
    assert out[0].split() == ["#iter", "err"]
    # cpu-raw semantics = warm persistent Vs; the survey's probe values at n = 8
    assert abs(errs[0] - 122091.06275197188) <= 1e-9 * 122091.0
    assert abs(errs[1] - 6828.1698388918103) <= 1e-9 * 6828.0


def test_fp32_close_to_fp64():
    kw = dict(dim=3, n=_n3(3, 64), smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
    a = _ctx(real="float", **kw)
    b = _ctx(real="double", **kw)
    a.init_point_charge()
    b.init_point_charge()
    a.cycles(10)
    b.cycles(10)
    pa, pb = a.get_psi().astype(np.float64), b.get_psi()
    rel = np.linalg.norm(pa - pb) / np.linalg.norm(pb)
    assert rel < 1e-5, rel


@pytest.mark.slow
def test_full_size_512_cube_one_cycle_bit_exact():
    """Config 3 at full size (3D 512^3 fp32, RB-GS 2+2 V, linear): psi bit-exact after 1 cycle."""
    kw = dict(dim=3, n=_n3(3, 512), real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
    ctx = _ctx(**kw)
    ctx.init_point_charge()
    e_gpu = ctx.cycle()
    o = Oracle(threads=16, **kw)
    o.init_point_charge()
    psi0 = o.get(0).astype(np.float64)
    e_ref = o.step()
    psi = ctx.get_psi()
    assert np.array_equal(psi, o.get(0))
    # At 1.3e8 cells the oracle's sequential fp64 sum carries ~1e-11 relative rounding; compare
    # the GPU's tree-summed err against numpy's pairwise sum instead (tolerance 1e-12) and the
    # oracle's within its own summation bound.
    d = psi.astype(np.float64) - psi0
    e_pairwise = float(np.sqrt(np.sum(d * d) / d.size))
    assert abs(e_gpu - e_pairwise) <= ERR_RTOL * e_pairwise
    assert abs(e_gpu - e_ref) <= 1e-9 * e_ref


def test_linearity_scaling_exact():
    """Size-independent property: every operation is linear and a x2 scaling is exact."""
    kw = dict(dim=3, n=_n3(3, 128), real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
    a, b = _ctx(**kw), _ctx(**kw)
    a.init_point_charge()
    b.set_f(2 * a.get_f())
    b.set_psi(2 * a.get_psi())
    a.cycles(3)
    b.cycles(3)
    assert np.array_equal(2 * a.get_psi(), b.get_psi())


def test_bad_options_fail_loudly():
    mg = _mg()
    with pytest.raises(mg.MGPError):
        mg.Context(mg.make_opts(dim=2, n=(12, 12, 1)))
