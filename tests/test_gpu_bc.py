"""GPU: the box boundaries MGP_BC_FACE (u = 0 on the face, cl = +1 on every level) and MGP_BC_NEUMANN (du/dn = 0,
cl = -1) on every engine, against the host model of bc_model.py, and mgp_remove_mean.

Level 0 carries a boundary-modified operator here for the first time, and the one-cell level is singular under
Neumann (its diagonal is 0: relaxed to +0).  Cases start from dense_start's fields (under Neumann f's mean is removed
on the host first).  Where nothing else is stated a case checks
  - psi bit-identical to the model after each of 3 cycles, err by test_gpu_parity._check_err;
  - u and f of every level bit-identical to the run with every engine switched off (and that run's to the model's).
"""
import math
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abi_model as A  # noqa: E402
from bc_model import BcModel, mean_free  # noqa: E402
from dense_start import dense_fields  # noqa: E402
from test_gpu_dense import SWITCHES, _env, _mg, _Run  # noqa: E402
from test_gpu_dense_fw import _check_err_raw  # noqa: E402
from test_gpu_parity import _check_err  # noqa: E402

BCS = ("face", "neumann")
RB = dict(smoother="rbgs", nu1=2, nu2=2)
RBL = dict(prolong="linear", **RB)
ALL_OFF = dict(MGP_FUSED=0, MGP_BLK=0, MGP_BLK2=0, MGP_BRES=0, MGP_TAIL=0, MGP_FRESH=0, MGP_RESFW=0)


def _n3(box):
    return tuple(box) + (1,) * (3 - len(box))


def _start(kw, seed):
    """(model, psi0, f0): dense fields, f mean-free under Neumann."""
    m = BcModel(**{k: v for k, v in kw.items() if k != "device"})
    psi0, f0 = dense_fields(m.shapes[0], m.dtype, seed)
    if kw["coarse_bc"] == "neumann":
        f0 = mean_free(f0)
    m.u[0], m.f[0] = psi0.copy(), f0.copy()
    return m, psi0, f0


def _compare(kw, seed, runs, cycles=3):
    """runs: the engines under test first, the all-off run last.  Returns the model after `cycles` cycles."""
    m, psi0, f0 = _start(kw, seed)
    for r in runs:
        r.ctx.set_psi(psi0)
        r.ctx.set_f(f0)
    for it in range(cycles):
        em = m.cycles(1)[0]
        old, new = m.cycle_log[0]
        assert np.isfinite(new).all()
        for i, r in enumerate(runs):
            e = r.cycle()
            r.errs.append(e)
            assert np.array_equal(r.ctx.get_psi(), new), f"run {i} {r.env}: psi differs after cycle {it + 1}"
            if kw.get("err_mode", 1):
                print(f"run {i} cycle {it + 1}: err {e!r} model {em!r}")
                (_check_err_raw if m.arith == "double" else _check_err)(e, em, new, old)
            else:
                assert math.isnan(e)
    ref = runs[-1].ctx
    for l in range(m.nlev):
        assert np.array_equal(ref.get_psi(l), m.u[l]), f"all-off run: u of level {l} differs from the model's"
        assert np.array_equal(ref.get_f(l), m.f[l]), f"all-off run: f of level {l} differs from the model's"
        for i, r in enumerate(runs[:-1]):
            assert np.array_equal(r.ctx.get_psi(l), ref.get_psi(l)), f"run {i} {r.env}: u of level {l}"
            assert np.array_equal(r.ctx.get_f(l), ref.get_f(l)), f"run {i} {r.env}: f of level {l}"
    return m


def _one_cell_is_plus_zero(ctx, m):
    if m.u[-1].size == 1:
        assert ctx.get_psi(m.nlev - 1).tobytes() == np.zeros(1, m.dtype).tobytes()


# ---- per-piece and the tail (the singular cell inside the LDS tail by default) ----

@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("real", ["double", "float"])
@pytest.mark.parametrize("box", [(8, 8), (16, 4), (8, 8, 8), (8, 8, 32)], ids=lambda b: "x".join(map(str, b)))
@pytest.mark.parametrize("tail", [0, None], ids=["tail0", "tail"])
def test_pieces_and_tail(bc, real, box, tail, monkeypatch):
    kw = dict(dim=len(box), n=_n3(box), real=real, coarse_bc=bc, **RBL)
    a = _Run(monkeypatch, kw, {} if tail is None else dict(MGP_TAIL=0))
    p = _Run(monkeypatch, kw, ALL_OFF)
    assert ("tail" in a.engines()) == (tail is None), a.engines()
    assert set(p.engines()) == {"piece"}
    m = _compare(kw, 11, [a, p])
    if bc == "neumann":
        _one_cell_is_plus_zero(a.ctx, m)
        _one_cell_is_plus_zero(p.ctx, m)


# ---- the options matrix ----

OPTIONS = {
    "jacobi-7+7": dict(real="double", smoother="jacobi", nu1=7, nu2=7, prolong="linear"),
    "gs_lex": dict(real="double", smoother="gs_lex", nu1=2, nu2=2, prolong="linear"),
    "arith-double": dict(real="float", arith="double", **RBL),
    "full-weighting": dict(real="float", restriction="full_weighting", **RBL),
    "F-cycle": dict(real="float", cycle="F", **RBL),
    "warm": dict(real="double", coarse_init="warm", **RBL),
    "pc": dict(real="float", prolong="pc", **RB),
}


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("box", [(16, 16, 16), (32, 32)], ids=["16^3", "32^2"])
@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_options(bc, box, opt, monkeypatch):
    kw = dict(dim=len(box), n=_n3(box), coarse_bc=bc, **OPTIONS[opt])
    a = _Run(monkeypatch, kw, {})
    p = _Run(monkeypatch, kw, ALL_OFF)
    m = _compare(kw, 21, [a, p])
    if bc == "neumann":
        _one_cell_is_plus_zero(a.ctx, m)


# ---- k_zs on level 0 with cl != 0 ----

def _args(name):
    return [s.strip() for s in name[name.index("<") + 1:name.rindex(">")].split(",")]


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("real,box,min_cells", [("float", (64, 32, 16), 32768), ("float", (128, 64, 32), 65536),
                                                ("double", (128, 64, 32), 65536)],
                         ids=["f32-one-tile", "f32-2x2-tiles", "f64"])
@pytest.mark.parametrize("err_mode", [1, 0])
def test_k_zs_level0_boundary_modified(bc, real, box, min_cells, err_mode, monkeypatch):
    kw = dict(dim=3, n=box, real=real, coarse_bc=bc, err_mode=err_mode, **RBL)
    a = _Run(monkeypatch, kw, dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=min_cells))
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert a.engines()[0] == "zs" and "zs" not in p.engines()
    m = _compare(kw, 31, [a, p])
    # one more cycle under mgp_timing: one PRE and one POST launch, no half-sweeps, on k_zs with CLZ = false
    em = m.cycles(1)[0]
    old, new = m.cycle_log[0]
    e, t, k = a.timed_cycle()
    assert np.array_equal(a.ctx.get_psi(), new)
    assert t["fused_pre"][1] == 1 and t["fused_post"][1] == 1 and t["half_sweep"][1] == 0, t
    for kind, pre in (("fused_pre", "true"), ("fused_post", "false")):
        name = k[kind][0]
        assert name.startswith("k_zs<"), k
        args = _args(name)  # <T, PRE, LINEAR, ERR, CLZ, WIDE>
        assert args[0] == real and args[1] == pre and args[4] == "false", k
    assert _args(k["fused_post"][0])[3] == ("true" if err_mode else "false"), k
    mg = _mg()
    if err_mode:
        _check_err(e, em, new, old)
        assert np.array_equal(a.ctx.get_field(mg.FIELD_PSI_OLD), m.psi_old)
        got, want = a.ctx.metrics(), m.metrics()
        assert got[1] == want[1]
        assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]) and abs(got[2] - want[2]) <= 1e-12 * abs(want[2])
    else:
        with pytest.raises(mg.MGPError):
            a.ctx.metrics()


# ---- two fused levels: zs + zpost with the stage-split cl PRE ----

@pytest.mark.parametrize("bc", BCS)
def test_two_fused_levels_zpost(bc, monkeypatch):
    kw = dict(dim=3, n=(128, 128, 128), real="float", coarse_bc=bc, **RBL)
    z = _Run(monkeypatch, kw, dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=1 << 21, MGP_ZPOST_MIN_CELLS=1 << 18))
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert z.engines()[:2] == ["zs", "zpost"], z.levels
    assert not {"zs", "zpost"} & set(p.engines())
    _compare(kw, 41, [z, p])


# ---- k_ys ----

@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("real", ["float", "double"])
def test_k_ys(bc, real, monkeypatch):
    kw = dict(dim=2, n=(1024, 1024, 1), real=real, coarse_bc=bc, **RBL)
    a = _Run(monkeypatch, kw, dict(MGP_FUSED=1, MGP_YS_MIN_CELLS=65536))
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert a.engines()[0] == "zs" and "zs" not in p.engines()
    m = _compare(kw, 51, [a, p])
    m.cycles(1)
    _, t, k = a.timed_cycle()
    assert np.array_equal(a.ctx.get_psi(), m.u[0])
    assert t["fused_pre"][1] == 1 and t["fused_post"][1] == 1 and t["half_sweep"][1] == 0, t
    assert k["fused_pre"][0].startswith("k_ys<") and k["fused_post"][0].startswith("k_ys<"), k


# ---- the default engines below the finest level (k_blk, k_blk2, k_bres, k_fresh, k_tail_c) ----

@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("box", [(64, 64, 64), (512, 512)], ids=["64^3", "512^2"])
def test_default_engines_against_everything_off(bc, box, monkeypatch):
    kw = dict(dim=len(box), n=_n3(box), real="float", coarse_bc=bc, **RBL)
    a = _Run(monkeypatch, kw, {})
    p = _Run(monkeypatch, kw, ALL_OFF)
    assert {"blk", "tail"} <= set(a.engines()), a.engines()
    assert set(p.engines()) == {"piece"}
    m = _compare(kw, 61, [a, p])
    if bc == "neumann":
        _one_cell_is_plus_zero(a.ctx, m)


# ---- slabs: world 2 through the loopback transport ----

def _slab_run(mg, kw, world, gather, psi0, f0, cycles):
    lb = mg.Loopback(world)
    res, errors = [None] * world, []

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(rank=r, world=world, gather_cells=gather, device=0, comm_id=b"\0" * 128, **kw),
                             loopback=lb)
            lv = ctx.levels[0]
            z = slice(lv["z0"], lv["z0"] + lv["nz_local"])
            ctx.set_planes(mg.FIELD_U, 0, psi0[z])
            ctx.set_planes(mg.FIELD_F, 0, f0[z])
            ctx.comm_log(reset=True)
            errs = list(ctx.cycles(cycles))
            res[r] = dict(psi=ctx.get_psi(), z=z, errs=errs, log=ctx.comm_log(), engines=[x["engine"] for x in ctx.levels],
                          dist=[x["distributed"] for x in ctx.levels])
            ctx.close()
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    lb.close()
    assert not errors, errors
    return res


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("box,env,gather", [((32, 32, 32), dict(MGP_FUSED=0), 512),
                                            ((64, 32, 64), dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536), 4096)],
                         ids=["32^3", "64x32x64-fused"])
def test_slabs_equal_one_domain(bc, box, env, gather, monkeypatch):
    for k in SWITCHES + ("MGP_DEEP_HALO",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    mg = _mg()
    kw = dict(dim=3, n=box, real="float", coarse_bc=bc, **RBL)
    m, psi0, f0 = _start(kw, 71)
    cycles = 3
    res = _slab_run(mg, kw, 2, gather, psi0, f0, cycles)
    one = mg.Context(mg.make_opts(**kw))
    one.set_psi(psi0)
    one.set_f(f0)
    e1 = list(one.cycles(cycles))
    m.cycles(cycles)
    psi = one.get_psi()
    assert np.array_equal(psi, m.u[0])
    assert res[0]["dist"][0] and res[0]["engines"][0] == ("zs" if env["MGP_FUSED"] else "piece"), res[0]
    for r in res:
        assert np.array_equal(r["psi"], psi[r["z"]])
        assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(r["errs"], e1)), (r["errs"], e1)
    plan = mg.plan_comm(mg.make_opts(rank=0, world=2, gather_cells=gather, comm_id=b"\0" * 128, **kw), cycles)
    assert res[0]["log"] == res[1]["log"] == plan and plan


# ---- batch ----

@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("kw", [dict(dim=2, n=(32, 32, 1), real="double", smoother="jacobi", nu1=7, nu2=7, prolong="linear"),
                                dict(dim=3, n=(16, 16, 16), real="float", **RBL)], ids=["32^2-jacobi-f64", "16^3-rbgs-f32"])
def test_batch_members_equal_the_context(bc, kw, monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(kw, coarse_bc=bc)
    B = 3
    b = mg.BatchContext(mg.make_opts(**kw), B)
    starts = [_start(kw, 81 + 10 * i) for i in range(B)]
    for i, (_, psi0, f0) in enumerate(starts):
        b.set_psi(psi0, member=i)
        b.set_f(f0, member=i)
    errs = b.cycles(3)
    for i, (m, psi0, f0) in enumerate(starts):
        c = mg.Context(mg.make_opts(**kw))
        c.set_psi(psi0)
        c.set_f(f0)
        ec = c.cycles(3)
        m.cycles(3)
        assert np.array_equal(c.get_psi(), m.u[0])
        assert np.array_equal(b.get_psi(member=i), c.get_psi()), f"member {i}"
        for l in range(m.nlev):
            assert np.array_equal(b.get_field(mg.FIELD_U, member=i, level=l), m.u[l]), (i, l)
            assert np.array_equal(b.get_field(mg.FIELD_F, member=i, level=l), m.f[l]), (i, l)
        assert all(abs(errs[k, i] - ec[k]) <= 1e-12 * abs(ec[k]) for k in range(3)), (errs[:, i], ec)


@pytest.mark.parametrize("bc", BCS)
def test_batch_solve_stops_each_member_on_its_own(bc, monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=3, n=(16, 16, 16), real="double", coarse_bc=bc, **RBL)
    B = 3
    b = mg.BatchContext(mg.make_opts(**kw), B)
    starts = [_start(kw, 91 + 10 * i) for i in range(B)]
    scale = [1.0, 1e-4, 1e4]  # members whose err passes epsilon after different numbers of cycles
    for i, (m, psi0, f0) in enumerate(starts):
        b.set_psi(psi0 * scale[i], member=i)
        b.set_f(f0 * scale[i], member=i)
    eps, maxiter = 1e-6, 30
    iters, last = b.solve(eps, maxiter)
    assert len(set(iters.tolist())) > 1, iters
    for i, (m, psi0, f0) in enumerate(starts):
        m.u[0], m.f[0] = psi0 * scale[i], f0 * scale[i]
        n = 0
        while n < maxiter:
            e = m.cycles(1)[0]
            n += 1
            if e < eps or not math.isfinite(e):
                break
        assert iters[i] == n, (i, iters, n)
        assert np.array_equal(b.get_psi(member=i), m.u[0]), f"member {i}"


# ---- refinement ----

@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("box", [(16, 16, 16), (32, 32)], ids=["16^3", "32^2"])
def test_refinement_matches_the_model_and_converges(bc, box, monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=len(box), n=_n3(box), real="float", coarse_bc=bc, **RBL)
    m = BcModel(**kw)
    c = mg.Context(mg.make_opts(**kw))
    rng = np.random.default_rng(101)
    psi64 = rng.uniform(-1, 1, m.shapes[0])
    f64 = rng.uniform(-1, 1, m.shapes[0])
    if bc == "neumann":
        f64 = f64 - f64.mean()
        f64 = f64 - f64.mean()
    c.refine_begin()
    m.refine_begin()
    for which, a in ((A.REFINE_PSI, psi64), (A.REFINE_F, f64)):
        c.refine_set(which, a)
        m.refine_set(which, a)
    rel = []
    for step in range(12):
        got, want = c.refine_step(2), m.refine_step(2)
        assert np.array_equal(c.refine_get(A.REFINE_PSI), m.psi64), f"step {step + 1}"
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-12 * abs(w), (step, got, want)
        rel.append(got[0] / got[1])
    rn, fn = c.refine_residual()
    rel.append(rn / fn)
    print(bc, box, ["%.2e" % r for r in rel])
    assert min(rel) <= 1e-12, rel
    c.refine_end()


# ---- CG ----

def test_cg_agrees_with_converged_multigrid_under_face(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=3, n=(16, 16, 16), real="double", coarse_bc="face", **RBL)
    c = mg.Context(mg.make_opts(**kw))
    _, psi0, f0 = _start(kw, 111)
    c.set_psi(psi0)
    c.set_f(f0)
    x, it, err = c.cg_solve(epsilon=1e-28, maxiter=4000)
    c.cycles(40)
    psi = c.get_psi()
    rn, fn = c.residual_norm()
    assert rn <= 1e-12 * fn
    assert np.abs(x - psi).max() <= 1e-9 * np.abs(psi).max(), (it, err)


def test_cg_runs_to_a_finite_result_under_neumann(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=3, n=(16, 16, 16), real="double", coarse_bc="neumann", **RBL)
    c = mg.Context(mg.make_opts(**kw))
    _, psi0, f0 = _start(kw, 121)
    c.set_psi(psi0)
    c.set_f(f0)
    x, it, err = c.cg_solve(epsilon=1e-20, maxiter=200)
    assert np.isfinite(x).all() and math.isfinite(err) and it >= 1


# ---- remove_mean ----

def _check_mean(before, after, mean):
    d = before.astype(np.float64)
    exact = math.fsum(d.ravel().tolist()) / d.size
    bound = d.size * 2.0 ** -53 * float(np.abs(d).mean())
    print(f"mean {mean!r} exact {exact!r} bound {bound:.3e}")
    assert abs(mean - exact) <= bound, (mean, exact, bound)
    assert np.array_equal(after, (d - mean).astype(before.dtype))


def _metrics_refused(mg, c):
    with pytest.raises(mg.MGPError) as ei:
        c.metrics()
    assert ei.value.code == A.ERR_STATE


@pytest.mark.parametrize("bc", ["zero", "face", "neumann"])
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", [(16, 16, 16), (32, 32)], ids=["16^3", "32^2"])
def test_remove_mean_every_level(bc, real, box, monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=len(box), n=_n3(box), real=real, coarse_bc=bc, **RBL)
    c = mg.Context(mg.make_opts(**kw))
    dt = c.dtype
    c.set_psi(A.dense(c.shape(0), dt, 5))
    c.set_f(A.dense(c.shape(0), dt, 6))
    c.cycle()
    c.metrics()
    for l in range(len(c.levels)):
        for which, seed in ((mg.FIELD_U, 131), (mg.FIELD_F, 132)):
            a = (A.dense(c.shape(l), dt, seed + l) + dt.type(0.25)).astype(dt)
            c.set_field(which, a, l)
            mean = c.remove_mean(l, which)
            _check_mean(a, c.get_field(which, l), mean)
            if l == 0:
                _metrics_refused(mg, c)
    e = c.cycle()  # the next outer iteration brings psiOld and the metrics back
    assert math.isfinite(e)
    c.metrics()


def test_remove_mean_padded_layout(monkeypatch):
    """Level 0's planes hold 2^16 slots, so MGP_PLANE_PAD makes its plane stride 2 H + 4352 / sizeof(real) (and every
    buffer starts at its default MGP_PAD_BYTES offset): the pad slots between the planes are neither summed nor
    written."""
    _env(monkeypatch, dict(MGP_PLANE_PAD=4352))
    mg = _mg()
    kw = dict(dim=3, n=(256, 256, 16), real="float", coarse_bc="neumann", **RBL)
    c = mg.Context(mg.make_opts(**kw))
    m, psi0, f0 = _start(kw, 141)
    a = (psi0 + np.float32(0.5)).astype(np.float32)
    c.set_psi(a)
    c.set_f(f0)
    m.u[0] = a.copy()
    mean = c.remove_mean(0, mg.FIELD_U)
    _check_mean(a, c.get_psi(), mean)
    m.remove_mean(0, A.U, mean)
    assert np.array_equal(c.get_psi(), m.u[0])
    c.cycles(2)  # (a pad slot that was written would enter the next cycles' stencils)
    m.cycles(2)
    assert np.array_equal(c.get_psi(), m.u[0])


@pytest.mark.parametrize("level", [0, 2])
def test_remove_mean_loopback_world_2(level, monkeypatch):
    _env(monkeypatch, dict(MGP_FUSED=0))
    mg = _mg()
    kw = dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="neumann", **RBL)
    world = 2
    shape = (32 >> level,) * 3
    a = (A.dense(shape, np.float32, 151) + np.float32(0.5)).astype(np.float32)
    lb = mg.Loopback(world)
    res, errors = [None] * world, []

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(rank=r, world=world, gather_cells=4096, device=0, comm_id=b"\0" * 128, **kw),
                             loopback=lb)
            lv = ctx.levels[level]
            z = slice(lv["z0"], lv["z0"] + lv["nz_local"]) if lv["distributed"] else slice(None)
            ctx.set_planes(mg.FIELD_F, 0, a[z], level)
            mean = ctx.remove_mean(level, mg.FIELD_F)
            res[r] = (z, mean, ctx.get_field(mg.FIELD_F, level), lv["distributed"])
            ctx.close()
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    lb.close()
    assert not errors, errors
    assert res[0][3] == (level == 0)
    assert res[0][1] == res[1][1]
    got = np.concatenate([res[0][2], res[1][2]]) if level == 0 else res[0][2]
    _check_mean(a, got, res[0][1])
    if level != 0:
        assert np.array_equal(res[1][2], res[0][2])


def test_remove_mean_group(monkeypatch):
    """mgp_group_remove_mean: two ranks of one process (sharing the GPU through the loopback transport), the global
    field in and out; a distributed level (0) and a replicated one."""
    _env(monkeypatch, dict(MGP_FUSED=0))
    mg = _mg()
    g = mg.Group(mg.make_opts(dim=3, n=(32, 32, 32), real="double", coarse_bc="neumann", gather_cells=4096, **RBL), 2,
                 devices=[0, 0])
    dist = [lv["distributed"] for lv in g.ranks[0].levels]
    assert dist[0] and not dist[2]
    for level in (0, 2):
        a = A.dense(g.shape(level), np.float64, 181 + level) + 0.4
        g.set_field(mg.FIELD_F, a, level)
        mean = g.remove_mean(level, mg.FIELD_F)
        _check_mean(a, g.get_field(mg.FIELD_F, level), mean)
    g.close()


def test_remove_mean_batch(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=3, n=(16, 16, 16), real="float", coarse_bc="neumann", **RBL)
    B = 3
    b = mg.BatchContext(mg.make_opts(**kw), B)
    for level in (0, 2, 4):
        shape = (16 >> level,) * 3
        a = [(A.dense(shape, np.float32, 161 + i) + np.float32(0.1 * (i + 1))).astype(np.float32) for i in range(B)]
        for i in range(B):
            b.set_field(mg.FIELD_F, a[i], member=i, level=level)
        means = b.remove_mean(level, mg.FIELD_F)
        for i in range(B):
            _check_mean(a[i], b.get_field(mg.FIELD_F, member=i, level=level), float(means[i]))


def test_remove_mean_refine(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=3, n=(16, 16, 16), real="float", coarse_bc="neumann", **RBL)
    c = mg.Context(mg.make_opts(**kw))
    with pytest.raises(mg.MGPError) as ei:
        c.refine_remove_mean(A.REFINE_F)
    assert ei.value.code == A.ERR_STATE
    c.refine_begin()
    with pytest.raises(mg.MGPError) as ei:
        c.remove_mean(0, mg.FIELD_F)
    assert ei.value.code == A.ERR_STATE
    for which, seed in ((A.REFINE_PSI, 171), (A.REFINE_F, 172)):
        a = np.random.default_rng(seed).uniform(-1, 1, c.shape(0)) + 0.3
        c.refine_set(which, a)
        mean = c.refine_remove_mean(which)
        _check_mean(a, c.refine_get(which), mean)
    a1 = (A.dense(c.shape(1), np.float32, 173) + np.float32(0.2)).astype(np.float32)
    c.set_field(mg.FIELD_U, a1, 1)  # the levels below stay ordinary
    mean1 = c.remove_mean(1, mg.FIELD_U)
    _check_mean(a1, c.get_field(mg.FIELD_U, 1), mean1)
    c.refine_end()


# ---- random call sequences of three existing configurations, replayed under each boundary ----

@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("cid", ["zs-64x32x16", "blk-bres-64x32x32-f64-F", "gslex-64"])
def test_sequences_under_the_new_boundaries(bc, cid, monkeypatch):
    import test_gpu_sequences as S

    ops = A.sequence(cid, A.SEEDS[0])
    kw, env, engines = A.CONFIGS[cid]
    monkeypatch.setitem(A.CONFIGS, cid, (dict(kw, coarse_bc=bc), env, engines))
    monkeypatch.setattr(A, "Model", BcModel)
    p = S._replay(monkeypatch, cid, ops, A.SEEDS[0])
    print(f"{cid} {bc}: engines {p.engines}; ops {dict(sorted(p.counts.items()))}")


# ---- the solver classes ----

def test_solver_class_neumann_solve(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    s = mg.MultigridHIP(size=32, boundary="neumann", smoother="rbgs", smooth=2, prolong="linear", maxiter=40)
    s.solve()
    psi = s.psi
    assert abs(psi.astype(np.float64).mean()) <= 32 * 32 * 2.0 ** -53 * np.abs(psi).mean() + np.abs(psi).max() * 2.0 ** -52
    m = BcModel(dim=2, n=(32, 32, 1), real="double", prolong="linear", coarse_bc="neumann", **RB)
    f = np.zeros((32, 32))
    f[16, 16] = -1e6
    m.u[0], m.f[0] = -f, mean_free(f)
    for _ in range(40):
        if m.cycles(1)[0] < s.epsilon:
            break
    rm, fm = m.residual_norm(0)
    rn, fn = s.ctx.residual_norm()
    print("residual", rn / fn, "model", rm / fm)
    # "as small as the model's": both runs stop by the same rule at the rounding floor of r = f - A psi, where f (its
    # mean removed by sums of different order) and psi (a constant apart, which A annihilates up to rounding) differ
    # in their last bits, so the two residuals are two samples of the same rounding noise: within a factor of 2
    assert rn / fn <= 2.0 * rm / fm
    with pytest.raises(ValueError):
        mg.MultigridHIP(size=32, boundary="face", coarse_bc="consistent")
    sb = mg.MultigridHIPBatch(size=16, batch=2, boundary="neumann", smoother="rbgs", smooth=2, prolong="linear", maxiter=30)
    sb.solve()
    assert np.abs(sb.psi.reshape(2, -1).astype(np.float64).mean(axis=1)).max() <= 1e-10 * np.abs(sb.psi).max()
