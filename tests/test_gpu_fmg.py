"""GPU: the full multigrid start (mgp_fmg, mgp_fmg_restrict_rhs, mgp_fmg_prolong) against the host model of
fmg_model.py.

Fields are compared bit for bit (tobytes()) from dense random fields.  An err is a fixed-order fp64 sum on the device
and a sequential one in the oracle, so errs are held by test_gpu_parity._check_err, as everywhere else.  Under Neumann
f's mean is removed on the host first.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bc_model import mean_free  # noqa: E402
from dense_start import dense_fields  # noqa: E402
from fmg_model import FmgModel  # noqa: E402
from test_fmg_model import SETTINGS, _center, _problem  # noqa: E402
from test_gpu_bc import ALL_OFF  # noqa: E402
from test_gpu_dense import _env, _mg, _Run  # noqa: E402
from test_gpu_parity import _check_err  # noqa: E402

BCS = ("zero", "consistent", "face", "neumann")
RB = dict(smoother="rbgs", nu1=2, nu2=2)
RBL = dict(prolong="linear", **RB)
ERR_ARG, ERR_STATE = -1, -5


def _n3(box):
    return tuple(box) + (1,) * (3 - len(box))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _model(kw):
    return FmgModel(**{k: v for k, v in kw.items() if k != "device"})


def _fill_all_levels(ctx, m, seed):
    for l in range(m.nlev):
        u, f = dense_fields(m.shapes[l], m.dtype, seed + 2 * l)
        m.u[l], m.f[l] = u.copy(), f.copy()
        ctx.set_psi(u, l)
        ctx.set_f(f, l)


def _all_levels_equal(ctx, m, what):
    for l in range(m.nlev):
        assert _same(ctx.get_psi(l), m.u[l]), f"{what}: u of level {l}"
        assert _same(ctx.get_f(l), m.f[l]), f"{what}: f of level {l}"


def _pieces(ctx, m, seed):
    _fill_all_levels(ctx, m, seed)
    for l in range(m.nlev - 1):  # f down the hierarchy, each level from the one just written
        ctx.fmg_restrict_rhs(l)
        m.fmg_restrict_rhs(l)
        assert _same(ctx.get_f(l + 1), m.f[l + 1]), f"restriction of f from level {l} {m.shapes[l]}"
    _all_levels_equal(ctx, m, "after the restrictions")
    for l in range(m.nlev - 2, -1, -1):  # u up the hierarchy
        ctx.fmg_prolong(l)
        m.fmg_prolong(l)
        assert _same(ctx.get_psi(l), m.u[l]), f"prolongation onto level {l} {m.shapes[l]}"
    _all_levels_equal(ctx, m, "after the prolongations")


# ---- the pieces on every level ----

# (8,8): coarse nx 1, 2, 4 (scalar form); (16,4): a 4 x 1 coarsest level; (64,64): the 2D vector form; (8,8,8); (8,8,32):
# a 1 x 1 x 4 coarsest level; (64,32,16): the vector form over several workgroups, nx != ny != nz
BOXES = [(8, 8), (16, 4), (64, 64), (8, 8, 8), (8, 8, 32), (64, 32, 16)]


@pytest.mark.parametrize("restriction", ["average", "full_weighting"])
@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", BOXES, ids=lambda b: "x".join(map(str, b)))
def test_pieces_on_every_level(box, real, bc, restriction, monkeypatch):
    _env(monkeypatch, {})
    kw = dict(dim=len(box), n=_n3(box), real=real, coarse_bc=bc, restriction=restriction, **RBL)
    mg = _mg()
    ctx = mg.Context(mg.make_opts(**kw))
    _pieces(ctx, _model(kw), 300 + len(box))
    ctx.close()


def test_pieces_padded_plane_stride(monkeypatch):
    _env(monkeypatch, dict(MGP_PLANE_PAD=4352))
    kw = dict(dim=3, n=(256, 256, 8), real="float", coarse_bc="face", **RBL)
    mg = _mg()
    ctx = mg.Context(mg.make_opts(**kw))
    _pieces(ctx, _model(kw), 340)
    ctx.close()


@pytest.mark.parametrize("real,box", [("float", (256, 256, 128)), ("double", (256, 256, 64)), ("float", (2048, 2048)),
                                      ("double", (2048, 2048))], ids=["3d-f32", "3d-f64", "2d-f32", "2d-f64"])
def test_pieces_where_a_thread_marches(real, box, monkeypatch):
    """The smallest levels on which the vector prolongation gives a thread more than one coarse row of its column
    (2^17 threads at two rows each; 2D fp64: four): level 0 here, one row per thread on the levels below."""
    _env(monkeypatch, {})
    kw = dict(dim=len(box), n=_n3(box), real=real, coarse_bc="consistent", **RBL)
    mg = _mg()
    ctx = mg.Context(mg.make_opts(**kw))
    _pieces(ctx, _model(kw), 360)
    ctx.close()


def test_prolong_onto_a_pending_zero_and_level0_invalidates_psi_old(monkeypatch):
    """After a cycle level 1's u is whatever the cycle left; a prolongation onto it replaces every cell.  On level 0
    psiOld and the metrics are gone afterwards."""
    kw = dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="consistent", **RBL)
    r = _Run(monkeypatch, kw, {})
    m = _model(kw)
    psi0, f0 = dense_fields(m.shapes[0], m.dtype, 350)
    m.u[0], m.f[0] = psi0.copy(), f0.copy()
    r.ctx.set_psi(psi0)
    r.ctx.set_f(f0)
    r.cycle()
    m.cycles(1)
    r.ctx.metrics()
    for l in (1, 0):
        r.ctx.fmg_prolong(l)
        m.fmg_prolong(l)
    _all_levels_equal(r.ctx, m, "prolongations after a cycle")
    mg = _mg()
    with pytest.raises(mg.MGPError) as e:
        r.ctx.metrics()
    assert e.value.code == ERR_STATE
    with pytest.raises(mg.MGPError):
        r.ctx.get_field(mg.FIELD_PSI_OLD)


# ---- whole mgp_fmg ----

ZS = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=32768)
YS = dict(MGP_FUSED=1, MGP_YS_MIN_CELLS=65536)
JAC = dict(smoother="jacobi", nu1=7, nu2=7, prolong="pc")
# id -> (keywords, environment, cycles, final, {level: engine} asserted)
FMG = {
    "default-32^3-f32-face": (dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="face", **RBL), {}, 1, 1, {1: "tail"}),
    "default-64^2-f64-consistent-F-warm": (dict(dim=2, n=(64, 64, 1), real="double", coarse_bc="consistent", cycle="F",
                                                coarse_init="warm", **RBL), {}, 2, 2, {}),
    "default-16x4-f64-neumann": (dict(dim=2, n=(16, 4, 1), real="double", coarse_bc="neumann", **RBL), {}, 1, 1, {}),
    "default-8x8x32-f32-neumann": (dict(dim=3, n=(8, 8, 32), real="float", coarse_bc="neumann", **RBL), {}, 2, 1, {}),
    "alloff-32^3-f32-neumann": (dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="neumann", **RBL), ALL_OFF, 1, 2,
                                {l: "piece" for l in range(6)}),
    "alloff-64^2-f64-zero-warm-pc": (dict(dim=2, n=(64, 64, 1), real="double", coarse_bc="zero", coarse_init="warm",
                                          prolong="pc", **RB), ALL_OFF, 2, 1, {l: "piece" for l in range(7)}),
    "zs-64x32x16-f32-consistent": (dict(dim=3, n=(64, 32, 16), real="float", coarse_bc="consistent", **RBL), ZS, 1, 1,
                                   {0: "zs"}),
    "zs-64x32x16-f32-face-F-final0": (dict(dim=3, n=(64, 32, 16), real="float", coarse_bc="face", cycle="F", **RBL), ZS,
                                      2, 0, {0: "zs"}),
    "zs-64x32x16-f64-neumann-warm": (dict(dim=3, n=(64, 32, 16), real="double", coarse_bc="neumann",
                                          coarse_init="warm", **RBL), ZS, 1, 2, {0: "zs"}),
    "ys-256^2-f64-face": (dict(dim=2, n=(256, 256, 1), real="double", coarse_bc="face", **RBL), YS, 1, 2, {0: "zs"}),
    "ys-1024^2-f32-neumann": (dict(dim=2, n=(1024, 1024, 1), real="float", coarse_bc="neumann", **RBL), YS, 1, 1,
                              {0: "zs"}),
    "ys-256^2-f64-consistent-warm": (dict(dim=2, n=(256, 256, 1), real="double", coarse_bc="consistent",
                                          coarse_init="warm", **RBL), YS, 2, 1, {0: "zs"}),
    "blk-64x32x32-f64-pc-zero-F": (dict(dim=3, n=(64, 32, 32), real="double", prolong="pc", coarse_bc="zero", cycle="F",
                                        **RB), {}, 1, 1, {0: "piece", 1: "blk", 2: "tail"}),
    "tail-64^2-f32-zero": (dict(dim=2, n=(64, 64, 1), real="float", coarse_bc="zero", **RBL), {}, 2, 1, {}),
    "blk2-128^2-f32-face": (dict(dim=2, n=(128, 128, 1), real="float", coarse_bc="face", prolong="pc", **RB),
                            dict(MGP_TAIL_CELLS=512), 1, 1, {1: "blk", 2: "blk", 3: "tail"}),
    "graph0-32^3-f32-consistent": (dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="consistent", **RBL),
                                   dict(MGP_GRAPH=0), 1, 2, {}),
    "jacobi-64^2-f64": (dict(dim=2, n=(64, 64, 1), real="double", **JAC), {}, 1, 1, {}),
    "jacobi-64^2-f64-warm-face": (dict(dim=2, n=(64, 64, 1), real="double", coarse_init="warm", coarse_bc="face", **JAC),
                                  {}, 2, 2, {}),
    "fw-32^3-f32-face": (dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="face", restriction="full_weighting",
                              **RBL), {}, 1, 1, {}),
    "fw-64^2-f64-consistent-alloff": (dict(dim=2, n=(64, 64, 1), real="double", coarse_bc="consistent",
                                           restriction="full_weighting", **RBL), ALL_OFF, 1, 1, {}),
    "noerr-64x32x16-f32": (dict(dim=3, n=(64, 32, 16), real="float", coarse_bc="consistent", err_mode=0, **RBL), ZS, 1, 1,
                           {0: "zs"}),
}


def _start(run, kw, seed):
    """The model and the context with dense psi (which mgp_fmg ignores) and f on level 0."""
    m = _model(kw)
    psi0, f0 = dense_fields(m.shapes[0], m.dtype, seed)
    if kw.get("coarse_bc") == "neumann":
        f0 = mean_free(f0)
    m.u[0], m.f[0] = psi0.copy(), f0.copy()
    run.ctx.set_psi(psi0)
    run.ctx.set_f(f0)
    return m


def _fmg_both(run, m, cycles, final):
    _env(run.mp, run.env)
    errs = run.ctx.fmg(cycles, final)
    want = m.fmg(cycles, final)
    assert len(errs) == len(want) == final
    assert all(np.isfinite(a).all() for a in m.u)
    for i, (e, em) in enumerate(zip(errs, want)):
        old, new = m.cycle_log[i]
        print(f"final cycle {i + 1}: err {e!r} model {em!r}")
        if m.kw["err_mode"]:
            _check_err(e, em, new, old)
        else:
            assert np.isnan(e)
    return errs


@pytest.mark.parametrize("cid", sorted(FMG))
def test_fmg_against_the_model(cid, monkeypatch):
    kw, env, cycles, final, engines = FMG[cid]
    r = _Run(monkeypatch, kw, env)
    for l, e in engines.items():
        if l < len(r.levels):
            assert r.engines()[l] == e, r.engines()
    m = _start(r, kw, 400 + sorted(FMG).index(cid))
    _fmg_both(r, m, cycles, final)
    assert _same(r.ctx.get_psi(), m.u[0]), "psi"
    _all_levels_equal(r.ctx, m, cid)
    mg = _mg()
    if final and kw.get("err_mode", 1):
        assert _same(r.ctx.get_field(mg.FIELD_PSI_OLD), m.psi_old), "psiOld"
    else:
        with pytest.raises(mg.MGPError) as e:
            r.ctx.get_field(mg.FIELD_PSI_OLD)
        assert e.value.code == ERR_STATE


# ---- the state afterwards ----

@pytest.mark.parametrize("cid", ["default-32^3-f32-face", "zs-64x32x16-f32-consistent", "ys-256^2-f64-face",
                                 "jacobi-64^2-f64"])
def test_cycles_metrics_and_two_grid_afterwards(cid, monkeypatch):
    kw, env, cycles, _, _ = FMG[cid]
    r = _Run(monkeypatch, kw, env)
    m = _start(r, kw, 500)
    mg = _mg()
    # final = 0: psi is the ascent's, psiOld and the metrics are invalid until the next outer iteration
    _fmg_both(r, m, cycles, 0)
    assert _same(r.ctx.get_psi(), m.u[0])
    with pytest.raises(mg.MGPError) as e:
        r.ctx.metrics()
    assert e.value.code == ERR_STATE
    # ... which brings them back
    _env(monkeypatch, env)
    errs = r.ctx.cycles(2)
    want = m.cycles(2)
    assert _same(r.ctx.get_psi(), m.u[0]), "psi after mgp_cycles(2)"
    for i in range(2):
        _check_err(errs[i], want[i], m.cycle_log[i][1], m.cycle_log[i][0])
    assert _same(r.ctx.get_field(mg.FIELD_PSI_OLD), m.psi_old)
    got, ref = r.ctx.metrics(), m.metrics()
    assert got[1] == ref[1]
    assert abs(got[0] - ref[0]) <= 1e-12 * abs(ref[0]) and abs(got[2] - ref[2]) <= 1e-12 * abs(ref[2])
    # a second start from the same f, with final cycles: metrics and psiOld work at once
    _fmg_both(r, m, cycles, 1)
    assert _same(r.ctx.get_psi(), m.u[0])
    assert _same(r.ctx.get_field(mg.FIELD_PSI_OLD), m.psi_old)
    got, ref = r.ctx.metrics(), m.metrics()
    assert got[1] == ref[1] and abs(got[2] - ref[2]) <= 1e-12 * abs(ref[2])
    # twoGrid on caller arrays afterwards: its own result, psi / f / psiOld untouched
    u2, f2 = dense_fields(m.shapes[0], m.dtype, 510)
    h = 1.0 / kw["n"][0]
    want_u = m.two_grid(h, u2, f2, kw["n"][0])
    got_u = u2.copy()
    _env(monkeypatch, env)
    r.ctx.two_grid(h, got_u, f2, kw["n"][0])
    assert _same(got_u, want_u), "mgp_two_grid after mgp_fmg"
    assert _same(r.ctx.get_psi(), m.u[0]) and _same(r.ctx.get_f(), m.f[0])
    assert _same(r.ctx.get_field(mg.FIELD_PSI_OLD), m.psi_old)


def test_debug_scans_the_pieces(monkeypatch):
    kw = dict(dim=3, n=(16, 16, 16), real="float", coarse_bc="face", **RBL)
    r = _Run(monkeypatch, kw, {})
    m = _start(r, kw, 520)
    mg = _mg()
    r.ctx.set_debug(1)
    _fmg_both(r, m, 1, 1)  # finite fields: no complaint, same bits
    assert _same(r.ctx.get_psi(), m.u[0])
    f = m.f[0].copy()
    f[3, 5, 7] = np.nan
    r.ctx.set_f(f)
    with pytest.raises(mg.MGPError) as e:
        r.ctx.fmg_restrict_rhs(0)
    assert "found a nan" in str(e.value) and "right-hand-side restriction" in str(e.value), str(e.value)
    with pytest.raises(mg.MGPError) as e:
        r.ctx.fmg(1, 0)
    assert "found a nan" in str(e.value) and "FMG" in str(e.value), str(e.value)
    r.ctx.set_debug(0)


# ---- refusals ----

def _refused(mg, code, fn, *a):
    with pytest.raises(mg.MGPError) as e:
        fn(*a)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_refuses_bad_arguments_and_arith_double(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=2, n=(32, 32, 1), real="float", **RBL)
    ctx = mg.Context(mg.make_opts(**kw))
    m = _model(kw)
    psi0, f0 = dense_fields(m.shapes[0], m.dtype, 530)
    ctx.set_psi(psi0)
    ctx.set_f(f0)
    for c, f in ((0, 1), (-1, 1), (1, -1)):
        _refused(mg, ERR_ARG, ctx.fmg, c, f)
    for l in (-1, m.nlev - 1, m.nlev):
        _refused(mg, ERR_ARG, ctx.fmg_restrict_rhs, l)
        _refused(mg, ERR_ARG, ctx.fmg_prolong, l)
    assert _same(ctx.get_psi(), psi0) and _same(ctx.get_f(), f0)  # nothing ran
    ctx.close()
    raw = mg.Context(mg.make_opts(arith="double", **kw))
    _refused(mg, ERR_ARG, raw.fmg, 1, 1)
    _refused(mg, ERR_ARG, raw.fmg_restrict_rhs, 0)
    _refused(mg, ERR_ARG, raw.fmg_prolong, 0)
    raw.close()


def test_refuses_refinement_and_handoff(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=2, n=(32, 32, 1), real="float", **RBL)
    ctx = mg.Context(mg.make_opts(**kw))
    m = _model(kw)
    psi0, f0 = dense_fields(m.shapes[0], m.dtype, 540)
    m.u[0], m.f[0] = psi0.copy(), f0.copy()
    ctx.set_psi(psi0)
    ctx.set_f(f0)
    ctx.refine_begin()
    for fn, a in ((ctx.fmg, (1, 1)), (ctx.fmg_restrict_rhs, (0,)), (ctx.fmg_prolong, (0,))):
        _refused(mg, ERR_STATE, fn, *a)
    ctx.refine_end()
    ctx.set_coarse_handoff(8, lambda h, u, f, n: None)
    assert "hand-off" in _refused(mg, ERR_STATE, ctx.fmg, 1, 1)
    ctx.set_coarse_handoff(0, None)
    # and afterwards it runs
    errs = ctx.fmg(1, 1)
    want = m.fmg(1, 1)
    assert _same(ctx.get_psi(), m.u[0])
    _check_err(errs[0], want[0], m.cycle_log[0][1], m.cycle_log[0][0])
    ctx.close()


def test_refuses_loopback_ranks(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="face", **RBL)
    world = 2
    lb = mg.Loopback(world)
    codes, errors = [None] * world, []

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(rank=r, world=world, gather_cells=512, device=0, comm_id=b"\0" * 128, **kw),
                             loopback=lb)
            got = []
            for fn, a in ((ctx.fmg, (1, 1)), (ctx.fmg_restrict_rhs, (0,)), (ctx.fmg_prolong, (0,))):
                try:
                    fn(*a)
                    got.append(0)
                except mg.MGPError as e:
                    got.append((e.code, "single-GPU contexts only" in str(e)))
            codes[r] = got
            ctx.close()
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    lb.close()
    assert not errors, errors
    assert codes == [[(ERR_STATE, True)] * 3] * world, codes


# ---- accuracy on the device, through the solver class ----

@pytest.mark.parametrize("real,bc", [("double", "face"), ("float", "neumann")])
def test_fmg_criterion_on_the_device(real, bc, monkeypatch):
    """alg/disc <= 1 after MultigridHIP.fmg(1, 1) at 32^3 (test_fmg_model.py's criterion and problems; the converged
    discrete solution is the fp64 host model's).  Under Neumann the class removes f's mean first and psi's after."""
    _env(monkeypatch, {})
    mg = _mg()
    n, dim = 32, 3
    f, exact = _problem(bc, dim, n)
    s = mg.MultigridHIP(size=n, dim=dim, real=real, smoother="rbgs", smooth=2, prolong="linear", boundary=bc)
    s.psi = np.ones_like(f)  # ignored
    s.f = f
    err = s.fmg(1, 1)
    assert np.isfinite(err)
    got = s.psi.astype(np.float64)
    if bc == "neumann":
        assert abs(got.sum() / got.size) <= 1e-6 * np.abs(got).max()
    c = FmgModel(dim=dim, n=(n, n, n), coarse_bc=bc, **SETTINGS)
    c.f[0] = f.copy()
    for _ in range(80):
        if c.cycles(1)[0] <= 1e-14 * np.abs(c.u[0]).max():
            break
    conv = _center(c.u[0], bc)
    alg = np.abs(_center(got, bc) - conv).max()
    disc = np.abs(conv - _center(exact, bc)).max()
    print(f"{bc} {real} 32^3 on the device: alg/disc = {alg / disc:.4f} (algebraic {alg:.3e}, discretisation {disc:.3e})")
    assert alg / disc <= 1.0
    with pytest.raises(ValueError, match="mixed"):
        mg.MultigridHIP(size=16, dim=2, real="mixed", smoother="rbgs", smooth=2).fmg()
