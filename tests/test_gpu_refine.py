"""GPU: mixed-precision defect correction (mgp_refine_*), through the C ABI via mgpoisson.Context.

fp64 psi / f, r = f - A psi in double, a few of the context's fp32 cycles on A e = r from e = 0, psi += e in double:
the outer loop of cpu.lua:196-216 with real = 'double' around float cycles.  The reference side is restated here
from tests/oracle_lib.py: residual_arr in double, Oracle(real='float').two_grid for the inner cycles.  Bars: the
defect kernel and every outer step are bit-exact against that restatement on every engine; the norms agree to the
project's 1e-12 (summation order differs); the iteration reaches the double solver's answer, which a plain float
context cannot (stated per test)."""
import functools

import numpy as np
import pytest

from oracle_lib import Oracle, residual_arr

pytestmark = pytest.mark.gpu

RB = dict(smoother="rbgs", nu1=2, nu2=2, prolong="linear")


def _mg():
    import mgpoisson

    return mgpoisson


def _shape(kw):
    n = kw["n"]
    return (n[2], n[1], n[0]) if kw["dim"] == 3 else (n[1], n[0])


def _ctx(kw, begin=True):
    mg = _mg()
    ctx = mg.Context(mg.make_opts(real="float", **kw))
    if begin:
        ctx.refine_begin()
    return ctx


def _point_charge(kw):
    """cpu.lua:180-193 in double: f = -1e6 at (n/2, n/2[, n/2]), psi = -f."""
    f = np.zeros(_shape(kw))
    f[tuple(s // 2 for s in f.shape)] = -1e6
    return -f, f


def _random(kw, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, _shape(kw)), rng.uniform(-1.0, 1.0, _shape(kw))


# ---- 1. the defect kernel -------------------------------------------------------------------------------------------

# (nx, ny[, nz]).  Rows of one or two cells take the scalar form, of >= 4 cells the 16-byte form, and from 2^20
# two-cell items the grid-stride form: 3D 128^3 sits exactly on that threshold and 2D 512 x 512 below it, so 2D
# 2048 x 1024 is added above it; 1 x 8, 2 x 16 and 2 x 8 x 4 are scalar-form rows with neighbours in y / z.
DEFECT_2D = [(1, 1), (2, 2), (4, 4), (8, 8), (64, 16), (32, 32), (512, 512), (1, 8), (2, 16), (2048, 1024)]
DEFECT_3D = [(2, 2, 2), (4, 4, 4), (8, 8, 32), (32, 16, 8), (16, 16, 16), (128, 128, 128), (2, 8, 4)]


@pytest.mark.parametrize("n", DEFECT_2D + DEFECT_3D, ids=lambda n: "x".join(map(str, n)))
def test_defect_matches_the_double_residual(n):
    mg = _mg()
    dim = len(n)
    kw = dict(dim=dim, n=tuple(n) + (1,) * (3 - dim), **RB)
    psi, f = _random(kw, seed=sum(n))
    ctx = _ctx(kw)
    ctx.refine_set(mg._lib.REFINE_PSI, psi)
    ctx.refine_set(mg._lib.REFINE_F, f)
    rn, fn = ctx.refine_residual()
    r = residual_arr(dim, psi, f, 1.0 / n[0])
    assert r.dtype == np.float64
    got = ctx.get_f()
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), r.astype(np.float32).view(np.uint32))
    print(f"defect {n}: rnorm {rn!r} vs {np.sqrt(np.sum(r * r))!r}, fnorm {fn!r} vs {np.sqrt(np.sum(f * f))!r}")
    np.testing.assert_allclose(rn, np.sqrt(np.sum(r * r)), rtol=1e-12)
    np.testing.assert_allclose(fn, np.sqrt(np.sum(f * f)), rtol=1e-12)
    assert np.array_equal(ctx.refine_get(mg._lib.REFINE_PSI).view(np.uint64), psi.view(np.uint64))
    assert np.array_equal(ctx.refine_get(mg._lib.REFINE_F).view(np.uint64), f.view(np.uint64))


# ---- 2. step bit-exactness ------------------------------------------------------------------------------------------

STEP_CASES = {
    "a-2d-rbgs-charge": (dict(dim=2, n=(32, 32, 1), **RB), "charge"),
    "a-2d-rbgs-random": (dict(dim=2, n=(32, 32, 1), **RB), "random"),
    "b-2d-jacobi-pc": (dict(dim=2, n=(16, 16, 1)), "charge"),  # the cpu.lua defaults: Jacobi 7+7, injection
    "c-3d-rbgs-charge": (dict(dim=3, n=(16, 16, 16), **RB), "charge"),
    "c-3d-rbgs-random": (dict(dim=3, n=(16, 16, 16), **RB), "random"),
    "d-3d-box-F": (dict(dim=3, n=(8, 8, 32), cycle="F", **RB), "charge"),
    "e-3d-fw": (dict(dim=3, n=(16, 16, 16), restriction="full_weighting", **RB), "charge"),
    "f-2d-gslex": (dict(dim=2, n=(32, 32, 1), smoother="gs_lex", nu1=2, nu2=2, prolong="linear"), "charge"),
}
OUTER = 3


def _start(case):
    kw, rhs = STEP_CASES[case]
    return _point_charge(kw) if rhs == "charge" else _random(kw, seed=11)


@functools.lru_cache(maxsize=None)
def _restated(case, inner):
    """The outer loop restated: [(psi, e, rnorm, err)] after each of OUTER steps.  Computed once per case; read only."""
    kw, _ = STEP_CASES[case]
    nx = kw["n"][0]
    h = 1.0 / nx
    psi, f = _start(case)
    orc = Oracle(real="float", **kw)
    out = []
    for _ in range(OUTER):
        r = residual_arr(kw["dim"], psi, f, h)
        e = np.zeros(_shape(kw), np.float32)
        r32 = r.astype(np.float32)
        for _ in range(inner):
            orc.two_grid(h, e, r32, nx)
        psi = psi + e.astype(np.float64)
        e64 = e.astype(np.float64)
        out.append((psi, e, float(np.sqrt(np.sum(r * r))), float(np.sqrt(np.sum(e64 * e64) / e.size))))
    return out


def _run_steps(case, inner):
    """[(psi64, level-0 u, rnorm, err)] of OUTER refine_step calls on a fresh context."""
    mg = _mg()
    kw, _ = STEP_CASES[case]
    psi, f = _start(case)
    ctx = _ctx(kw)
    ctx.refine_set(mg._lib.REFINE_PSI, psi)
    ctx.refine_set(mg._lib.REFINE_F, f)
    out = []
    for _ in range(OUTER):
        rn, _fn, err = ctx.refine_step(inner)
        out.append((ctx.refine_get(mg._lib.REFINE_PSI), ctx.get_psi(), rn, err))
    return out


@pytest.mark.parametrize("inner", [1, 4])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_is_bit_exact(case, inner):
    ref = _restated(case, inner)
    got = _run_steps(case, inner)
    for k, ((psi, u, rn, err), (psi_r, e_r, rn_r, err_r)) in enumerate(zip(got, ref)):
        print(f"{case} inner {inner} step {k + 1}: rnorm {rn!r} vs {rn_r!r}, err {err!r} vs {err_r!r}")
        assert psi.dtype == np.float64 and u.dtype == np.float32
        assert np.array_equal(u.view(np.uint32), e_r.view(np.uint32)), f"e of step {k + 1}"
        assert np.array_equal(psi.view(np.uint64), psi_r.view(np.uint64)), f"psi of step {k + 1}"
        np.testing.assert_allclose(rn, rn_r, rtol=1e-12)
        np.testing.assert_allclose(err, err_r, rtol=1e-12)


# ---- 3. engine independence -----------------------------------------------------------------------------------------

ENGINES = {
    "eager": {"MGP_GRAPH": "0"},
    "pieces": {"MGP_FUSED": "0", "MGP_BLK": "0", "MGP_TAIL": "0"},
    "memset-zero": {"MGP_LAZY_ZERO": "0"},
}


@functools.lru_cache(maxsize=None)
def _default_psi(case):
    return [s[0] for s in _run_steps(case, 4)]


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("case", ["a-2d-rbgs-charge", "a-2d-rbgs-random", "c-3d-rbgs-charge", "c-3d-rbgs-random"])
def test_steps_do_not_depend_on_the_engine(case, engine, monkeypatch):
    ref = _default_psi(case)  # (before the switches are set)
    for k, v in ENGINES[engine].items():
        monkeypatch.setenv(k, v)
    got = _run_steps(case, 4)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g[0].view(np.uint64), r.view(np.uint64)), f"psi of step {k + 1}"


# ---- 4. it reaches double's answer ----------------------------------------------------------------------------------


def _rel_max(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("kw", [dict(dim=3, n=(16, 16, 16), **RB), dict(dim=2, n=(32, 32, 1), **RB)], ids=["3d-16", "2d-32"])
def test_refine_solve_reaches_the_double_answer(kw):
    """Oracle figures: final rel 4e-16 (3D) / 1.5e-15 (2D); distance to double 8.9e-17 / 4.9e-16; plain float
    4.1e-8 / 1.0e-7."""
    mg = _mg()
    dbl = mg.Context(mg.make_opts(real="double", **kw))
    dbl.init_point_charge()
    dbl.cycles(80)
    psi_d = dbl.get_psi()
    flt = _ctx(kw, begin=False)
    flt.init_point_charge()
    flt.cycles(80)
    ctx = _ctx(kw)
    ctx.init_point_charge()
    steps, rel, err = ctx.refine_solve(inner=4, rtol=0.0, epsilon=0.0, maxouter=12)
    d_mixed = _rel_max(ctx.refine_get(mg._lib.REFINE_PSI), psi_d)
    d_float = _rel_max(flt.get_psi().astype(np.float64), psi_d)
    print(f"steps {steps}, rel_hist {rel.tolist()}, err_hist {err.tolist()}, mixed-double {d_mixed!r}, float-double {d_float!r}")
    assert steps == 12 and len(rel) == 13 and len(err) == 12
    assert rel[-1] <= 1e-13
    assert d_mixed <= 1e-13
    assert d_float >= 1e-8
    for a, b in zip(rel[:-1], rel[1:]):
        if a >= 1e-14:
            assert b <= a, rel.tolist()


# ---- 5. the drop-in protocol ----------------------------------------------------------------------------------------


def test_solver_protocol_mixed():
    mg = _mg()
    build = dict(size=16, dim=3, smoother="rbgs", smooth=2, prolong="linear")
    seen = []
    s = mg.MultigridHIP(real="mixed", maxiter=50, errorCallback=lambda it, err: seen.append((it, err)) and False, **build)
    assert s.innerCycles == 4
    s.solve()
    print("mixed solve():", seen)
    assert 1 <= len(seen) <= 8 and seen[-1][1] < 1e-10  # (the oracle: step 6)
    assert [it for it, _ in seen] == list(range(1, len(seen) + 1))
    assert all(e >= 1e-10 for _, e in seen[:-1])
    psi = s.psi
    assert psi.dtype == np.float64 and s.f.dtype == np.float64
    d = mg.MultigridHIP(real="double", maxiter=80, epsilon=0.0, **build)
    d.solve()
    print("mixed - double:", _rel_max(psi, d.psi))
    assert _rel_max(psi, d.psi) <= 1e-13
    n_float = []
    fl = mg.MultigridHIP(real="float", maxiter=50, errorCallback=lambda it, err: n_float.append(err) and False, **build)
    fl.solve()
    assert len(n_float) == 50  # the float solver's err never gets below epsilon = 1e-10
    with pytest.raises(mg.MGPError):
        s.twoGrid(1.0 / 16, np.zeros((16, 16, 16), np.float32), np.zeros((16, 16, 16), np.float32))


def test_solver_rebuild_keeps_the_double_fields():
    mg = _mg()
    s = mg.MultigridHIP(size=16, dim=3, real="mixed", smoother="rbgs", smooth=2, prolong="linear")
    s.step()
    psi, f = s.psi, s.f
    s.smooth = 3  # rebuilds the device context on next use
    assert s.ctx.opts.nu1 == 3
    assert np.array_equal(s.psi.view(np.uint64), psi.view(np.uint64))
    assert np.array_equal(s.f.view(np.uint64), f.view(np.uint64))
    s.inPlaceIterativeSolver = mg.MultigridHIP.Jacobi
    assert np.array_equal(s.psi.view(np.uint64), psi.view(np.uint64))
    assert np.isfinite(s.step())


def test_raw_protocol_mixed():
    mg = _mg()
    with pytest.raises(ValueError):
        mg.MultigridHIPRaw(16, "mixed", arith="double")
    s = mg.MultigridHIPRaw(16, "mixed")
    s.quiet = True
    assert s.arith == "real" and s.ctx.opts.real_bytes == 4 and s.ctx.opts.arith == 0
    errs = s.run()
    assert len(errs) == 2 and all(np.isfinite(errs))
    assert s.psi.dtype == np.float64 and s.f.dtype == np.float64


# ---- 6. stopping rules ----------------------------------------------------------------------------------------------


def test_refine_solve_stopping_rules():
    mg = _mg()
    kw = dict(dim=3, n=(16, 16, 16), **RB)
    ctx = _ctx(kw)
    ctx.init_point_charge()
    steps, rel, err = ctx.refine_solve(inner=4, rtol=1e-6, epsilon=0.0, maxouter=12)
    print("rtol 1e-6:", steps, rel.tolist())
    first = next(i for i, v in enumerate(rel) if v <= 1e-6)
    assert steps == first == len(rel) - 1 and len(err) == steps
    # no cycle ran after the defect that met rtol: psi still has exactly that defect
    rn, fn = ctx.refine_residual()
    assert rn / fn == rel[-1]
    ctx2 = _ctx(kw)
    ctx2.init_point_charge()
    steps, rel, err = ctx2.refine_solve(inner=4, rtol=0.0, epsilon=0.0, maxouter=2)
    assert steps == 2 and len(rel) == 3 and len(err) == 2
    # err < epsilon ends the loop after that step
    ctx3 = _ctx(kw)
    ctx3.init_point_charge()
    steps, rel, err = ctx3.refine_solve(inner=4, rtol=0.0, epsilon=1e30, maxouter=5)
    assert steps == 1 and len(rel) == 1 and len(err) == 1


# ---- 7. state rules -------------------------------------------------------------------------------------------------


def _code(exc):
    return exc.value.code


def test_begin_refusals(monkeypatch):
    mg = _mg()
    ARG, STATE = -1, -5
    kw = dict(dim=3, n=(16, 16, 16), **RB)
    with pytest.raises(mg.MGPError) as e:
        mg.Context(mg.make_opts(real="double", **kw)).refine_begin()
    assert _code(e) == ARG
    with pytest.raises(mg.MGPError) as e:
        mg.Context(mg.make_opts(real="float", arith="double", **kw)).refine_begin()
    assert _code(e) == ARG
    ctx = _ctx(kw)
    with pytest.raises(mg.MGPError) as e:
        ctx.refine_begin()  # twice
    assert _code(e) == STATE
    # world > 1 on the loopback transport
    lb = mg.Loopback(2)
    ranks = [mg.Context(mg.make_opts(real="float", world=2, rank=r, device=0, comm_id=b"\0" * 128, **kw), loopback=lb)
             for r in range(2)]
    with pytest.raises(mg.MGPError) as e:
        ranks[0].refine_begin()
    assert _code(e) == STATE
    for r in ranks:
        r.close()
    lb.close()
    # a group's rank context
    g = mg.Group(mg.make_opts(real="float", **kw), 2, devices=[0, 0])
    with pytest.raises(mg.MGPError) as e:
        g.ranks[0].refine_begin()
    assert _code(e) == STATE
    g.close()
    # world 1 on a one-rank RCCL communicator
    monkeypatch.setenv("MGP_TRANSPORT", "rccl")
    rc = mg.Context(mg.make_opts(real="float", **kw))
    with pytest.raises(mg.MGPError) as e:
        rc.refine_begin()
    assert _code(e) == STATE
    rc.close()


def test_calls_outside_their_state():
    mg = _mg()
    L = mg._lib
    ARG, STATE = -1, -5
    kw = dict(dim=2, n=(32, 32, 1), **RB)
    ctx = _ctx(kw, begin=False)
    ctx.init_point_charge()
    for call in (lambda: ctx.refine_step(4), ctx.refine_end, ctx.refine_residual, lambda: ctx.refine_get(L.REFINE_PSI),
                 lambda: ctx.refine_set(L.REFINE_F, np.zeros((32, 32))), lambda: ctx.refine_solve(4, 0.0, 0.0, 1)):
        with pytest.raises(mg.MGPError) as e:
            call()
        assert _code(e) == STATE
    ctx.refine_begin()
    with pytest.raises(mg.MGPError) as e:
        ctx.refine_step(0)
    assert _code(e) == ARG
    with pytest.raises(mg.MGPError) as e:
        ctx.refine_set(L.REFINE_PSI, np.zeros((32, 16)))  # a wrong count
    assert _code(e) == ARG
    with pytest.raises(mg.MGPError) as e:
        ctx.refine_set(2, np.zeros((32, 32)))
    assert _code(e) == ARG
    for call in (ctx.cycle, lambda: ctx.cycles(2), lambda: ctx.set_psi(np.zeros((32, 32), np.float32)),
                 lambda: ctx.set_f(np.zeros((32, 32), np.float32)), ctx.metrics, ctx.cg_solve,
                 lambda: ctx.two_grid(1.0 / 32, np.zeros((32, 32), np.float32), np.zeros((32, 32), np.float32), 32),
                 lambda: ctx.set_planes(L.FIELD_U, 0, np.zeros((1, 32, 32), np.float32))):
        with pytest.raises(mg.MGPError, match="refinement is active") as e:
            call()
        assert _code(e) == STATE
    ctx.set_field(L.FIELD_F, np.zeros((16, 16), np.float32), level=1)  # coarse levels stay writable


def test_begin_widens_and_end_narrows():
    mg = _mg()
    L = mg._lib
    kw = dict(dim=3, n=(16, 16, 16), **RB)
    u0, f0 = (a.astype(np.float32) for a in _random(kw, seed=3))
    ctx = _ctx(kw, begin=False)
    ctx.set_psi(u0)
    ctx.set_f(f0)
    ctx.refine_begin()
    assert np.array_equal(ctx.refine_get(L.REFINE_PSI), u0.astype(np.float64))
    assert np.array_equal(ctx.refine_get(L.REFINE_F), f0.astype(np.float64))
    ctx.refine_step(2)
    psi, f = ctx.refine_get(L.REFINE_PSI), ctx.refine_get(L.REFINE_F)
    ctx.refine_end()
    assert np.array_equal(ctx.get_psi().view(np.uint32), psi.astype(np.float32).view(np.uint32))
    assert np.array_equal(ctx.get_f().view(np.uint32), f.astype(np.float32).view(np.uint32))
    errs = ctx.cycles(2)  # an ordinary fp32 context again
    fresh = _ctx(kw, begin=False)
    fresh.set_psi(psi.astype(np.float32))
    fresh.set_f(f.astype(np.float32))
    np.testing.assert_array_equal(errs, fresh.cycles(2))
    assert np.array_equal(ctx.get_psi().view(np.uint32), fresh.get_psi().view(np.uint32))
    ctx.refine_begin()  # begin -> end -> begin
    assert np.array_equal(ctx.refine_get(L.REFINE_PSI), fresh.get_psi().astype(np.float64))
    assert np.isfinite(ctx.refine_step(4)[2])


@pytest.mark.parametrize("kw", [dict(dim=3, n=(16, 16, 16), **RB), dict(dim=2, n=(32, 32, 1), **RB)], ids=["3d", "2d"])
def test_init_point_charge_while_active(kw):
    mg = _mg()
    L = mg._lib
    ctx = _ctx(kw)
    ctx.refine_set(L.REFINE_PSI, np.ones(_shape(kw)))
    ctx.init_point_charge()
    psi, f = ctx.refine_get(L.REFINE_PSI), ctx.refine_get(L.REFINE_F)
    psi_r, f_r = _point_charge(kw)
    assert np.array_equal(f, f_r) and np.count_nonzero(f) == 1 and f.min() == -1e6
    assert np.array_equal(psi, -f)
    assert np.array_equal(psi, psi_r)


# ---- 8. debug and timing --------------------------------------------------------------------------------------------


def test_debug_check_in_a_step():
    """With mgp_set_debug(1) the narrowed defect is scanned like every phase of the inner cycles: a NaN in the fp64
    f fails the step with the existing "found a nan" message, naming the defect (the documented behaviour)."""
    mg = _mg()
    L = mg._lib
    kw = dict(dim=3, n=(16, 16, 16), **RB)
    ref = _ctx(kw)
    ref.init_point_charge()
    want = ref.refine_step(4)
    ctx = _ctx(kw)
    ctx.init_point_charge()
    ctx.set_debug(1)
    assert ctx.refine_step(4) == want
    assert np.array_equal(ctx.refine_get(L.REFINE_PSI).view(np.uint64), ref.refine_get(L.REFINE_PSI).view(np.uint64))
    f = ctx.refine_get(L.REFINE_F)
    f.flat[f.size // 3] = np.nan
    ctx.refine_set(L.REFINE_F, f)
    with pytest.raises(mg.MGPError, match=r"found a nan .*the defect"):
        ctx.refine_step(4)
    ctx.set_debug(0)
    rn, _fn, err = ctx.refine_step(4)  # unchecked: non-finite figures, the outer loop's break (cpu.lua:214)
    assert not np.isfinite(rn) and not np.isfinite(err)


def test_timing_brackets_the_two_passes():
    kw = dict(dim=3, n=(16, 16, 16), **RB)
    ctx = _ctx(kw)
    ctx.init_point_charge()
    ctx.timing(True)
    ctx.refine_step(2)
    ctx.refine_residual()
    t = ctx.timing_read()
    cells = 16 ** 3
    assert t["refine_defect"][1] == 2 and t["refine_defect"][2] == (24 + 20) * cells
    assert t["refine_add"][1] == 1 and t["refine_add"][2] == 20 * cells
    assert t["refine_defect"][0] > 0 and t["refine_add"][0] > 0
