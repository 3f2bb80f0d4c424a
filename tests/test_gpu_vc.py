"""GPU: variable coefficients (mgp_set_coefficients and what follows beta) against the host model of vc_model.py.

Fields and coefficients are compared bit for bit (tobytes()); err and the norms, fp64 sums in another order, to 1e-12
relative as in the constant cycle's tests.  Shapes: the smallest that reach every code form: 64^2, 16^3 and the 32-long
rows run the 16-byte vector half-sweep on their upper levels, everything else the scalar form down through nx = 4, 2, 1,
the one-cell level and the 1 x 1 x 4 coarsest level.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import project_model as pm  # noqa: E402
import vc_model as vm  # noqa: E402
from abi_model import RESIDUAL, dense  # noqa: E402
from bc_model import mean_free  # noqa: E402
from test_gpu_dense import _env, _mg  # noqa: E402

ERR_ARG, ERR_STATE = -1, -5
BOXES_2D = [(16, 16), (64, 64), (32, 8)]
BOXES_3D = [(8, 8, 8), (16, 16, 16), (32, 8, 8), (8, 8, 32)]
BOXES = BOXES_2D + BOXES_3D
# (real, boundary, cycle, prolongation, coarse guess)
COMBOS = [("float", "zero", "V", "linear", "fresh"), ("double", "consistent", "F", "pc", "warm"),
          ("float", "face", "F", "linear", "warm"), ("double", "neumann", "V", "pc", "fresh"),
          ("float", "neumann", "F", "linear", "fresh"), ("double", "face", "V", "linear", "fresh"),
          ("float", "consistent", "V", "pc", "warm"), ("double", "zero", "F", "linear", "warm")]
# every combination on one 2D and two 3D boxes, two each (all eight between them) on the others
CROSS = [(b, c) for b in ((16, 16), (8, 8, 8), (8, 8, 32)) for c in COMBOS] + \
        [(b, COMBOS[(2 * i + k) % 8]) for i, b in enumerate(((64, 64), (32, 8), (16, 16, 16), (32, 8, 8))) for k in (0, 1)]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v[0], int) else "-".join(v)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.size == b.size and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _kw(box, real, bc, cycle="V", prolong="linear", init="fresh", **extra):
    return dict(dim=len(box), n=tuple(box) + (1,) * (3 - len(box)), real=real, coarse_bc=bc, smoother="rbgs", nu1=2,
                nu2=2, cycle=cycle, prolong=prolong, coarse_init=init, **extra)


def _L():
    from mgpoisson import _lib

    return _lib


def _ctx(kw):
    mg = _mg()
    return mg.Context(mg.make_opts(**kw))


def _beta(m, seed, kind="random"):
    if kind == "smooth":
        return vm.smooth_beta(m.shapes[0], m.dim, m.dtype)
    return vm.random_beta(np.random.default_rng(seed), m.shapes[0], m.dim, m.dtype)


def _fill(ctx, m, seed):
    """The same dense psi and f on every level of the context and of the model (level 0's f mean-free under Neumann)."""
    mg = _mg()
    for l, s in enumerate(m.shapes):
        u, f = dense(s, m.dtype, seed + l), dense(s, m.dtype, seed + 40 + l)
        if l == 0 and m.kw["coarse_bc"] == "neumann":
            f = mean_free(f)
        m.u[l], m.f[l] = u.copy(), f.copy()
        ctx.set_field(mg.FIELD_U, u, level=l)
        ctx.set_field(mg.FIELD_F, f, level=l)


def _pair(kw, seed, kind="random"):
    ctx, m = _ctx(kw), vm.make_model(**kw)
    B = _beta(m, seed, kind)
    ctx.set_coefficients(*B[:m.dim])
    m.set_coefficients(*B)
    _fill(ctx, m, seed + 100)
    return ctx, m, B


def _levels_same(ctx, m, what):
    mg = _mg()
    for l in range(m.nlev):
        assert _same(ctx.get_field(mg.FIELD_U, level=l), m.u[l]), f"{what}: u, level {l}"
        assert _same(ctx.get_field(mg.FIELD_F, level=l), m.f[l]), f"{what}: f, level {l}"


def _close(a, b, tol=1e-12):
    return abs(a - b) <= tol * abs(b)


# ---- 1. the coefficients of every level ----

@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", BOXES, ids=_ids)
def test_coefficients_of_every_level(box, real, monkeypatch):
    _env(monkeypatch, {})
    kw = _kw(box, real, "face")
    ctx, m = _ctx(kw), vm.make_model(**kw)
    assert not ctx.has_coefficients()
    with pytest.raises(_mg().MGPError) as e:
        ctx.get_coefficients(0, 0)
    assert e.value.code == ERR_STATE
    B = _beta(m, 5)
    ctx.set_coefficients(*B[:m.dim])
    m.set_coefficients(*B)
    assert ctx.has_coefficients() and all(lv["engine"] == "piece" for lv in ctx.levels)
    for l in range(m.nlev):
        for a in range(m.dim):
            assert _same(ctx.get_coefficients(l, a), m.coef[l][a]), (l, a)
    ctx.close()


# ---- 2. the pieces ----

@pytest.mark.parametrize("bc", ["zero", "consistent", "face", "neumann"])
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", BOXES, ids=_ids)
def test_pieces(box, real, bc, monkeypatch):
    mg = _mg()
    _env(monkeypatch, {})
    ctx, m, _ = _pair(_kw(box, real, bc), 20 + sum(box))
    for l in range(m.nlev):
        assert _same(ctx.get_field(mg.FIELD_RESIDUAL, level=l), m.view(l, RESIDUAL)), f"residual field, level {l}"
        rn, fn = ctx.residual_norm(l)
        wr, wf = m.residual_norm(l)
        assert _close(rn, wr) and _close(fn, wf), (l, rn, wr, fn, wf)
    for l in range(m.nlev):
        ctx.smooth(l, 2)
        m.smooth(l, 2)
    _levels_same(ctx, m, "smooth")
    for l in range(m.nlev - 1):
        ctx.residual_restrict(l)
        m.residual_restrict(l)
    _levels_same(ctx, m, "residual + restrict")
    ctx.coarse_solve()
    m.coarse_solve()
    _levels_same(ctx, m, "coarse solve")
    for l in range(m.nlev - 2, -1, -1):
        ctx.prolong_correct(l)
        m.prolong_correct(l)
    _levels_same(ctx, m, "prolong + correct")
    ctx.close()


# The residual + restriction takes its 16-byte form where MGP_RR_SCALAR_CELLS is given, from that many coarse cells up
# (by default a thread per coarse cell everywhere: measured faster): with the threshold at 0 every level whose coarse rows
# hold 16 bytes runs it, the shorter ones the scalar form, and both give the model's bits.
@pytest.mark.parametrize("bc", ["zero", "consistent", "face", "neumann"])
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", [(64, 64), (32, 8), (16, 16, 16), (32, 8, 8), (8, 8, 32)], ids=_ids)
def test_vector_residual_restrict(box, real, bc, monkeypatch):
    _env(monkeypatch, {})
    monkeypatch.setenv("MGP_RR_SCALAR_CELLS", "0")
    ctx, m, _ = _pair(_kw(box, real, bc), 250 + sum(box))
    for l in range(m.nlev - 1):
        ctx.residual_restrict(l)
        m.residual_restrict(l)
    _levels_same(ctx, m, "residual + restrict, 16-byte form")
    ctx.cycles(2)
    m.cycles(2)
    _levels_same(ctx, m, "2 cycles, 16-byte residual + restrict")
    ctx.close()


# ---- 3. whole cycles, replayed and enqueued ----

@pytest.mark.parametrize("box,combo", CROSS, ids=_ids)
def test_three_cycles(box, combo, monkeypatch):
    real, bc, cycle, prolong, init = combo
    kw = _kw(box, real, bc, cycle, prolong, init)
    out = []
    for env in ({}, dict(MGP_GRAPH=0)):
        _env(monkeypatch, env)
        ctx, m, _ = _pair(kw, 300 + sum(box))
        errs = ctx.cycles(3)
        want = m.cycles(3)
        _levels_same(ctx, m, f"3 cycles {env}")
        print(f"{_ids(box)} {combo} {env}: err {list(errs)} model {want}")
        assert all(_close(float(e), w) for e, w in zip(errs, want)), (errs, want)
        rel, cnt, frob = ctx.metrics()
        wrel, wcnt, wfrob = m.metrics()
        assert cnt == wcnt and _close(frob, wfrob) and _close(rel, wrel)
        out.append((errs.tobytes(), ctx.get_psi().tobytes()))
        ctx.close()
    assert out[0] == out[1], "MGP_GRAPH=0 and replay differ"


# ---- 4. beta = 1 is the constant context ----

@pytest.mark.parametrize("bc", ["zero", "consistent", "face", "neumann"])
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", [(16, 16), (64, 64), (8, 8, 8), (16, 16, 16), (8, 8, 32)], ids=_ids)
def test_ones_give_the_constant_bits(box, real, bc, monkeypatch):
    _env(monkeypatch, {})
    kw = _kw(box, real, bc)
    a, b = _ctx(kw), _ctx(kw)
    m = vm.make_model(**kw)
    a.set_coefficients(*vm.ones_beta(m.shapes[0], m.dim, m.dtype)[:m.dim])
    _fill(a, m, 410)
    _fill(b, m, 410)
    ea, eb = a.cycles(3), b.cycles(3)
    assert _same(a.get_psi(), b.get_psi()) and ea.tobytes() == eb.tobytes(), (ea, eb)
    a.close()
    b.close()


# ---- 5. set, replace, clear ----

@pytest.mark.parametrize("real,box", [("float", (16, 16, 16)), ("double", (64, 64))], ids=str)
def test_set_replace_clear(real, box, monkeypatch):
    _env(monkeypatch, {})
    kw = _kw(box, real, "face")
    ctx, m, _ = _pair(kw, 500)
    const = _ctx(kw)
    engines = [lv["engine"] for lv in const.levels]
    ctx.cycles(2)
    m.cycles(2)
    _levels_same(ctx, m, "first coefficients")
    B2 = _beta(m, 501)
    ctx.set_coefficients(*B2[:m.dim])
    m.set_coefficients(*B2)
    ctx.cycles(2)
    m.cycles(2)
    _levels_same(ctx, m, "second coefficients")
    ctx.clear_coefficients()
    m.clear_coefficients()
    assert not ctx.has_coefficients() and [lv["engine"] for lv in ctx.levels] == engines
    psi, f = ctx.get_psi(), ctx.get_f()
    const.set_psi(psi)
    const.set_f(f)
    e1, e2 = ctx.cycles(2), const.cycles(2)
    m.cycles(2)
    assert _same(ctx.get_psi(), m.u[0]) and _same(ctx.get_psi(), const.get_psi()) and e1.tobytes() == e2.tobytes()
    ctx.close()
    const.close()


# ---- 6. invalid coefficients ----

@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")], ids=str)
@pytest.mark.parametrize("earlier", [False, True], ids=["none-set", "earlier-set"])
@pytest.mark.parametrize("real,box", [("float", (16, 16, 16)), ("double", (32, 8))], ids=str)
def test_invalid_coefficients_change_nothing(real, box, earlier, bad, monkeypatch):
    mg = _mg()
    _env(monkeypatch, {})
    kw = _kw(box, real, "zero")
    a, b = _ctx(kw), _ctx(kw)
    m = vm.make_model(**kw)
    B = _beta(m, 600)
    if earlier:
        for c in (a, b):
            c.set_coefficients(*B[:m.dim])
    _fill(a, m, 610)
    _fill(b, m, 610)
    axis = m.dim - 1 if bad == float("inf") else 0
    W = [None if x is None else x.copy() for x in _beta(m, 601)]
    W[axis].flat[W[axis].size - 1 if bad == float("inf") else W[axis].size // 3] = bad
    with pytest.raises(mg.MGPError) as e:
        a.set_coefficients(*W[:m.dim])
    assert e.value.code == ERR_ARG and f"coefficient not positive and finite: axis {axis}" in str(e.value)
    assert a.has_coefficients() == earlier
    ea, eb = a.cycles(2), b.cycles(2)
    assert _same(a.get_psi(), b.get_psi()) and ea.tobytes() == eb.tobytes()
    if earlier:
        for ax in range(m.dim):
            assert _same(a.get_coefficients(0, ax), B[ax])
    a.close()
    b.close()


# ---- 7. refusals ----

def _refused(code, fn, *args, **kw):
    with pytest.raises(_mg().MGPError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_set_coefficients_refusals(monkeypatch):
    mg = _mg()
    _env(monkeypatch, {})
    box = (16, 16, 16)
    m = vm.make_model(**_kw(box, "float", "face"))
    B = _beta(m, 700)
    for extra in (dict(arith="double"), dict(smoother="jacobi"), dict(smoother="gs_lex"), dict(restriction="full_weighting")):
        kw = _kw(box, "float", "face")
        kw.update(extra)
        ctx = _ctx(kw)
        _refused(ERR_ARG, ctx.set_coefficients, *B)
        assert not ctx.has_coefficients()
        ctx.close()
    ctx = _ctx(_kw(box, "float", "face"))
    p = [b.ctypes.data for b in B]
    _refused(ERR_ARG, ctx.set_coefficients_ptr, None, p[1], p[2], mem=_L().MEM_HOST)
    _refused(ERR_ARG, ctx.set_coefficients_ptr, p[0], None, p[2], mem=_L().MEM_HOST)
    _refused(ERR_ARG, ctx.set_coefficients_ptr, p[0], p[1], None, mem=_L().MEM_HOST)
    _refused(ERR_ARG, ctx.set_coefficients_ptr, p[0], p[1], p[2], mem=7)
    ctx.refine_begin()
    _refused(ERR_STATE, ctx.set_coefficients, *B)
    ctx.refine_end()
    ctx.set_coarse_handoff(4, lambda h, u, f, n: None)
    _refused(ERR_STATE, ctx.set_coefficients, *B)
    ctx.set_coarse_handoff(4, None)
    ctx.set_coefficients(*B)  # and now it is accepted
    assert ctx.has_coefficients()
    ctx.close()
    assert _L().lib.mgp_set_coefficients(None, p[0], p[1], p[2], _L().MEM_HOST) == ERR_ARG
    # 2D ignores bz
    m2 = vm.make_model(**_kw((16, 16), "float", "face"))
    B2 = _beta(m2, 701)
    c2 = _ctx(_kw((16, 16), "float", "face"))
    c2.set_coefficients_ptr(B2[0].ctypes.data, B2[1].ctypes.data, None, mem=_L().MEM_HOST)
    assert _same(c2.get_coefficients(0, 1), B2[1])
    c2.close()


def test_multi_rank_contexts_are_refused(monkeypatch):
    mg = _mg()
    _env(monkeypatch, {})
    box, world = (16, 16, 16), 2
    m = vm.make_model(**_kw(box, "float", "face"))
    B = _beta(m, 710)
    # loopback ranks
    lb = mg.Loopback(world)
    codes, errors = [None] * world, []

    def rank_main(r):
        try:
            kw = _kw(box, "float", "face")
            ctx = mg.Context(mg.make_opts(rank=r, world=world, device=0, comm_id=b"\0" * 128, **kw), loopback=lb)
            try:
                codes[r] = _L().lib.mgp_set_coefficients(ctx._h, B[0].ctypes.data, B[1].ctypes.data, B[2].ctypes.data, _L().MEM_HOST)
            finally:
                ctx.close()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    lb.close()
    assert not errors and codes == [ERR_STATE] * world, (errors, codes)
    # group ranks
    g = mg.Group(mg.make_opts(**_kw(box, "float", "face")), world, devices=[0] * world)
    _refused(ERR_STATE, g.ranks[0].set_coefficients_ptr, B[0].ctypes.data, B[1].ctypes.data, B[2].ctypes.data, mem=_L().MEM_HOST)
    g.close()
    # a one-rank RCCL communicator
    monkeypatch.setenv("MGP_TRANSPORT", "rccl")
    ctx = _ctx(_kw(box, "float", "face"))
    with pytest.raises(mg.MGPError) as e:
        ctx.set_coefficients(*B)
    assert e.value.code == ERR_STATE and "single-GPU contexts only" in str(e.value)
    ctx.close()
    monkeypatch.delenv("MGP_TRANSPORT")


def test_refused_while_coefficients_are_set(monkeypatch):
    mg = _mg()
    _env(monkeypatch, {})
    box = (16, 16, 16)
    ctx, m, B = _pair(_kw(box, "float", "face"), 720)
    shape = m.shapes[0]
    u, f = dense(shape, m.dtype, 1), dense(shape, m.dtype, 2)
    _refused(ERR_STATE, ctx.two_grid, 1.0 / 16, u, f, 16)
    _refused(ERR_STATE, ctx.cg_solve, 1e-10, 5)
    _refused(ERR_STATE, ctx.fmg, 1, 1)
    _refused(ERR_STATE, ctx.fmg_restrict_rhs, 0)
    _refused(ERR_STATE, ctx.fmg_prolong, 0)
    _refused(ERR_STATE, ctx.refine_begin)
    _refused(ERR_STATE, ctx.set_coarse_handoff, 4, lambda h, u, f, n: None)
    _refused(ERR_STATE, ctx.set_coarse_level, 4)
    v = pm.random_faces(np.random.default_rng(3), shape, 3, m.dtype)
    _refused(ERR_STATE, ctx.project, *v, fmg=1, cycles=1)
    # nothing changed: f was not written, and the cycle is the model's
    assert _same(ctx.get_f(), m.f[0]) and _same(ctx.get_psi(), m.u[0])
    ctx.cycles(2)
    m.cycles(2)
    _levels_same(ctx, m, "after the refusals")
    ctx.close()


# ---- 8. the gradient with coefficients ----

@pytest.mark.parametrize("bc", ["zero", "consistent", "face", "neumann"])
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", [(16, 16), (64, 64), (32, 8), (8, 8, 8), (32, 8, 8), (8, 8, 32)], ids=_ids)
def test_gradient_with_coefficients(box, real, bc, monkeypatch):
    import torch

    _env(monkeypatch, {})
    ctx, m, B = _pair(_kw(box, real, bc), 800 + sum(box))
    dim, shape3 = m.dim, (m.shapes[0] if m.dim == 3 else (1,) + m.shapes[0])
    v = pm.random_faces(np.random.default_rng(801), shape3, dim, m.dtype)
    c0 = pm.C0[bc]
    store, sub = vm.gradient(m.u[0], B, dim, c0), vm.gradient(m.u[0], B, dim, c0, v)
    got_store, got_sub = ctx.gradient(*v[:dim], subtract=False), ctx.gradient(*v[:dim], subtract=True)
    for a in range(dim):
        assert _same(got_store[a], store[a]), f"store, axis {a}"
        assert _same(got_sub[a], sub[a]), f"subtract, axis {a}"
    for subtract, want in ((True, sub), (False, store)):
        t = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in v[:dim]]
        torch.cuda.synchronize()
        ctx.gradient_ptr(*[x.data_ptr() for x in t], *([None] * (3 - dim)), subtract=subtract)
        for a in range(dim):
            assert _same(t[a].cpu().numpy(), want[a]), f"device, subtract {subtract}, axis {a}"
    assert _same(ctx.get_psi(), m.u[0])
    ctx.close()


# ---- 9. the variable-density projection ----

@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box,bc", [((16, 16, 16), "neumann"), ((32, 32), "face")], ids=str)
@pytest.mark.parametrize("k", [0, 3])
def test_projection(box, bc, real, k, monkeypatch):
    _env(monkeypatch, {})
    ctx, m, B = _pair(_kw(box, real, bc), 900, kind="smooth")
    dim, shape = m.dim, m.shapes[0]
    shape3 = shape if dim == 3 else (1,) + shape
    v = list(pm.random_faces(np.random.default_rng(901), shape3, dim, m.dtype))
    if bc == "neumann":  # no flow through the walls
        v[0][:, :, 0] = v[0][:, :, -1] = 0
        v[1][:, 0, :] = v[1][:, -1, :] = 0
        v[2][0] = v[2][-1] = 0
    faces, norms = ctx.project(*v[:dim], fmg=0, cycles=k)
    # the model's same steps; f = D v, under Neumann with its mean removed by the constant context's mgp_remove_mean
    # (that pass does not see beta, and its fixed-order fp64 sum is not numpy's)
    f = pm.divergence(v[0], v[1], v[2], dim).reshape(shape)
    if bc == "neumann":
        mg = _mg()
        ref = _ctx(_kw(box, real, bc))
        ref.set_f(f)
        ref.remove_mean(0, mg.FIELD_F)
        f = ref.get_f().reshape(shape)
        ref.close()
    m.f[0] = f
    m.cycles(k)
    want = vm.gradient(m.u[0], B, dim, pm.C0[bc], v)
    assert _same(ctx.get_f(), m.f[0]) and _same(ctx.get_psi(), m.u[0])
    for a in range(dim):
        assert _same(faces[a], want[a]), f"projected faces, axis {a}"
    wr, wf = m.residual_norm(0)
    assert _close(norms[0], wf) and _close(norms[1], wr), (norms, wf, wr)
    # norms[1] is the divergence norm of the returned faces, to rounding
    got = tuple(faces) + (None,) * (3 - dim)
    div_new = pm.divergence(got[0], got[1], got[2], dim)
    host = float(np.sqrt(np.sum(div_new.astype(np.float64) ** 2)))
    n0 = float(box[0])
    bmax = max(float(b.max()) for b in B[:dim])
    vmax = max(float(np.abs(x).max()) for x in v[:dim])
    bound = 64 * np.finfo(m.dtype).eps * (bmax * n0 * n0 * float(np.abs(m.u[0]).max()) + n0 * vmax) * np.sqrt(m.u[0].size)
    print(f"{_ids(box)} {real} {bc} k={k}: div before {norms[0]:.6e}, after {norms[1]:.6e}, host {host:.6e}, bound {bound:.3e}")
    assert abs(norms[1] - host) <= bound
    ctx.close()
