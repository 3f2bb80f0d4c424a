"""GPU: the MAC-grid projection (mgp_divergence, mgp_gradient, mgp_project) against the host model of project_model.py.

Fields are compared bit for bit (tobytes()).  Device-memory face arrays are PyTorch tensors passed by data_ptr().
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import project_model as pm  # noqa: E402
from dense_start import dense_fields  # noqa: E402
from test_gpu_dense import _env, _mg  # noqa: E402

BCS = ("zero", "consistent", "face", "neumann")
RBL = dict(smoother="rbgs", nu1=2, nu2=2, prolong="linear")
ERR_ARG, ERR_STATE = -1, -5

# (nx, ny[, nz]).  2x2 .. 4x4(x4): the scalar forms; 64x16, 16x64, 8^3, 16x8x4, 64x4x2, 32^3: the vector forms, one and
# several items per row; 2x16x64: scalar rows in many planes; 128x64x32: many workgroups (fp32 128, fp64 256), so the XCD
# band order of the workgroups and rows shared between workgroups; 1x1x4, 1x8, 8x1: one-cell axes (empty slots of nx = 1
# rows, both ghosts from one cell).  A second grid-stride step needs more than kMaxBlocks workgroups (2^28 items, 2^31
# cells in fp32), which no quick test can hold: the loop is mgp_mean.hip's (`it += gridDim.x * kBlock`).
BOXES_2D = [(2, 2), (4, 4), (64, 16), (16, 64), (1, 8), (8, 1)]
BOXES_3D = [(2, 2, 2), (4, 4, 4), (8, 8, 8), (16, 8, 4), (64, 4, 2), (2, 16, 64), (32, 32, 32), (128, 64, 32), (1, 1, 4)]
BOXES = BOXES_2D + BOXES_3D


def _n3(box):
    return tuple(box) + (1,) * (3 - len(box))


def _shape(box):
    return (box[2] if len(box) == 3 else 1, box[1], box[0])


def _ids(box):
    return "x".join(map(str, box))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.size == b.size and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _kw(box, real, bc, **extra):
    return dict(dim=len(box), n=_n3(box), real=real, coarse_bc=bc, **RBL, **extra)


def _ctx(box, real, bc, **extra):
    mg = _mg()
    return mg.Context(mg.make_opts(**_kw(box, real, bc, **extra)))


def _faces_same(got, want, what):
    for a, (g, w) in enumerate(zip(got, want)):
        if w is not None:
            assert _same(g, w), f"{what}: axis {a}"


def _special_fields(box, dt, seed):
    """Dense random psi and faces with a -0 and a subnormal in each."""
    shape, dim = _shape(box), len(box)
    rng = np.random.default_rng(seed)
    psi = rng.uniform(-1, 1, shape).astype(dt)
    v = pm.random_faces(rng, shape, dim, dt)
    tiny = np.finfo(dt).smallest_subnormal
    psi.flat[0] = dt.type(-0.0)
    psi.flat[psi.size - 1] = tiny
    for a in v:
        if a is not None:
            a.flat[0] = dt.type(-0.0)
            a.flat[a.size - 1] = -tiny
            a.flat[a.size // 2] = tiny
    return psi, v


class _Dev:
    """Face arrays in device memory (PyTorch tensors)."""

    def __init__(self, v):
        import torch

        self.t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in v]
        torch.cuda.synchronize()
        self.ptrs = [None if t is None else t.data_ptr() for t in self.t]

    def host(self):
        return tuple(None if t is None else t.cpu().numpy() for t in self.t)


def _check_operators(ctx, box, bc, seed):
    dim, dt = len(box), ctx.dtype
    c0 = pm.C0[bc]
    psi, v = _special_fields(box, dt, seed)
    ctx.set_psi(psi)
    want_f = pm.divergence(*v, dim)
    want_g = pm.gradient(psi, dim, c0)
    want_w = pm.subtract(v, want_g)
    # host memory
    ctx.divergence(*v)
    assert _same(ctx.get_f(), want_f), "divergence (host)"
    _faces_same(ctx.gradient(*v, subtract=False), want_g, "gradient store (host)")
    _faces_same(ctx.gradient(*v, subtract=True), want_w, "gradient subtract (host)")
    # device memory
    ctx.set_f(np.ones(_shape(box), dt))
    d = _Dev(v)
    ctx.divergence_ptr(*d.ptrs)
    assert _same(ctx.get_f(), want_f), "divergence (device)"
    _faces_same(d.host(), v, "divergence leaves the faces")
    ctx.gradient_ptr(*d.ptrs, subtract=True)
    _faces_same(d.host(), want_w, "gradient subtract (device)")
    ctx.gradient_ptr(*d.ptrs, subtract=False)
    _faces_same(d.host(), want_g, "gradient store (device)")
    assert _same(ctx.get_psi(), psi) and _same(ctx.get_f(), want_f), "psi and f untouched by the gradient"
    return want_f


# ---- 1. bit parity with the model ----

@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", BOXES, ids=_ids)
def test_operators_match_the_model(box, real, bc, monkeypatch):
    _env(monkeypatch, {})
    ctx = _ctx(box, real, bc)
    _check_operators(ctx, box, bc, 700 + sum(box))
    ctx.close()


# ---- 2. layout: plane stride and buffer offsets ----

# 256x256x4: the smallest planes (2^16 slots) that take the padded stride
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", [(16, 8, 4), (32, 32, 32), (256, 256, 4)], ids=_ids)
def test_layout_switches(box, real, monkeypatch):
    mg = _mg()
    out = []
    for plane_pad, pad_bytes in ((None, None), (4352, None), (None, 0), (4352, 0)):
        _env(monkeypatch, {} if plane_pad is None else dict(MGP_PLANE_PAD=plane_pad))
        if pad_bytes is None:
            monkeypatch.delenv("MGP_PAD_BYTES", raising=False)
        else:
            monkeypatch.setenv("MGP_PAD_BYTES", str(pad_bytes))
        ctx = _ctx(box, real, "face")
        want_f = _check_operators(ctx, box, "face", 760)
        stats = ctx.field_stats(mg.FIELD_F)
        # pad slots and ghost planes of f stayed 0: a cycle from this f gives the bits of every other layout
        err = ctx.cycle()
        out.append((stats, err, ctx.get_psi().tobytes(), ctx.get_f().tobytes()))
        assert _same(ctx.get_f(), want_f)
        ctx.close()
    monkeypatch.delenv("MGP_PAD_BYTES", raising=False)
    assert all(o == out[0] for o in out[1:])


# ---- 3. the gradient reads the psi that get_field(U) returns ----

def test_gradient_reads_the_current_psi(monkeypatch):
    mg = _mg()
    box = (64, 32, 64)
    _env(monkeypatch, dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536))
    ctx = _ctx(box, "float", "consistent")  # (c_0 = 0: the engine of the dense cycle tests)
    assert ctx.levels[0]["engine"] == "zs" and ctx.opts.err_mode == 1
    shape, dt = _shape(box), ctx.dtype
    v = pm.random_faces(np.random.default_rng(771), shape, 3, dt)

    def check(what):
        psi = ctx.get_psi()
        _faces_same(ctx.gradient(*v, subtract=False), pm.gradient(psi, 3, 0.0), what + " (store)")
        d = _Dev(v)
        ctx.gradient_ptr(*d.ptrs, subtract=True)
        _faces_same(d.host(), pm.subtract(v, pm.gradient(psi, 3, 0.0)), what + " (subtract, device)")
        assert _same(ctx.get_psi(), psi)
        return psi

    assert not check("a fresh context").any()  # the lazily zeroed guess
    ctx.init_point_charge()
    assert check("after init_point_charge").any()
    psi0, f0 = dense_fields(shape, dt, 772)
    ctx.set_psi(psi0)
    ctx.set_f(f0)
    ctx.cycles(2)
    old = ctx.get_field(mg.FIELD_PSI_OLD)
    psi = check("after two temporally blocked cycles with err")
    assert not _same(psi, psi0) and not _same(psi, old)
    assert _same(ctx.get_field(mg.FIELD_PSI_OLD), old)  # psiOld survived the gradient
    ctx.cycles(1)
    check("after a third cycle (the other rotating buffer)")
    ctx.close()


# ---- 4. D(v - G psi) == f - A psi on the device ----

@pytest.mark.parametrize("bc", ["face", "neumann"])
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", [(16, 8, 4), (64, 16)], ids=_ids)
def test_identity_on_the_device(box, real, bc, monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    ctx = _ctx(box, real, bc)
    shape, dim, dt = _shape(box), len(box), ctx.dtype
    rng = np.random.default_rng(780)
    psi = pm.dyadic(rng, shape, dt)
    v = pm.dyadic_faces(rng, shape, dim, dt)
    ctx.set_psi(psi)
    ctx.divergence(*v)
    r = ctx.get_field(mg.FIELD_RESIDUAL)
    assert np.any(r != 0)
    w = ctx.gradient(*v, subtract=True)
    ctx.divergence(*w)
    assert _same(ctx.get_f(), r)
    ctx.close()


# ---- 5. mgp_project is the composition of the separate calls ----

@pytest.mark.parametrize("device_mem", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmg,cycles", [(1, 1), (0, 2), (0, 0)])
@pytest.mark.parametrize("box,real,bc", [((32, 32, 32), "float", "neumann"), ((64, 64), "double", "face")],
                         ids=["3d-f32-neumann", "2d-f64-face"])
def test_project_is_the_composition(box, real, bc, fmg, cycles, device_mem, monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    a, b = _ctx(box, real, bc), _ctx(box, real, bc)
    shape, dim, dt = _shape(box), len(box), a.dtype
    psi0, _ = dense_fields(shape, dt, 790)
    v = pm.random_faces(np.random.default_rng(791), shape, dim, dt)
    if bc == "neumann":
        # no flow through the walls, as a Neumann projection requires: D v then has zero mean up to rounding, so the
        # mean removed from f in step 2 does not separate ||f - A psi|| from ||D (v - G psi)||
        v[0][:, :, 0] = v[0][:, :, -1] = 0
        v[1][:, 0, :] = v[1][:, -1, :] = 0
        if dim == 3:
            v[2][0] = v[2][-1] = 0
    for c in (a, b):
        c.set_psi(psi0)
    # one call
    if device_mem:
        d = _Dev(v)
        norms = a.project_ptr(*d.ptrs, fmg=fmg, cycles=cycles)
        faces = d.host()
    else:
        faces, norms = a.project(*v, fmg=fmg, cycles=cycles)
    # the separate calls
    b.divergence(*v)
    if bc == "neumann":
        b.remove_mean(0, mg.FIELD_F)
    if fmg >= 1:
        b.fmg(fmg, cycles)
    else:
        b.cycles(cycles)
    want = b.gradient(*v, subtract=True)
    rn, fn = b.residual_norm(0)
    assert _same(a.get_psi(), b.get_psi()) and _same(a.get_f(), b.get_f())
    _faces_same(faces, want, "projected faces")
    assert norms == (fn, rn), (norms, fn, rn)
    if cycles == 0 and fmg == 0:
        assert _same(a.get_psi(), psi0)
    # norms[1] is the divergence norm of the projected field, to rounding
    psi = a.get_psi().reshape(shape)
    faces = tuple(faces) + (None,) * (3 - len(faces))
    div_new = pm.divergence(*faces[:3], dim)
    host = float(np.sqrt(np.sum(div_new.astype(np.float64) ** 2)))
    n0 = float(box[0])
    vmax = max(np.abs(x).max() for x in v if x is not None)
    bound = 64 * np.finfo(dt).eps * (n0 * n0 * np.abs(psi).max() + n0 * vmax) * np.sqrt(psi.size)
    print(f"{_ids(box)} {real} {bc} ({fmg}, {cycles}): div before {norms[0]:.6e}, after {norms[1]:.6e}, host {host:.6e}, "
          f"|diff| {abs(norms[1] - host):.3e}, bound {bound:.3e}")
    assert abs(norms[1] - host) <= bound
    if fmg >= 1:  # (the dense random psi0 of the warm starts is no guess: its residual is far above ||f||)
        assert norms[1] < norms[0]
    a.close()
    b.close()


def test_solver_class_projects(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    n = 32
    s = mg.MultigridHIP(size=n, dim=2, real="double", smoother="rbgs", smooth=2, prolong="linear", boundary="neumann")
    v = list(pm.random_faces(np.random.default_rng(795), (1, n, n), 2, np.dtype(np.float64)))
    v[0][:, :, 0] = v[0][:, :, -1] = 0  # no flow through the walls: D v has zero mean
    v[1][:, 0, :] = v[1][:, -1, :] = 0
    (wx, wy), (before, after) = s.project(v[0], v[1], fmg=1, cycles=3)
    assert wx.shape == v[0].shape and wy.shape == v[1].shape
    assert after < 1e-2 * before  # (a V(2,2) cycle gains more than a factor 5)
    assert _same(wx[:, :, 0], v[0][:, :, 0]) and _same(wy[:, -1, :], v[1][:, -1, :])  # the walls keep their bits
    with pytest.raises(ValueError, match="shape"):
        s.project(v[1], v[0])
    s.divergence(wx, wy)
    assert abs(np.sqrt(np.sum(s.f.astype(np.float64) ** 2)) - after) <= 1e-9 * before


# ---- 6. refusals and debug ----

def _raw_calls(mg, ctx, dim=3):
    """(name, call) of the three entry points on a buffer large enough for any face array of the tests here."""
    lib = mg._lib.lib
    buf = np.zeros(1 << 17, np.float64)
    p = buf.ctypes.data
    vz = p if dim == 3 else None
    return buf, [("mgp_divergence", lambda: lib.mgp_divergence(ctx._h, p, p, vz, 0)),
                 ("mgp_gradient", lambda: lib.mgp_gradient(ctx._h, 1, p, p, vz, 0)),
                 ("mgp_project", lambda: lib.mgp_project(ctx._h, p, p, vz, 0, 1, 1, None))]


def _all_refuse(mg, ctx, code, text, dim=3):
    buf, calls = _raw_calls(mg, ctx, dim)
    for name, call in calls:
        assert call() == code, name
        msg = mg._lib.lib.mgp_last_error(ctx._h).decode()
        assert name in msg and text in msg, msg
    del buf


def test_refuses_bad_arguments_and_arith_double(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    lib = mg._lib.lib
    ctx = _ctx((16, 8, 4), "float", "face")
    psi0, f0 = dense_fields((4, 8, 16), ctx.dtype, 800)
    ctx.set_psi(psi0)
    ctx.set_f(f0)
    buf = np.zeros(1 << 12, np.float32)
    p = buf.ctypes.data

    def msg():
        return lib.mgp_last_error(ctx._h).decode()

    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.mgp_divergence(ctx._h, *args, 0) == ERR_ARG and "NULL face array" in msg()
        assert lib.mgp_gradient(ctx._h, 1, *args, 0) == ERR_ARG and "NULL face array" in msg()
        assert lib.mgp_project(ctx._h, *args, 0, 1, 1, None) == ERR_ARG and "NULL face array" in msg()
    assert lib.mgp_divergence(ctx._h, p, p, p, 2) == ERR_ARG and "unknown mem" in msg()
    assert lib.mgp_gradient(ctx._h, 1, p, p, p, -1) == ERR_ARG and "unknown mem" in msg()
    assert lib.mgp_project(ctx._h, p, p, p, 7, 1, 1, None) == ERR_ARG and "unknown mem" in msg()
    assert lib.mgp_gradient(ctx._h, 2, p, p, p, 0) == ERR_ARG and "unknown op" in msg()
    assert lib.mgp_gradient(ctx._h, -1, p, p, p, 0) == ERR_ARG and "unknown op" in msg()
    assert lib.mgp_project(ctx._h, p, p, p, 0, -1, 1, None) == ERR_ARG and "fmg_cycles >= 0" in msg()
    assert lib.mgp_project(ctx._h, p, p, p, 0, 1, -1, None) == ERR_ARG and "cycles >= 0" in msg()
    assert _same(ctx.get_psi(), psi0) and _same(ctx.get_f(), f0) and not buf.any()  # nothing ran
    with pytest.raises(ValueError, match="shape"):
        ctx.divergence(np.zeros((4, 8, 16), np.float32), np.zeros((4, 9, 16), np.float32), np.zeros((5, 8, 16), np.float32))
    ctx.close()
    # 2D ignores vz
    c2 = _ctx((16, 16), "double", "zero")
    vx, vy = np.zeros((1, 16, 17)), np.zeros((1, 17, 16))
    assert lib.mgp_divergence(c2._h, vx.ctypes.data, vy.ctypes.data, None, 0) == 0
    c2.close()
    raw = _ctx((16, 8, 4), "float", "face", arith="double")
    _all_refuse(mg, raw, ERR_ARG, "MGP_ARITH_DOUBLE")
    raw.close()


def test_refuses_refinement_and_handoff(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    ctx = _ctx((32, 32), "float", "face")
    ctx.init_point_charge()
    ctx.refine_begin()
    _all_refuse(mg, ctx, ERR_STATE, "refinement is active", dim=2)
    ctx.refine_end()
    ctx.set_coarse_handoff(8, lambda h, u, f, n: None)
    v = pm.random_faces(np.random.default_rng(810), (1, 32, 32), 2, ctx.dtype)
    with pytest.raises(mg.MGPError) as e:
        ctx.project(*v, fmg=1, cycles=1)  # whatever mgp_fmg refuses
    assert e.value.code == ERR_STATE and "hand-off" in str(e.value)
    ctx.set_coarse_handoff(0, None)
    _, (before, after) = ctx.project(*v, fmg=1, cycles=1)  # and afterwards it runs
    assert after < before
    ctx.close()


def test_refuses_multi_rank_contexts(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    kw = _kw((32, 32, 32), "float", "face")
    world = 2
    lb = mg.Loopback(world)
    errors = []

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(rank=r, world=world, gather_cells=512, device=0, comm_id=b"\0" * 128, **kw),
                             loopback=lb)
            _all_refuse(mg, ctx, ERR_STATE, "single-GPU contexts only")
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
    g = mg.Group(mg.make_opts(**kw), 2, devices=[0, 0])  # a group's rank context
    _all_refuse(mg, g.ranks[0], ERR_STATE, "single-GPU contexts only")
    g.close()
    monkeypatch.setenv("MGP_TRANSPORT", "rccl")  # world 1 on a one-rank RCCL communicator
    rc = mg.Context(mg.make_opts(**kw))
    _all_refuse(mg, rc, ERR_STATE, "single-GPU contexts only")
    rc.close()


def test_debug_names_a_nan_face(monkeypatch):
    _env(monkeypatch, {})
    mg = _mg()
    box = (16, 8, 4)
    ctx = _ctx(box, "float", "face")
    psi, v = _special_fields(box, ctx.dtype, 820)
    ctx.set_psi(psi)
    ctx.set_debug(1)
    ctx.divergence(*v)  # finite: no complaint
    _faces_same(ctx.gradient(*v), pm.subtract(v, pm.gradient(psi, 3, 1.0)), "debug mode keeps the bits")
    bad = [a.copy() for a in v]
    bad[1][2, 3, 5] = np.nan
    with pytest.raises(mg.MGPError) as e:
        ctx.divergence(*bad)
    assert e.value.code == ERR_STATE and "found a nan: mgp_divergence" in str(e.value), str(e.value)
    with pytest.raises(mg.MGPError) as e:
        ctx.gradient(*bad)
    assert e.value.code == ERR_STATE and "found a nan: mgp_gradient, axis 1" in str(e.value), str(e.value)
    bad = [a.copy() for a in v]
    bad[2][4, 7, 15] = np.inf  # the last face of the last axis
    with pytest.raises(mg.MGPError) as e:
        ctx.gradient(*bad)
    assert "found a nan: mgp_gradient, axis 2" in str(e.value), str(e.value)
    ctx.set_debug(0)
    ctx.divergence(*bad)  # not scanned
    ctx.close()
