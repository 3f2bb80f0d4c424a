"""GPU: the batched MAC-grid projection (mgp_batch_divergence, mgp_batch_gradient, mgp_batch_project) against the host
model of project_model.py applied to each member, against an ordinary context per member, and against the separate
batch calls.

Members get different data; B = 5 is odd and no power of two, so a wrong member mapping shows.  Fields are compared bit
for bit (tobytes()).  Faces are passed both as host arrays and as PyTorch tensors by data_ptr().
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import project_model as pm  # noqa: E402
from dense_start import dense_fields  # noqa: E402
from test_gpu_project import _Dev, _faces_same, _ids, _n3, _same, _shape, _special_fields  # noqa: E402

BCS = ("zero", "consistent", "face", "neumann")
RBL = dict(smoother="rbgs", nu1=2, nu2=2, prolong="linear")
ERR_ARG = -1
B5 = 5

# Member boxes (nx, ny[, nz]).  2x2, 4x4, 2^3, 4^3: the scalar form (4x4: 16 slots per member, so member boundaries fall
# inside a wave); 64x16, 16x64: the vector form with one and several items per row; 8^3 (fp32: 64 items per member, a
# workgroup spans four members), 16x8x4, 64x4x2, 32^3: the vector form in 3D; 1x8, 8x1, 1x1x4: one-cell axes.
BOXES_2D = [(2, 2), (4, 4), (64, 16), (16, 64), (1, 8), (8, 1)]
BOXES_3D = [(2, 2, 2), (4, 4, 4), (8, 8, 8), (16, 8, 4), (64, 4, 2), (32, 32, 32), (1, 1, 4)]


def _mg():
    import mgpoisson

    return mgpoisson


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("MGP_TAIL", "MGP_GRAPH", "MGP_PLANE_PAD", "MGP_PAD_BYTES"):
        monkeypatch.delenv(name, raising=False)


def _kw(box, real, bc, **extra):
    return dict(dim=len(box), n=_n3(box), real=real, coarse_bc=bc, **RBL, **extra)


def _batch(box, real, bc, B=B5, **extra):
    mg = _mg()
    return mg.BatchContext(mg.make_opts(**_kw(box, real, bc, **extra)), B)


def _members(box, dt, B, seed):
    """psi (B, nz, ny, nx) and the face arrays [vx, vy, vz | None], member slowest: dense random, different per member,
    with a -0 and a subnormal in each member's arrays."""
    per = [_special_fields(box, dt, seed + 7 * m) for m in range(B)]
    psi = np.stack([p for p, _ in per])
    v = [None if per[0][1][a] is None else np.stack([vm[a] for _, vm in per]) for a in range(3)]
    return psi, v


def _mem(v, m):
    return tuple(None if a is None else a[m] for a in v)


def _stack(per_member):
    return [None if per_member[0][a] is None else np.stack([x[a] for x in per_member]) for a in range(3)]


def _model(psi, v, dim, bc):
    """(f, G psi, v - G psi) of project_model.py applied to each member."""
    B = psi.shape[0]
    want_f = np.stack([pm.divergence(*_mem(v, m), dim) for m in range(B)])
    g = [pm.gradient(psi[m], dim, pm.C0[bc]) for m in range(B)]
    want_g = _stack(g)
    want_w = _stack([pm.subtract(_mem(v, m), g[m]) for m in range(B)])
    return want_f, want_g, want_w


def _no_wall_flow(v, dim):
    """Zero wall faces on every member, as a Neumann projection requires (D v then has zero mean up to rounding)."""
    v[0][..., 0] = v[0][..., -1] = 0
    v[1][..., 0, :] = v[1][..., -1, :] = 0
    if dim == 3:
        v[2][:, 0] = v[2][:, -1] = 0


def _check_operators(b, box, bc, B, seed):
    dim, dt = len(box), b.dtype
    psi, v = _members(box, dt, B, seed)
    want_f, want_g, want_w = _model(psi, v, dim, bc)
    b.set_psi(psi)
    # host memory
    b.divergence(*v)
    assert _same(b.get_f(), want_f), "divergence (host)"
    _faces_same(b.gradient(*v, subtract=False), want_g, "gradient store (host)")
    _faces_same(b.gradient(*v, subtract=True), want_w, "gradient subtract (host)")
    # device memory
    b.set_f(np.ones(b.shape(), dt))
    d = _Dev(v)
    b.divergence_ptr(*d.ptrs)
    assert _same(b.get_f(), want_f), "divergence (device)"
    _faces_same(d.host(), v, "divergence leaves the faces")
    b.gradient_ptr(*d.ptrs, subtract=True)
    _faces_same(d.host(), want_w, "gradient subtract (device)")
    b.gradient_ptr(*d.ptrs, subtract=False)
    _faces_same(d.host(), want_g, "gradient store (device)")
    assert _same(b.get_psi(), psi) and _same(b.get_f(), want_f), "psi and f untouched by the gradient"


# ---- 1. the operators against the model, per member ----

@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", BOXES_2D + BOXES_3D, ids=_ids)
def test_operators_match_the_model(box, real, bc):
    b = _batch(box, real, bc)
    _check_operators(b, box, bc, B5, 900 + sum(box))
    b.close()


def test_operators_many_members_per_workgroup():
    """B = 64 members of 8^3 in fp32: 4096 items, a launch of 16 workgroups with four members in each."""
    box, B = (8, 8, 8), 64
    b = _batch(box, "float", "face", B)
    _check_operators(b, box, "face", B, 940)
    b.close()


# ---- 2. one member at a time ----

@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", [(16, 8, 4), (64, 16)], ids=_ids)
def test_one_member(box, real):
    bc, dim = "face", len(box)
    b = _batch(box, real, bc)
    dt = b.dtype
    psi, v = _members(box, dt, B5, 950)
    want_f, _, _ = _model(psi, v, dim, bc)
    f0 = np.stack([dense_fields(_shape(box), dt, 960 + m)[1] for m in range(B5)])
    b.set_psi(psi)
    all_g = b.gradient(*v, subtract=False)
    all_w = b.gradient(*v, subtract=True)
    for m in (0, 3, 4):
        vm = _mem(v, m)
        for device in (False, True):
            b.set_f(f0)
            if device:
                d = _Dev(vm)
                b.divergence_ptr(*d.ptrs, member=m)
            else:
                b.divergence(*vm, member=m)
            got = b.get_f()
            for o in range(B5):
                assert _same(got[o], want_f[m] if o == m else f0[o]), f"member {m} ({'device' if device else 'host'}): f of {o}"
            assert _same(b.get_f(member=m), want_f[m])
        _faces_same(b.gradient(*vm, subtract=False, member=m), _mem(all_g + (None,), m), f"store, member {m}")
        _faces_same(b.gradient(*vm, subtract=True, member=m), _mem(all_w + (None,), m), f"subtract, member {m}")
        d = _Dev(vm)
        b.gradient_ptr(*d.ptrs, subtract=True, member=m)
        _faces_same(d.host(), _mem(all_w + (None,), m), f"subtract (device), member {m}")
    assert _same(b.get_psi(), psi)
    b.close()


# ---- 3. against an ordinary context ----

@pytest.mark.parametrize("box,real,bc", [((32, 32, 32), "float", "neumann"), ((64, 64), "double", "face")],
                         ids=["3d-f32-neumann", "2d-f64-face"])
def test_members_equal_an_ordinary_context(box, real, bc):
    mg = _mg()
    b = _batch(box, real, bc)
    c = mg.Context(mg.make_opts(**_kw(box, real, bc)))
    psi, v = _members(box, b.dtype, B5, 970)
    b.set_psi(psi)
    b.divergence(*v)
    f = b.get_f()
    g = b.gradient(*v, subtract=False) + (None,)
    w = b.gradient(*v, subtract=True) + (None,)
    for m in range(B5):
        vm = _mem(v, m)
        c.set_psi(psi[m])
        c.divergence(*vm)
        assert _same(f[m], c.get_f()), f"member {m}: f"
        _faces_same(_mem(g, m), c.gradient(*vm, subtract=False), f"member {m}: store")
        _faces_same(_mem(w, m), c.gradient(*vm, subtract=True), f"member {m}: subtract")
    c.close()
    b.close()


# ---- 4. an unaligned device pointer takes the scalar form ----

def test_unaligned_device_pointers():
    import torch

    box, real, bc = (64, 16), "float", "face"
    b = _batch(box, real, bc)
    psi, v = _members(box, b.dtype, B5, 980)
    want_f, want_g, want_w = _model(psi, v, 2, bc)
    b.set_psi(psi)

    def shifted(a):
        """a's values in a tensor whose data_ptr() is 4 bytes off a 16-byte boundary."""
        t = torch.empty(a.size + 1, dtype=torch.float32, device="cuda:0")
        assert t.data_ptr() % 16 == 0
        s = t[1:]
        s.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        assert s.data_ptr() % 16 == 4
        return s

    for which in ("vy", "all"):
        for sub, want in ((True, want_w), (False, want_g)):
            tx = shifted(v[0]) if which == "all" else torch.from_numpy(v[0]).to("cuda:0")
            ty = shifted(v[1])
            torch.cuda.synchronize()
            b.set_f(np.ones(b.shape(), b.dtype))
            b.divergence_ptr(tx.data_ptr(), ty.data_ptr(), None)
            assert _same(b.get_f(), want_f), f"divergence, {which} unaligned"
            b.gradient_ptr(tx.data_ptr(), ty.data_ptr(), None, subtract=sub)
            assert _same(tx.cpu().numpy(), want[0]) and _same(ty.cpu().numpy(), want[1]), f"gradient {sub}, {which} unaligned"
    b.close()


# ---- 5. D(v - G psi) == f - A psi on the device ----

@pytest.mark.parametrize("bc", ["face", "neumann"])
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", [(16, 8, 4), (64, 16)], ids=_ids)
def test_identity_on_the_device(box, real, bc):
    """Dyadic fields: every operation is exact, so the residual of a zero psi against f = D(v - G psi) is the residual
    of psi against f = D v; both sums run over the same cells in the same order."""
    b = _batch(box, real, bc)
    shape, dim, dt = _shape(box), len(box), b.dtype
    rng = np.random.default_rng(990)
    psi = np.stack([pm.dyadic(rng, shape, dt) for _ in range(B5)])
    v = _stack([pm.dyadic_faces(rng, shape, dim, dt) for _ in range(B5)])
    b.set_psi(psi)
    b.divergence(*v)
    rn, _ = b.residual_norm()
    w = b.gradient(*v, subtract=True)
    b.set_psi(np.zeros(b.shape(), dt))
    b.divergence(*w)
    rn2, fn2 = b.residual_norm()
    assert np.all(rn != 0), rn
    assert rn2.tobytes() == fn2.tobytes() == rn.tobytes(), (rn, rn2, fn2)
    b.close()


# ---- 6. mgp_batch_project is the composition of the separate calls ----

def _composition(b, v, bc, fmg, cycles):
    """The separate calls of mgp_batch_project's steps: (faces, rnorm, fnorm)."""
    mg = _mg()
    b.divergence(*v)
    if bc == "neumann":
        b.remove_mean(0, mg.FIELD_F)
    if fmg >= 1:
        b.fmg(fmg, cycles)
    else:
        b.cycles(cycles)
    want = b.gradient(*v, subtract=True)
    rn, fn = b.residual_norm()
    return want, rn, fn


@pytest.mark.parametrize("device_mem", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmg,cycles", [(1, 1), (0, 2), (0, 0)])
@pytest.mark.parametrize("box,real,bc", [((32, 32, 32), "float", "neumann"), ((64, 64), "double", "face")],
                         ids=["3d-f32-neumann", "2d-f64-face"])
def test_project_is_the_composition(box, real, bc, fmg, cycles, device_mem):
    mg = _mg()
    a, b = _batch(box, real, bc), _batch(box, real, bc)
    shape, dim, dt = _shape(box), len(box), a.dtype
    psi0 = np.stack([dense_fields(shape, dt, 1000 + 2 * m)[0] for m in range(B5)])
    rng = np.random.default_rng(1001)
    v = _stack([pm.random_faces(rng, shape, dim, dt) for _ in range(B5)])
    if bc == "neumann":
        _no_wall_flow(v, dim)
    for x in (a, b):
        x.set_psi(psi0)
    if device_mem:
        d = _Dev(v)
        before, after = a.project_ptr(*d.ptrs, fmg=fmg, cycles=cycles)
        faces = d.host()
    else:
        faces, (before, after) = a.project(*v, fmg=fmg, cycles=cycles)
    want, rn, fn = _composition(b, v, bc, fmg, cycles)
    assert _same(a.get_psi(), b.get_psi()) and _same(a.get_f(), b.get_f())
    _faces_same(faces, want, "projected faces")
    assert before.tobytes() == fn.tobytes() and after.tobytes() == rn.tobytes(), (before, fn, after, rn)
    if fmg == 0 and cycles == 0:
        assert _same(a.get_psi(), psi0)
    if fmg >= 1:  # (the dense random psi0 of the warm starts is no guess: its residual is far above ||f||)
        assert np.all(after < before), (before, after)
    # two members against an ordinary context's one call.  Its norms are fp64 sums of the same N non-negative terms in
    # another order: each sum is within N 2^-53 relative of the exact one, so the two norms within N 2^-52
    psi, f = a.get_psi(), a.get_f()
    faces = tuple(faces) + (None,) * (3 - len(faces))
    ncells = int(np.prod(shape))
    c = mg.Context(mg.make_opts(**_kw(box, real, bc)))
    for m in (1, 4):
        c.set_psi(psi0[m])
        cf, (cb, ca) = c.project(*_mem(v, m), fmg=fmg, cycles=cycles)
        assert _same(psi[m], c.get_psi()) and _same(f[m], c.get_f()), f"member {m}: psi, f"
        _faces_same(_mem(faces, m), cf, f"member {m}: faces")
        tol = ncells * 2.0 ** -52
        db, da = abs(before[m] - cb) / cb, abs(after[m] - ca) / ca
        print(f"{_ids(box)} {real} {bc} ({fmg}, {cycles}) member {m}: before {before[m]:.6e} after {after[m]:.6e}, relative "
              f"difference to the ordinary context {db:.3e} / {da:.3e}, bound {tol:.3e}")
        assert db <= tol and da <= tol
    c.close()
    a.close()
    b.close()


# ---- 7. after a per-member stop ----

def test_project_after_a_per_member_stop():
    mg = _mg()
    box, real, bc = (16, 16, 16), "float", "face"
    a, c = _batch(box, real, bc), _batch(box, real, bc)
    shape, dt = _shape(box), a.dtype
    assert a.opts.err_mode == 1
    scale = [1.0, 4.0, 16.0, 64.0, 256.0]  # a member's first err is proportional to its data
    psi0 = np.stack([dense_fields(shape, dt, 1010 + 2 * m)[0] * dt.type(scale[m]) for m in range(B5)])
    f0 = np.stack([dense_fields(shape, dt, 1010 + 2 * m)[1] * dt.type(scale[m]) for m in range(B5)])
    a.set_psi(psi0)
    a.set_f(f0)
    e1 = a.cycles(1)[0]
    order = np.sort(e1)
    eps = float(np.sqrt(order[1] * order[2]))  # between the second and the third smallest recorded err
    a.set_psi(psi0)
    a.set_f(f0)
    iters, _ = a.solve(eps, 2)
    stopped, ran = iters == 1, iters == 2
    assert stopped.any() and ran.any() and (stopped | ran).all(), (e1, eps, iters)
    psi_s, f_s = a.get_psi(), a.get_f()
    c.set_psi(psi_s)
    c.set_f(f_s)
    v = _stack([pm.random_faces(np.random.default_rng(1020 + m), shape, 3, dt) for m in range(B5)])
    faces, (before, after) = a.project(*v, fmg=0, cycles=1)
    want, rn, fn = _composition(c, v, bc, 0, 1)
    psi = a.get_psi()
    for m in range(B5):
        assert not _same(psi[m], psi_s[m]), f"member {m} (iters {iters[m]}) was left out"
    assert _same(psi, c.get_psi()) and _same(a.get_f(), c.get_f())
    _faces_same(faces, want, "projected faces")
    assert before.tobytes() == fn.tobytes() and after.tobytes() == rn.tobytes()
    a.close()
    c.close()


# ---- 8. the solver class ----

def test_solver_class_projects():
    mg = _mg()
    n, B = 32, 3
    s = mg.MultigridHIPBatch(size=n, batch=B, dim=2, real="double", smoother="rbgs", smooth=2, prolong="linear",
                             boundary="neumann")
    rng = np.random.default_rng(1030)
    v = _stack([pm.random_faces(rng, (1, n, n), 2, np.dtype(np.float64)) for _ in range(B)])
    _no_wall_flow(v, 2)
    (wx, wy), (before, after) = s.project(v[0], v[1], fmg=1, cycles=3)
    assert wx.shape == v[0].shape == (B, 1, n, n + 1) and wy.shape == v[1].shape == (B, 1, n + 1, n)
    assert before.shape == after.shape == (B,)
    assert np.all(after < 1e-2 * before), (before, after)  # (a V(2,2) cycle gains more than a factor 5)
    assert _same(wx[..., 0], v[0][..., 0]) and _same(wx[..., -1], v[0][..., -1])  # the walls keep their bits
    assert _same(wy[..., 0, :], v[1][..., 0, :]) and _same(wy[..., -1, :], v[1][..., -1, :])
    with pytest.raises(ValueError, match="shape"):
        s.project(v[1], v[0])
    with pytest.raises(ValueError, match="shape"):
        s.divergence(v[0][0], v[1][0])  # one member's arrays for all members


# ---- 9. refusals ----

def test_refusals():
    mg = _mg()
    lib = mg._lib.lib
    box = (16, 8, 4)
    b = _batch(box, "float", "face")
    psi0 = np.stack([dense_fields(_shape(box), b.dtype, 1040 + 2 * m)[0] for m in range(B5)])
    f0 = np.stack([dense_fields(_shape(box), b.dtype, 1040 + 2 * m)[1] for m in range(B5)])
    b.set_psi(psi0)
    b.set_f(f0)
    buf = np.zeros(1 << 14, np.float32)  # room for any face array of all members
    p = buf.ctypes.data
    h = b._h

    def refused(rc, name, text):
        msg = lib.mgp_batch_last_error(h).decode()
        assert rc == ERR_ARG and name in msg and text in msg, (rc, msg)

    for args in ((None, p, p), (p, None, p), (p, p, None)):
        refused(lib.mgp_batch_divergence(h, -1, *args, 0), "mgp_batch_divergence", "NULL face array")
        refused(lib.mgp_batch_gradient(h, -1, 1, *args, 0), "mgp_batch_gradient", "NULL face array")
        refused(lib.mgp_batch_project(h, *args, 0, 1, 1, None, None), "mgp_batch_project", "NULL face array")
    refused(lib.mgp_batch_divergence(h, -1, p, p, p, 2), "mgp_batch_divergence", "unknown mem")
    refused(lib.mgp_batch_gradient(h, -1, 1, p, p, p, -1), "mgp_batch_gradient", "unknown mem")
    refused(lib.mgp_batch_project(h, p, p, p, 7, 1, 1, None, None), "mgp_batch_project", "unknown mem")
    refused(lib.mgp_batch_gradient(h, -1, 2, p, p, p, 0), "mgp_batch_gradient", "unknown op")
    refused(lib.mgp_batch_gradient(h, -1, -1, p, p, p, 0), "mgp_batch_gradient", "unknown op")
    for member in (-2, B5):
        refused(lib.mgp_batch_divergence(h, member, p, p, p, 0), "mgp_batch_divergence", "member")
        refused(lib.mgp_batch_gradient(h, member, 1, p, p, p, 0), "mgp_batch_gradient", "member")
    refused(lib.mgp_batch_project(h, p, p, p, 0, -1, 1, None, None), "mgp_batch_project", "fmg_cycles >= 0")
    refused(lib.mgp_batch_project(h, p, p, p, 0, 1, -1, None, None), "mgp_batch_project", "cycles >= 0")
    assert _same(b.get_psi(), psi0) and _same(b.get_f(), f0) and not buf.any()  # nothing ran
    with pytest.raises(ValueError, match="shape"):
        b.divergence(np.zeros((B5, 4, 8, 16), np.float32), np.zeros((B5, 4, 9, 16), np.float32),
                     np.zeros((B5, 5, 8, 16), np.float32))
    b.close()
    # 2D ignores vz: NULL succeeds on each entry point
    b2 = _batch((16, 16), "double", "zero", 3)
    vx, vy = np.zeros((3, 1, 16, 17)), np.zeros((3, 1, 17, 16))
    assert lib.mgp_batch_divergence(b2._h, -1, vx.ctypes.data, vy.ctypes.data, None, 0) == 0
    assert lib.mgp_batch_gradient(b2._h, -1, 1, vx.ctypes.data, vy.ctypes.data, None, 0) == 0
    assert lib.mgp_batch_project(b2._h, vx.ctypes.data, vy.ctypes.data, None, 0, 1, 1, None, None) == 0
    b2.close()


# ---- 10. the switches that promise identical bits ----

def test_graph_off_and_tail_off_same_bits(monkeypatch):
    box, real, bc = (32, 32, 32), "float", "face"
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(1050)
    v = _stack([pm.random_faces(rng, _shape(box), 3, dt) for _ in range(B5)])
    out = []
    for env in ({}, dict(MGP_GRAPH="0"), dict(MGP_TAIL="0")):
        for k in ("MGP_GRAPH", "MGP_TAIL"):
            monkeypatch.delenv(k, raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        b = _batch(box, real, bc)
        faces, (before, after) = b.project(*v, fmg=1, cycles=1)
        out.append((b.get_psi().tobytes(), b.get_f().tobytes(), [a.tobytes() for a in faces], before.tobytes(),
                    after.tobytes()))
        b.close()
    assert out[1] == out[0], "MGP_GRAPH=0"
    assert out[2] == out[0], "MGP_TAIL=0"
