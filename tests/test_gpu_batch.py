"""Batched solves (mgp_batch_*): B members in one hierarchy against the C oracle stepped on each member's data.

Bar: every member's psi is BIT-IDENTICAL to the oracle's (and so to the ordinary context's); the one reordered
reduction, err, is held to 1e-12 relative to a pairwise (numpy) sum of the same arrays, the project's tolerance for
it (tests/test_gpu_parity.py).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle_lib import Oracle  # noqa: E402

ERR_RTOL = 1e-12
REAL = {"double": np.float64, "float": np.float32}


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


def _rand(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=shape).astype(dtype)


def _shape(kw):
    nx, ny, nz = kw["n"]
    return (nz, ny, nx) if kw["dim"] == 3 else (ny, nx)


RB22 = dict(smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
C_2D_8 = dict(dim=2, n=(8, 8, 1), real="double")  # every level LDS-resident
C_2D_128_WARM = dict(dim=2, n=(128, 128, 1), real="double", coarse_init="warm")  # per-piece levels + the LDS engine
C_2D_128_F32 = dict(dim=2, n=(128, 128, 1), real="float", cycle="F", **RB22)
C_3D_32 = dict(dim=3, n=(32, 32, 32), real="float", cycle="V", **RB22)
C_3D_16 = dict(dim=3, n=(16, 16, 16), real="double", smoother="rbgs", nu1=1, nu2=3, cycle="F", prolong="pc",
               coarse_bc="consistent")
C_3D_BOX = dict(dim=3, n=(32, 16, 8), real="float", **RB22)
# (not in the issue's list) a box whose two finest levels run one launch per piece
C_3D_BOX_PIECE = dict(dim=3, n=(64, 32, 16), real="float", **RB22)
CYCLE_CONFIGS = [C_2D_8, C_2D_128_WARM, C_2D_128_F32, C_3D_32, C_3D_16, C_3D_BOX, C_3D_BOX_PIECE]
B5 = 5  # odd and no power of two: a wrong member-to-workgroup mapping shows


def _member_data(kw, B, seed=100):
    dt = REAL[kw["real"]]
    shp = _shape(kw)
    psi = np.stack([_rand(shp, dt, seed + 2 * m) for m in range(B)])
    f = np.stack([_rand(shp, dt, seed + 2 * m + 1) for m in range(B)])
    return psi, f


def _batch(kw, B, psi, f, **extra):
    mg = _mg()
    b = mg.BatchContext(mg.make_opts(**kw, **extra), B)
    b.set_psi(psi)
    b.set_f(f)
    return b


def _oracles(kw, psi, f):
    out = []
    for m in range(psi.shape[0]):
        o = Oracle(**kw)
        o.set(0, psi[m])
        o.set(1, f[m])
        out.append(o)
    return out


def _step_and_compare(b, oracles, steps=3):
    """steps x cycles(1): every member's psi equals its oracle's bit for bit, its err passes _check_err"""
    for it in range(steps):
        old = [o.get(0) for o in oracles]
        errs = b.cycles(1)
        assert errs.shape == (1, len(oracles))
        got = b.get_psi()
        for m, o in enumerate(oracles):
            e_ref = o.step()
            assert np.array_equal(got[m], o.get(0)), f"cycle {it + 1}, member {m}"
            _check_err(errs[0, m], e_ref, got[m], old[m])
        assert np.array_equal(b.get_psi_old(), np.stack(old))


@pytest.mark.parametrize("kw", CYCLE_CONFIGS, ids=lambda kw: "%dd-%s-%s" % (kw["dim"], "x".join(map(str, kw["n"])), kw["real"]))
def test_cycles_bit_for_bit(kw):
    psi, f = _member_data(kw, B5)
    b = _batch(kw, B5, psi, f)
    assert np.array_equal(b.get_psi(), psi) and np.array_equal(b.get_f(), f)
    assert np.array_equal(b.get_psi(member=3), psi[3]) and np.array_equal(b.get_f(member=4), f[4])
    _step_and_compare(b, _oracles(kw, psi, f))


def test_member_equals_ordinary_context():
    mg = _mg()
    kw = C_3D_32
    psi, f = _member_data(kw, B5)
    b = _batch(kw, B5, psi, f)
    c = mg.Context(mg.make_opts(**kw))
    c.set_psi(psi[3])
    c.set_f(f[3])
    for _ in range(3):
        eb = b.cycles(1)[0, 3]
        ec = c.cycle()
        assert np.array_equal(b.get_psi(member=3), c.get_psi())
        assert abs(eb - ec) <= ERR_RTOL * abs(ec)


def test_per_piece_engine_on_every_level(monkeypatch):
    """MGP_TAIL=0 turns the LDS engine off: the coarse levels down to one cell run one launch per piece"""
    mg = _mg()
    monkeypatch.setenv("MGP_TAIL", "0")
    for kw in (C_3D_16, dict(C_2D_8, n=(16, 16, 1), nu1=3, nu2=2, coarse_init="warm")):
        assert {d["engine"] for d in mg.plan_batch(mg.make_opts(**kw), B5)} == {"piece"}
        psi, f = _member_data(kw, B5)
        _step_and_compare(_batch(kw, B5, psi, f), _oracles(kw, psi, f), steps=2)


@pytest.mark.parametrize("kw", [C_2D_128_WARM, C_3D_32], ids=["2d", "3d"])
def test_cycles_k_in_one_call(kw):
    psi, f = _member_data(kw, B5)
    one = _batch(kw, B5, psi, f)
    e1 = np.concatenate([one.cycles(1) for _ in range(3)])
    many = _batch(kw, B5, psi, f)
    e3 = many.cycles(3)
    assert e3.shape == (3, B5)
    assert np.array_equal(e3, e1)
    assert np.array_equal(many.get_psi(), one.get_psi())


@pytest.mark.parametrize("kw", [C_2D_128_F32, C_3D_32], ids=["2d", "3d"])
def test_members_are_isolated(kw):
    """A kernel that reads across a member boundary lets member 2's inf leak into its neighbours"""
    psi, f = _member_data(kw, B5)
    ref = _batch(kw, B5, psi, f)
    ref.cycles(2)
    f_inf = f.copy()
    f_inf[2] = np.inf
    b = _batch(kw, B5, psi, f_inf)
    b.cycles(2)
    got, want = b.get_psi(), ref.get_psi()
    for m in (0, 1, 3, 4):
        assert np.array_equal(got[m], want[m]), f"member {m}"
    assert not np.all(np.isfinite(got[2]))


@pytest.mark.parametrize("kw", [C_2D_128_F32, C_3D_32], ids=["2d", "3d"])
def test_launches_do_not_depend_on_batch(kw):
    n = []
    for B in (1, 7):
        psi, f = _member_data(kw, B)
        b = _batch(kw, B, psi, f)
        b.cycles(1)
        n.append(b.launches())
    assert n[0] == n[1] and n[0] > 0


# ---- per-member stop (cpu.lua:208-216 per member) -----------------------------------------------------------------

STOP_A = dict(kw=dict(dim=3, n=(16, 16, 16), real="double", cycle="V", **RB22), charges=[-1e6, -1.0, -1e-6, -1e-12],
              epsilon=1e-10, maxiter=50, iters=[13, 7, 2, 1])
STOP_B = dict(kw=dict(dim=2, n=(64, 64, 1), real="float", **RB22), charges=[-1e6, -1.0, -1e-6], epsilon=1e-8, maxiter=50,
              iters=[26, 4, 2])
STOP_C = dict(kw=dict(dim=2, n=(32, 32, 1), real="double"), charges=[-1.0, -1e-6, -1e-12], epsilon=1e-10, maxiter=12,
              iters=[12, 10, 1])


def _charges(kw, charges):
    """f = a point charge of the given value at the centre cell, psi = -f (cpu.lua:180-193 scaled)"""
    shp = _shape(kw)
    f = np.zeros((len(charges),) + shp, REAL[kw["real"]])
    centre = tuple(s // 2 for s in shp)
    for m, q in enumerate(charges):
        f[(m,) + centre] = q
    return -f, f


def _oracle_solve(kw, psi, f, epsilon, maxiter):
    """The cpu.lua break rule on the oracle: (iters, psi at the stop, psi before the last iteration)"""
    o = Oracle(**kw)
    o.set(0, psi)
    o.set(1, f)
    it, old = 0, None
    for it in range(1, maxiter + 1):
        old = o.get(0)
        err = o.step()
        if err < epsilon or not math.isfinite(err):
            break
    return it, o.get(0), old


def _check_stop(case, graph_results=None, **extra):
    kw = case["kw"]
    psi, f = _charges(kw, case["charges"])
    want = [_oracle_solve(kw, psi[m], f[m], case["epsilon"], case["maxiter"]) for m in range(len(psi))]
    assert [w[0] for w in want] == case["iters"]
    assert len(set(case["iters"])) == len(case["iters"])  # the stops really are staggered
    b = _batch(kw, len(psi), psi, f, **extra)
    iters, last = b.solve(case["epsilon"], case["maxiter"])
    got = b.get_psi()
    print("iters", iters.tolist(), "last_err", last.tolist())
    assert iters.tolist() == case["iters"]
    for m, (_, p, old) in enumerate(want):
        assert np.array_equal(got[m], p), f"member {m}"
        d = p.astype(np.float64) - old.astype(np.float64)
        e_pw = float(np.sqrt(np.sum(d * d) / d.size))
        assert abs(last[m] - e_pw) <= ERR_RTOL * abs(e_pw), (m, last[m], e_pw)
    return iters, last, got


@pytest.mark.parametrize("case", [STOP_A, STOP_B, STOP_C], ids=["A", "B", "C"])
def test_per_member_stop(case):
    _check_stop(case)


def test_stop_on_non_finite_err():
    kw = STOP_A["kw"]
    psi, f = _charges(kw, STOP_A["charges"])
    ref = _batch(kw, 4, psi, f)
    it_ref, err_ref = ref.solve(STOP_A["epsilon"], STOP_A["maxiter"])
    f_inf = f.copy()
    f_inf[1] = np.inf
    b = _batch(kw, 4, psi, f_inf)
    iters, last = b.solve(STOP_A["epsilon"], STOP_A["maxiter"])
    assert iters[1] == 1 and not math.isfinite(last[1])
    for m in (0, 2, 3):
        assert iters[m] == it_ref[m] == STOP_A["iters"][m]
        assert last[m] == err_ref[m]
        assert np.array_equal(b.get_psi(member=m), ref.get_psi(member=m))


def test_solve_needs_err_mode():
    mg = _mg()
    b = mg.BatchContext(mg.make_opts(dim=2, n=(16, 16, 1), err_mode=0), 3)
    b.init_point_charge()
    with pytest.raises(mg.MGPError) as ei:
        b.solve(1e-10, 5)
    assert "MGP_ERR_STATE" in str(ei.value)
    assert np.all(np.isnan(b.cycles(2)))


def test_graph_off_same_bits(monkeypatch):
    kw = C_3D_32
    psi, f = _member_data(kw, B5)
    on = _batch(kw, B5, psi, f)
    e_on = on.cycles(3)
    it_on, last_on, psi_on = _check_stop(STOP_A)
    monkeypatch.setenv("MGP_GRAPH", "0")
    off = _batch(kw, B5, psi, f)
    e_off = off.cycles(3)
    assert np.array_equal(e_off, e_on)
    assert np.array_equal(off.get_psi(), on.get_psi())
    assert off.launches() == on.launches()
    it_off, last_off, psi_off = _check_stop(STOP_A)
    assert np.array_equal(it_off, it_on) and np.array_equal(last_off, last_on) and np.array_equal(psi_off, psi_on)


def test_device_buffers():
    import torch

    mg = _mg()
    B = 4
    kw = dict(dim=2, n=(32, 32, 1), real="float", **RB22)
    psi, f = _member_data(kw, B)
    host = _batch(kw, B, psi, f)
    host.cycles(2)
    t_psi = torch.from_numpy(psi).cuda()
    t_f = torch.from_numpy(f).cuda()
    assert t_psi.shape == (B, 32, 32) and t_psi.is_contiguous()
    torch.cuda.synchronize()
    dev = mg.BatchContext(mg.make_opts(**kw), B)
    dev.set_psi_ptr(t_psi.data_ptr())
    dev.set_f_ptr(t_f.data_ptr())
    assert np.array_equal(dev.get_psi(), psi) and np.array_equal(dev.get_f(), f)
    dev.cycles(2)
    assert np.array_equal(dev.get_psi(), host.get_psi())
    out = torch.empty_like(t_psi)
    dev.get_psi_ptr(out.data_ptr())
    assert np.array_equal(out.cpu().numpy(), dev.get_psi())
    one = torch.empty((32, 32), dtype=torch.float32, device="cuda")
    dev.get_f_ptr(one.data_ptr(), member=2)
    assert np.array_equal(one.cpu().numpy(), f[2])


def test_multigrid_hip_batch_equals_three_solvers():
    mg = _mg()
    build = dict(size=16, dim=3, smoother=mg.MultigridHIP.RedBlackGaussSeidel, smooth=2, prolong="linear",
                 coarse_bc="consistent")
    kw = dict(dim=3, n=(16, 16, 16), real="double")
    psi, f = _charges(kw, [-1e6, -1.0, -1e-6])
    s = mg.MultigridHIPBatch(batch=3, **build)
    assert s.psi.shape == (3, 16, 16, 16)
    assert np.array_equal(s.f[0], f[0]) and np.array_equal(s.f[2], f[0])  # cpu.lua's point charge on every member
    s.f = f
    s.psi = psi
    e1 = s.step()
    assert e1.shape == (3,)
    s.f = f
    s.psi = psi
    s.solve()
    got = s.psi
    for m in range(3):
        one = mg.MultigridHIP(**build)
        one.f = f[m]
        one.psi = psi[m]
        it, err = 0, None
        for it in range(1, one.maxiter + 1):  # cpu.lua:208-216
            err = one.step()
            if err < one.epsilon or not math.isfinite(err):
                break
        assert s.iters[m] == it
        assert abs(s.err[m] - err) <= ERR_RTOL * abs(err)
        assert np.array_equal(got[m], one.psi), f"member {m}"
    assert len(set(s.iters.tolist())) == 3


def test_residual_norm_per_member():
    mg = _mg()
    kw = C_3D_32
    psi, f = _member_data(kw, B5)
    b = _batch(kw, B5, psi, f)
    b.cycles(1)
    rn, fn = b.residual_norm()
    for m in range(B5):
        c = mg.Context(mg.make_opts(**kw))
        c.set_psi(psi[m])
        c.set_f(f[m])
        c.cycle()
        r1, f1 = c.residual_norm(0)
        assert abs(rn[m] - r1) <= ERR_RTOL * r1, (m, rn[m], r1)
        assert abs(fn[m] - f1) <= ERR_RTOL * f1, (m, fn[m], f1)
