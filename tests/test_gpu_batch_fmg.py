"""GPU: the batched full multigrid start (mgp_batch_fmg, mgp_batch_fmg_restrict_rhs, mgp_batch_fmg_prolong) against the
host model of fmg_model.py, stepped on each member's data.

Members get different dense random f (mean-free per member under Neumann, on the host).  Before a call every level's u
and the f of every level >= 1 are NaN on all members: the result must be finite and bit-identical (tobytes()) to the
model on every level's u and f, per member, so nothing stale is read.  An err is a fixed-order fp64 sum on the device
and a sequential one in the model: test_gpu_batch._check_err, as everywhere else.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bc_model import mean_free  # noqa: E402
from dense_start import dense_fields  # noqa: E402
from fmg_model import FmgModel  # noqa: E402
from test_gpu_batch import _check_err  # noqa: E402

ERR_ARG, ERR_STATE = -1, -5
RB = dict(smoother="rbgs", nu1=2, nu2=2)
RBL = dict(prolong="linear", **RB)
BCS = ("zero", "consistent", "face", "neumann")
B5 = 5  # odd and no power of two: a wrong member-to-workgroup mapping shows


def _mg():
    import mgpoisson

    return mgpoisson


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("MGP_TAIL", "MGP_GRAPH"):
        monkeypatch.delenv(name, raising=False)


def _n3(box):
    return tuple(box) + (1,) * (3 - len(box))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _members_f(kw, B, seed):
    """One dense f per member (the f of dense_fields with a seed of its own), mean-free under Neumann."""
    m = FmgModel(**kw)
    f = [dense_fields(m.shapes[0], m.dtype, seed + 2 * i)[1] for i in range(B)]
    if kw.get("coarse_bc") == "neumann":
        f = [mean_free(a) for a in f]
    return np.stack(f)


def _poison(b):
    """NaN in every level's u and in the f of every level >= 1, on all members."""
    for l in range(len(b.levels)):
        nan = np.full(b.shape(None, l), np.nan, b.dtype)
        b.set_psi(nan, level=l)
        if l:
            b.set_f(nan, level=l)


def _start(kw, B, seed):
    """(batch, models, f): f set on level 0 of both, everything else NaN on the device."""
    mg = _mg()
    f = _members_f(kw, B, seed)
    b = mg.BatchContext(mg.make_opts(**kw), B)
    _poison(b)
    b.set_f(f)
    models = [FmgModel(**kw) for _ in range(B)]
    for m, fm in zip(models, f):
        m.f[0] = fm.copy()
    return b, models, f


def _levels_equal(b, models, what):
    for l in range(models[0].nlev):
        u, f = b.get_psi(level=l), b.get_f(level=l)
        assert np.isfinite(u).all() and np.isfinite(f).all(), f"{what}: level {l} is not finite"
        for i, m in enumerate(models):
            assert _same(u[i], m.u[l]), f"{what}: u of level {l}, member {i}"
            assert _same(f[i], m.f[l]), f"{what}: f of level {l}, member {i}"


def _check_errs(errs, wants, models, final):
    assert errs.shape == (final, len(models))
    for i, (m, want) in enumerate(zip(models, wants)):
        assert len(want) == final
        for it in range(final):
            if m.kw["err_mode"]:
                old, new = m.cycle_log[it]
                _check_err(errs[it, i], want[it], new, old)
            else:
                assert np.isnan(errs[it, i])


def _fmg_both(b, models, cycles, final, what="fmg"):
    errs = b.fmg(cycles, final)
    wants = [m.fmg(cycles, final) for m in models]
    _check_errs(errs, wants, models, final)
    _levels_equal(b, models, what)
    mg = _mg()
    if final and models[0].kw["err_mode"]:
        old = b.get_psi_old()
        for i, m in enumerate(models):
            assert _same(old[i], m.psi_old), f"{what}: psiOld of member {i}"
    else:
        with pytest.raises(mg.MGPError) as e:
            b.get_psi_old()
        assert e.value.code == ERR_STATE
    return errs


def _engines(b):
    return [lv["engine"] for lv in b.levels]


# ---- whole mgp_batch_fmg: the smallest shapes that reach each path ----

JAC = dict(smoother="jacobi", prolong="pc")
# id -> (keywords, B, cycles, final, engines asserted for the first levels)
CASES = {
    # T = 0: the whole ascent is one launch
    "2d-8x8-f64-consistent": (dict(dim=2, n=(8, 8, 1), real="double", coarse_bc="consistent", **RBL), B5, 1, 1, ["tail"]),
    # a 4 x 1 coarsest level
    "2d-16x4-f64-neumann": (dict(dim=2, n=(16, 4, 1), real="double", coarse_bc="neumann", **RBL), B5, 1, 1, ["tail"]),
    # a 1 x 1 x 4 coarsest level: the m = 1 ghost rule
    "3d-8x8x32-f32-neumann-c2": (dict(dim=3, n=(8, 8, 32), real="float", coarse_bc="neumann", **RBL), B5, 2, 1, ["tail"]),
    # level 0 per piece with the vector P3 (coarse nx 16), T = 1
    "3d-32^3-f32-face": (dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="face", **RBL), B5, 1, 1, ["piece", "tail"]),
    # nx != ny != nz: the vector P3 over several workgroups per member
    "3d-64x32x16-f32-consistent": (dict(dim=3, n=(64, 32, 16), real="float", coarse_bc="consistent", **RBL), 3, 1, 1,
                                   ["piece", "tail"]),
    "3d-64x32x16-f64-neumann-warm": (dict(dim=3, n=(64, 32, 16), real="double", coarse_bc="neumann", coarse_init="warm",
                                          **RBL), 3, 1, 2, ["piece", "tail"]),
    # two per-piece levels: a cycle between two per-piece P3s
    "3d-64x32x32-f32-face-c2": (dict(dim=3, n=(64, 32, 32), real="float", coarse_bc="face", **RBL), 3, 2, 1,
                                ["piece", "piece", "tail"]),
    # a long F program
    "2d-128^2-f32-F-c2": (dict(dim=2, n=(128, 128, 1), real="float", coarse_bc="consistent", cycle="F", **RBL), B5, 2, 1,
                          ["piece", "tail"]),
    "2d-128^2-f64-warm-V": (dict(dim=2, n=(128, 128, 1), real="double", coarse_bc="consistent", coarse_init="warm", **RBL),
                            B5, 1, 1, ["piece", "tail"]),
    "2d-64^2-f64-jacobi-7+7-pc": (dict(dim=2, n=(64, 64, 1), real="double", nu1=7, nu2=7, **JAC), B5, 1, 1, ["tail"]),
    # odd sweep counts leave results in the Jacobi target buffer: in_t / cur with P3
    "2d-64^2-f64-jacobi-3+2-warm-face": (dict(dim=2, n=(64, 64, 1), real="double", nu1=3, nu2=2, coarse_init="warm",
                                              coarse_bc="face", **JAC), B5, 2, 2, ["tail"]),
    # ... and on per-piece levels above the LDS engine
    "2d-128^2-f64-jacobi-3+2-warm-face": (dict(dim=2, n=(128, 128, 1), real="double", nu1=3, nu2=2, coarse_init="warm",
                                               coarse_bc="face", **JAC), 3, 2, 1, ["piece", "tail"]),
    "3d-16^3-f32-noerr": (dict(dim=3, n=(16, 16, 16), real="float", coarse_bc="face", err_mode=0, **RBL), B5, 1, 2, ["tail"]),
    "3d-32^3-f32-face-final0": (dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="face", cycle="F", **RBL), B5, 1, 0,
                                ["piece", "tail"]),
    "2d-64^2-f64-final2": (dict(dim=2, n=(64, 64, 1), real="double", coarse_bc="consistent", **RBL), B5, 1, 2, ["tail"]),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_fmg_against_the_model(cid):
    kw, B, cycles, final, engines = CASES[cid]
    b, models, _ = _start(kw, B, 700 + sorted(CASES).index(cid))
    assert _engines(b)[:len(engines)] == engines, _engines(b)
    _fmg_both(b, models, cycles, final, cid)
    if engines[0] == "tail":
        assert b.fmg_launches() == 1  # the whole ascent is the LDS launch
    else:
        assert b.fmg_launches() > 1
    b.close()


def test_every_level_per_piece(monkeypatch):
    monkeypatch.setenv("MGP_TAIL", "0")
    kw = dict(dim=3, n=(16, 16, 16), real="double", coarse_bc="consistent", **RBL)
    b, models, _ = _start(kw, B5, 760)
    assert set(_engines(b)) == {"piece"}
    _fmg_both(b, models, 1, 1, "MGP_TAIL=0")
    assert b.fmg_launches() > len(b.levels)
    b.close()


def test_every_level_per_piece_jacobi_odd_sweeps(monkeypatch):
    monkeypatch.setenv("MGP_TAIL", "0")
    kw = dict(dim=2, n=(16, 16, 1), real="double", nu1=3, nu2=2, coarse_init="warm", coarse_bc="neumann", **JAC)
    b, models, _ = _start(kw, B5, 764)
    assert set(_engines(b)) == {"piece"}
    _fmg_both(b, models, 2, 1, "MGP_TAIL=0, Jacobi 3 + 2")
    b.close()


def test_graph_off_same_bits(monkeypatch):
    kw = dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="consistent", **RBL)
    on, models, f = _start(kw, B5, 770)
    e_on = _fmg_both(on, models, 1, 2, "graph")
    monkeypatch.setenv("MGP_GRAPH", "0")
    mg = _mg()
    off = mg.BatchContext(mg.make_opts(**kw), B5)
    _poison(off)
    off.set_f(f)
    e_off = off.fmg(1, 2)
    assert np.array_equal(e_off, e_on)
    _levels_equal(off, models, "MGP_GRAPH=0")
    assert off.fmg_launches() == on.fmg_launches()
    on.close()
    off.close()


@pytest.mark.parametrize("cid", ["3d-32^3-f32-face", "2d-8x8-f64-consistent"])
def test_program_and_graph_follow_cycles_per_level(cid):
    """A second call with another cycles_per_level, then the first again: the cached program and graph are rebuilt."""
    kw, B, _, _, _ = CASES[cid]
    b, models, f = _start(kw, B, 780)
    launches = {}
    for cycles in (1, 2, 1, 1):
        _poison(b)
        b.set_f(f)
        _fmg_both(b, models, cycles, 1, f"cycles_per_level {cycles}")
        assert launches.setdefault(cycles, b.fmg_launches()) == b.fmg_launches()
    b.close()


def test_program_over_the_cap_runs_per_piece():
    """8 x 8: 17 ops per cycles_per_level, so 300 of them are over the 4096-op cap: the LDS levels' ascent runs per piece
    (Jacobi: on target buffers allocated then), with the bits of the model.  Afterwards one cycle per level is the one
    LDS launch again."""
    kw = dict(dim=2, n=(8, 8, 1), real="double", nu1=1, nu2=2, coarse_init="warm", coarse_bc="face", **JAC)
    b, models, f = _start(kw, 2, 790)
    assert set(_engines(b)) == {"tail"}
    _fmg_both(b, models, 300, 1, "over the cap")
    assert b.fmg_launches() > 300
    _poison(b)
    b.set_f(f)
    _fmg_both(b, models, 1, 1, "under the cap again")
    assert b.fmg_launches() == 1
    b.close()


# ---- the pieces on every level ----

BOXES = [(8, 8), (64, 64), (8, 8, 8), (64, 32, 16)]


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("box", BOXES, ids=lambda b: "x".join(map(str, b)))
def test_pieces_on_every_level(box, real, bc):
    mg = _mg()
    kw = dict(dim=len(box), n=_n3(box), real=real, coarse_bc=bc, **RBL)
    B = 3 if box == (64, 32, 16) else B5
    b = mg.BatchContext(mg.make_opts(**kw), B)
    models = [FmgModel(**kw) for _ in range(B)]
    for l in range(models[0].nlev):
        us, fs = [], []
        for i, m in enumerate(models):
            u, f = dense_fields(m.shapes[l], m.dtype, 300 + 20 * i + 2 * l)
            m.u[l], m.f[l] = u.copy(), f.copy()
            us.append(u)
            fs.append(f)
        b.set_psi(np.stack(us), level=l)
        b.set_f(np.stack(fs), level=l)
    for l in range(models[0].nlev - 1):  # f down the hierarchy, each level from the one just written
        b.fmg_restrict_rhs(l)
        for m in models:
            m.fmg_restrict_rhs(l)
    _levels_equal(b, models, "after the restrictions")
    for l in range(models[0].nlev - 2, -1, -1):  # u up the hierarchy
        b.fmg_prolong(l)
        for m in models:
            m.fmg_prolong(l)
        got = b.get_psi(level=l)
        for i, m in enumerate(models):
            assert _same(got[i], m.u[l]), f"prolongation onto level {l} {m.shapes[l]}, member {i}"
    _levels_equal(b, models, "after the prolongations")
    with pytest.raises(mg.MGPError) as e:  # level 0 was replaced
        b.get_psi_old()
    assert e.value.code == ERR_STATE
    b.close()


def test_pieces_run_on_stopped_members():
    """After a solve that stopped every member the pieces still write all of them."""
    mg = _mg()
    kw = dict(dim=2, n=(64, 64, 1), real="float", coarse_bc="face", **RBL)
    b, models, f = _start(kw, B5, 320)
    b.set_psi(np.zeros(b.shape(), b.dtype))
    b.solve(1e30, 5)  # every member stops after its first iteration
    _poison(b)
    us = np.stack([dense_fields(models[0].shapes[1], b.dtype, 330 + i)[0] for i in range(B5)])
    b.set_psi(us, level=1)
    b.fmg_restrict_rhs(0)
    b.fmg_prolong(0)
    for i, m in enumerate(models):
        m.u[1] = us[i].copy()
        m.fmg_restrict_rhs(0)
        m.fmg_prolong(0)
        assert _same(b.get_f(member=i, level=1), m.f[1]) and _same(b.get_psi(member=i), m.u[0]), f"member {i}"
    b.close()


# ---- members ----

def test_member_equals_ordinary_context():
    mg = _mg()
    kw = dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="face", **RBL)
    b, _, f = _start(kw, B5, 800)
    eb = b.fmg(1, 1)
    c = mg.Context(mg.make_opts(**kw))
    c.set_f(f[3])
    ec = c.fmg(1, 1)
    assert _same(b.get_psi(member=3), c.get_psi())
    assert abs(eb[0, 3] - ec[0]) <= 1e-12 * abs(ec[0])
    c.close()
    b.close()


@pytest.mark.parametrize("cid", ["3d-32^3-f32-face", "2d-128^2-f32-F-c2"])
def test_members_are_isolated(cid):
    """Changing member 2's f changes only member 2's fields."""
    kw, B, cycles, _, _ = CASES[cid]
    ref, _, f = _start(kw, B, 810)
    ref.fmg(cycles, 1)
    f2 = f.copy()
    f2[2] = np.inf
    mg = _mg()
    b = mg.BatchContext(mg.make_opts(**kw), B)
    _poison(b)
    b.set_f(f2)
    b.fmg(cycles, 1)
    for l in range(len(b.levels)):
        gu, wu, gf, wf = b.get_psi(level=l), ref.get_psi(level=l), b.get_f(level=l), ref.get_f(level=l)
        for m in (0, 1, 3, 4):
            assert _same(gu[m], wu[m]) and _same(gf[m], wf[m]), f"level {l}, member {m}"
    assert not np.all(np.isfinite(b.get_psi(member=2)))
    ref.close()
    b.close()


@pytest.mark.parametrize("cid", ["3d-64x32x16-f32-consistent", "2d-128^2-f32-F-c2"], ids=["3d", "2d"])
def test_launches_do_not_depend_on_batch(cid):
    kw, _, cycles, _, _ = CASES[cid]
    n = []
    for B in (1, B5):
        b, _, _ = _start(kw, B, 820)
        b.fmg(cycles, 1)
        n.append(b.fmg_launches())
        b.close()
    assert n[0] == n[1] and n[0] > 1


def test_a_stopped_member_is_started_again():
    kw = dict(dim=2, n=(64, 64, 1), real="double", coarse_bc="consistent", **RBL)
    b, models, f = _start(kw, B5, 830)
    b.set_psi(np.zeros(b.shape(), b.dtype))
    iters, _ = b.solve(1e30, 5)  # every member stops after its first iteration
    assert iters.tolist() == [1] * B5
    _poison(b)
    _fmg_both(b, models, 1, 1, "after a solve that stopped everybody")
    b.close()


def test_cycles_and_solve_continue_from_the_models_state():
    kw = dict(dim=3, n=(32, 32, 32), real="float", coarse_bc="face", **RBL)
    b, models, _ = _start(kw, B5, 840)
    _fmg_both(b, models, 1, 0, "final = 0")
    errs = b.cycles(2)
    _check_errs(errs, [m.cycles(2) for m in models], models, 2)
    _levels_equal(b, models, "cycles(2) after fmg")
    old = b.get_psi_old()  # valid again
    for i, m in enumerate(models):
        assert _same(old[i], m.psi_old)
    iters, last = b.solve(0.0, 3)  # (no err is below 0: three iterations each)
    assert iters.tolist() == [3] * B5
    want = [m.cycles(3) for m in models]
    _levels_equal(b, models, "solve after fmg")
    for i, m in enumerate(models):
        _check_err(last[i], want[i][2], m.cycle_log[2][1], m.cycle_log[2][0])
    b.close()


# ---- refusals ----

def test_refusals():
    mg = _mg()
    kw = dict(dim=2, n=(32, 32, 1), real="float", **RBL)
    b, models, f = _start(kw, 3, 850)
    psi = np.stack([dense_fields(models[0].shapes[0], b.dtype, 860 + i)[0] for i in range(3)])
    b.set_psi(psi)
    for c, fin in ((0, 1), (-1, 1), (1, -1)):
        with pytest.raises(mg.MGPError) as e:
            b.fmg(c, fin)
        assert e.value.code == ERR_ARG and "cycles_per_level" in str(e.value), str(e.value)
    for l in (-1, models[0].nlev - 1, models[0].nlev):
        for fn in (b.fmg_restrict_rhs, b.fmg_prolong):
            with pytest.raises(mg.MGPError) as e:
                fn(l)
            assert e.value.code == ERR_ARG and "level" in str(e.value), str(e.value)
    assert _same(b.get_psi(), psi) and _same(b.get_f(), f)  # nothing ran
    b.close()


# ---- the solver class ----

def test_multigrid_hip_batch_fmg_equals_the_solvers():
    mg = _mg()
    build = dict(size=16, dim=3, real="double", smoother="rbgs", smooth=2, prolong="linear", boundary="face")
    B = 3
    f = np.stack([dense_fields((16, 16, 16), np.float64, 870 + 2 * i)[1] for i in range(B)])
    s = mg.MultigridHIPBatch(batch=B, **build)
    s.f = f
    errs = s.fmg(1, 1)
    assert errs.shape == (B,)
    got = s.psi
    for i in range(B):
        one = mg.MultigridHIP(**build)
        one.f = f[i]
        e1 = one.fmg(1, 1)
        assert _same(got[i], one.psi), f"member {i}"
        assert abs(errs[i] - e1) <= 1e-12 * abs(e1)
    assert np.isnan(s.fmg(1, 0)).all()


def test_multigrid_hip_batch_fmg_neumann_removes_the_means():
    """boundary='neumann': every member's f loses its mean first and its psi afterwards.  The batch's and the ordinary
    context's mean reductions sum in different fixed orders, so the means (and with them f) can differ in the last
    bit between the two classes: the class is held, bit for bit, to the same three calls on a BatchContext, whose
    fmg is held to the model above, and to MultigridHIP.fmg per member within the bound below.

    The bound, with N = 4096 cells and eps = 2^-53.  (1) Two fp64 sums of N terms in different orders differ by at most
    2 N eps max|x| in the mean, and RN(x - mean) adds one rounding each: the two f, and likewise the two psi after
    their mean removal, differ by at most (2 N + 2) eps max|.| per cell from that step alone.  (2) One start is a
    linear map of f that approximates the inverse of the Neumann Laplacian on mean-free fields (norm 1 / pi^2 < 1 on
    the unit box; the constant part of a difference in f is annihilated by the final mean removal), so the
    difference in f reaches psi at most once over: (2 N + 2) eps max|f|.  (3) The two runs round differently from
    the first differing bit on: each value of psi is the end of a chain of fewer than N / 2 rounded operations (four
    sweeps, a residual, a restriction, a correction and a cubic interpolation per level visit, two visits of each
    of five levels), at most eps max|psi| each, in both runs: N eps max|psi|.  Together below
    4 N eps (max|f| + max|psi|), about 2e-12 here, where a forgotten mean removal of f (mean about 1e-2) or of psi
    changes psi in its leading digits."""
    mg = _mg()
    build = dict(size=16, dim=3, real="double", smoother="rbgs", smooth=2, prolong="linear", boundary="neumann")
    B = 3
    f = np.stack([dense_fields((16, 16, 16), np.float64, 880 + 2 * i)[1] for i in range(B)])
    s = mg.MultigridHIPBatch(batch=B, **build)
    s.f = f
    errs = s.fmg(1, 1)
    b = mg.BatchContext(mg.make_opts(dim=3, n=(16, 16, 16), real="double", coarse_bc="neumann", **RBL), B)
    b.set_f(f)
    fmeans = b.remove_mean(0, mg.FIELD_F)
    want = b.fmg(1, 1)
    b.remove_mean(0, mg.FIELD_U)
    assert np.allclose(fmeans, f.reshape(B, -1).mean(axis=1), rtol=0, atol=1e-14)
    assert np.array_equal(errs, want[-1])
    assert _same(s.psi, b.get_psi()) and _same(s.f, b.get_f())
    psi = s.psi
    assert np.abs(psi.reshape(B, -1).mean(axis=1)).max() <= 1e-14 * np.abs(psi).max()
    for i in range(B):  # and each member is the ordinary class's answer up to that last bit of the means
        one = mg.MultigridHIP(**build)
        one.f = f[i]
        one.fmg(1, 1)
        diff = np.abs(psi[i] - one.psi).max()
        tol = 4 * 4096 * 2.0 ** -53 * (np.abs(f[i]).max() + np.abs(one.psi).max())
        print("member", i, "max |batch - single|", diff, "bound", tol, "max |psi|", np.abs(one.psi).max(),
              "mean f", f[i].mean())
        assert diff <= tol, (i, diff, tol)
        assert np.abs(one.psi).max() > 1e3 * tol  # (the bound is far below psi itself)
    b.close()
