"""k_zs on levels with a boundary-modified operator (cl != 0): the steps at the box's z faces.

On such a level k_zs's generic steps take the row's table diagonals (the table Markstein division, which equals the
plain one for every such divisor), a chunk at the lower face skips the whole groups of steps whose planes all lie below
the box, and the steady range is not rounded to whole groups of steps, so a steady step may follow a generic one inside
a group and the other way round.  None of it may change a bit: psi and f of every level equal the per-piece kernels'
(MGP_FUSED=0: one launch per half-sweep), the level-0 psi equals the C oracle's after every cycle, the errs of the two
GPU paths agree to 1e-12 relative (the same fp64 sum in another order) and to test_gpu_parity._check_err's bounds
against the oracle.  Every case reads the name and the grid of the launches it means to test from timing_kernels(), so
a case that fell back to other kernels fails.

MGP_FUSED_MIN_CELLS=32768 puts level 1 of the small boxes on k_zs; MGP_ZS_SPLIT_CL stays off there (its default on
fused levels), so that PRE from a fresh guess is k_zs's too.  Shapes (helpers and shapes of test_gpu_zs_split_cl):
128 x 64 x 32 has the one-tile level 1 64 x 32 x 16, one chunk that is both faces: nothing but face steps, no steady
one; 128 x 64 x 128 a level 1 of four 16-plane chunks: lower face, two interior, upper face, with seams; 256 x 128 x 64
a level 1 of 2 x 2 tiles (the x / y / z corner diagonals on the face planes); 128^3 with cycle = F or a warm hierarchy
revisits level 1 with u != 0 (the warm PRE); the world-2 slabs of 128 x 64 x 64 have one box face and one seam each
(the seam is no face: the test is on the global plane); coarse_bc = face / neumann make level 0 itself a cl != 0 level,
which covers POST with the err sum (the C oracle has no such boundary: there the reference is bc_model.py's host model,
as in test_gpu_bc).
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dense_start import dense_start  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
from test_gpu_bc import RBL, _compare  # noqa: E402
from test_gpu_dense import _Run  # noqa: E402
from test_gpu_parity import _check_err  # noqa: E402
from test_gpu_zs_split_cl import BASE, MIN_CELLS, _ctx, _mg, _pair, _run, _same_levels  # noqa: E402

PRE_FRESH = "k_zs<%s, true, 0, true, false, false>"
PRE_WARM = "k_zs<%s, true, 0, false, false, false>"
POST = "k_zs<%s, false, 1, false, false, false>"
POST_ERR = "k_zs<%s, false, 1, true, false, false>"
# threads of a workgroup: the fp32 cl != 0 tile is 64 x 32 in both phases (7 waves PRE, 12 POST); fp64 PRE 32 x 32, POST
# 64 x 16
TILE = {("float", "pre"): (64, 32, 448), ("float", "post"): (64, 32, 768)}
CYCLES = 3


def _env(monkeypatch):
    monkeypatch.setenv("MGP_FUSED", "1")
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", str(MIN_CELLS))
    monkeypatch.setenv("MGP_ZS_SPLIT_CL", "0")


def _wgs(level, tx, ty):
    """Workgroups of a k_zs launch on a level: its tiles times the z-chunks of fused_zc (halved while there are fewer
    than 256 workgroups and a chunk keeps >= 16 planes)."""
    tiles, chunks = (level["nx"] // tx) * (level["ny"] // ty), 1
    while tiles * chunks < 256 and level["nz_local"] // (2 * chunks) >= 16:
        chunks *= 2
    return tiles * chunks


def _launch(level, phase, real="float"):
    tx, ty, ntl = TILE[(real, phase)]
    return _wgs(level, tx, ty) * ntl


def _check(a, b, kw, start=None, cycles=CYCLES):
    """Both contexts and the oracle from the same start: the level-0 psi of either context equals the oracle's after
    every cycle, every level's psi and f are equal between the contexts at the end, the errs agree.  Returns the two
    (timing_read, timing_kernels)."""
    pa, pb = [], []
    ea, ta, ka = _run(a, cycles, start, pa)
    eb, tb, kb = _run(b, cycles, start, pb)
    o = Oracle(threads=8, **kw)
    if start is None:
        o.init_point_charge()
    else:
        start(o)
    eo = []
    for i in range(cycles):
        eo.append(o.step())
        assert np.array_equal(pa[i + 1], o.get(0)), f"k_zs psi differs from the oracle after cycle {i + 1}"
        assert np.array_equal(pb[i + 1], o.get(0)), f"the pieces' psi differs from the oracle after cycle {i + 1}"
    _same_levels(a, b)
    print("err k_zs", ea, "pieces", eb, "oracle", eo)
    np.testing.assert_allclose(ea, eb, rtol=1e-12, atol=0)
    for i in range(cycles):
        _check_err(ea[i], eo[i], pa[i + 1], pa[i])
    assert tb["fused_pre_sub"][1] == 0 and tb["fused_post_sub"][1] == 0, tb  # (the other path is the pieces)
    assert tb["fused_pre"][1] == 0 and tb["fused_post"][1] == 0, tb
    return (ta, ka), (tb, kb)


V_CASES = [((128, 64, 32), 1), ((128, 64, 128), 1), ((256, 128, 64), 2)]


@pytest.mark.parametrize("box,nsub", V_CASES, ids=["one-chunk-both-faces", "four-chunks", "2x2-tiles"])
def test_fused_levels_equal_pieces_and_oracle(box, nsub, monkeypatch):
    """V-cycles: every fused level below the finest (nsub of them) runs k_zs's cl != 0 PRE and POST."""
    _env(monkeypatch)
    kw = dict(BASE, n=box)
    a, b = _pair(monkeypatch, kw, switch="MGP_FUSED")
    eng = [lv["engine"] for lv in a.levels]
    assert eng[:nsub + 1] == ["zs"] * (nsub + 1) and eng[nsub + 1] != "zs", eng
    (ta, ka), _ = _check(a, b, kw)
    assert ta["fused_pre_sub"][1] == CYCLES * nsub and ta["fused_post_sub"][1] == CYCLES * nsub, ta
    # (the last PRE of a cycle is the deepest fused level's, the last POST level 1's)
    assert ka["fused_pre_sub"] == (PRE_FRESH % "float", _launch(a.levels[nsub], "pre")), ka
    assert ka["fused_post_sub"] == (POST % "float", _launch(a.levels[1], "post")), ka


@pytest.mark.parametrize("extra,per_cycle", [(dict(cycle="F"), 2), (dict(coarse_init="warm"), 1)], ids=["F-cycle", "warm"])
def test_warm_pre(extra, per_cycle, monkeypatch):
    """128^3, level 1 = 64^3 (two 32-plane chunks): an F-cycle's second visit and every visit of a warm hierarchy start
    from u != 0, the warm PRE, which has no other kernel than k_zs."""
    _env(monkeypatch)
    kw = dict(BASE, n=(128, 128, 128), **extra)
    a, b = _pair(monkeypatch, kw, switch="MGP_FUSED")
    assert [lv["engine"] for lv in a.levels[:2]] == ["zs", "zs"] and a.levels[2]["engine"] != "zs", a.levels
    (ta, ka), _ = _check(a, b, kw)
    assert ta["fused_pre_sub"][1] == CYCLES * per_cycle and ta["fused_post_sub"][1] == CYCLES * per_cycle, ta
    assert ka["fused_pre_sub"] == (PRE_WARM % "float", _launch(a.levels[1], "pre")), ka
    assert ka["fused_post_sub"] == (POST % "float", _launch(a.levels[1], "post")), ka


def test_dense_start(monkeypatch):
    """From seeded dense random psi and f on the 2 x 2-tile box no load reads a zero for a zero."""
    _env(monkeypatch)
    kw = dict(BASE, n=(256, 128, 64))
    a, b = _pair(monkeypatch, kw, switch="MGP_FUSED")
    seen = []

    def start(x):
        seen.append(dense_start(x, 2002))

    (ta, ka), _ = _check(a, b, kw, start)
    for psi0, f0 in seen:  # the three runs started from the same fields, with no zero cell
        assert np.array_equal(psi0, seen[0][0]) and np.array_equal(f0, seen[0][1])
        assert np.all(psi0 != 0) and np.all(f0 != 0)
    assert np.all(a.get_f(1) != 0) and np.all(np.isfinite(a.get_psi()))
    assert ka["fused_pre_sub"] == (PRE_FRESH % "float", _launch(a.levels[2], "pre")), ka
    assert ka["fused_post_sub"] == (POST % "float", _launch(a.levels[1], "post")), ka


def test_loopback_slabs(monkeypatch):
    """A world-2 split of 128 x 64 x 64: level 1 (64 x 32 x 32, 16 planes per rank) is a distributed fused cl != 0 level;
    rank 0's chunk has the lower box face and a seam above, rank 1's a seam below and the upper face.  The gathered
    psi equals the single domain's pieces and the oracle."""
    _env(monkeypatch)
    box, gather, world = (128, 64, 64), 4096, 2
    cfg = {k: v for k, v in BASE.items() if k != "dim"}
    mg = _mg()
    lb = mg.Loopback(world)
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(dim=3, n=box, rank=r, world=world, gather_cells=gather, device=0,
                                          comm_id=b"\0" * 128, **cfg), loopback=lb)
            ctx.init_point_charge()
            ctx.timing(True)
            psis = []
            for _ in range(CYCLES):
                ctx.cycle()
                psis.append(ctx.get_psi())
            t, k = ctx.timing_read(), ctx.timing_kernels()
            ctx.timing(False)
            ctx._read_levels()
            out[r] = (psis, t, k, ctx.levels)
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
    kw = dict(BASE, n=box)
    monkeypatch.setenv("MGP_FUSED", "0")
    ref = _ctx(**dict(kw, gather_cells=gather))
    ref.init_point_charge()
    o = Oracle(threads=8, **kw)
    o.init_point_charge()
    for i in range(CYCLES):
        ref.cycle()
        o.step()
        psi = np.concatenate([out[r][0][i] for r in range(world)], axis=0)
        assert np.array_equal(psi, o.get(0)), f"the slabs' psi differs from the oracle after cycle {i + 1}"
        assert np.array_equal(psi, ref.get_psi()), f"the slabs' psi differs from the pieces' after cycle {i + 1}"
    for r in range(world):
        _, t, k, levels = out[r]
        assert levels[1]["engine"] == "zs" and levels[1]["distributed"] and levels[1]["nz_local"] == 16, levels[1]
        assert t["fused_pre_sub"][1] == CYCLES and t["fused_post_sub"][1] == CYCLES, t
        assert k["fused_pre_sub"] == (PRE_FRESH % "float", _launch(levels[1], "pre")), k
        assert k["fused_post_sub"] == (POST % "float", _launch(levels[1], "post")), k


def _model_case(monkeypatch, kw, seed):
    """coarse_bc = face / neumann, which the C oracle does not know: the reference is the host model of bc_model.py, as
    in test_gpu_bc (dense fields; after each of 3 cycles psi equal to the model's and the err to _check_err's bounds;
    psi and f of every level equal between k_zs and the pieces and the model).  Then one cycle under timing."""
    a = _Run(monkeypatch, kw, dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=MIN_CELLS))
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert "zs" not in p.engines()
    m = _compare(kw, seed, [a, p], cycles=CYCLES)
    print("err k_zs", a.errs, "pieces", p.errs)
    np.testing.assert_allclose(a.errs, p.errs, rtol=1e-12, atol=0)
    m.cycles(1)
    e, t, k = a.timed_cycle()
    assert np.array_equal(a.ctx.get_psi(), m.cycle_log[0][1])
    assert t["fused_pre"][1] == 1 and t["fused_post"][1] == 1 and t["half_sweep"][1] == 0, t
    return a, t, k


@pytest.mark.parametrize("bc", ["face", "neumann"])
def test_boundary_modified_level0(bc, monkeypatch):
    """coarse_bc = face / neumann on 128 x 64 x 32: level 0 itself has cl != 0 (2 x 2 tiles, two 16-plane chunks, each
    with one face), its PRE starts from psi and its POST sums the err; level 1 is the one chunk with both faces."""
    kw = dict(dim=3, n=(128, 64, 32), real="float", coarse_bc=bc, **RBL)
    a, t, k = _model_case(monkeypatch, kw, 41)
    assert a.engines()[:2] == ["zs", "zs"] and a.engines()[2] != "zs", a.engines()
    assert t["fused_pre_sub"][1] == 1 and t["fused_post_sub"][1] == 1, t
    assert k["fused_pre"] == (PRE_WARM % "float", _launch(a.levels[0], "pre")), k
    assert k["fused_post"] == (POST_ERR % "float", _launch(a.levels[0], "post")), k
    assert k["fused_pre_sub"] == (PRE_FRESH % "float", _launch(a.levels[1], "pre")), k
    assert k["fused_post_sub"] == (POST % "float", _launch(a.levels[1], "post")), k


def test_fp64_boundary_modified_level0(monkeypatch):
    """fp64, coarse_bc = face on 64 x 32 x 32 (level 0 the only fused level, cl != 0, two 16-plane chunks with one face
    each): the double table's Markstein division in the generic steps."""
    kw = dict(dim=3, n=(64, 32, 32), real="double", coarse_bc="face", **RBL)
    a, t, k = _model_case(monkeypatch, kw, 42)
    assert a.engines()[0] == "zs" and a.engines()[1] != "zs", a.engines()
    # (whole waves of up to 1024 threads on the fp64 tiles: 32 x 32 PRE, 64 x 16 POST)
    for kind, name, (tx, ty) in (("fused_pre", PRE_WARM, (32, 32)), ("fused_post", POST_ERR, (64, 16))):
        wgs = _wgs(a.levels[0], tx, ty)
        assert k[kind][0] == name % "double", k
        assert k[kind][1] % (64 * wgs) == 0 and 64 * wgs <= k[kind][1] <= 1024 * wgs, (k, wgs)
