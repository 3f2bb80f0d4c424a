"""The stage-split PRE on levels with a boundary-modified operator (k_zs_split_cl: fp32, cl != 0, the 2^3-average
restriction, a fresh zero guess) against k_zs, the per-piece kernels and the C oracle.

k_zs_split_cl keeps k_zs's expressions and their order (the steady diagonals; the generic steps take the table
Markstein division, which equals the plain one for every such divisor), so the bar is bit identity: psi and f of every
level equal between MGP_ZS_SPLIT_CL=1 and 0 (k_zs; fused levels) or between the default and MGP_ZPOST_PRE=0 (the pieces;
a `zpost` level, whose split PRE does not depend on MGP_ZS_SPLIT_CL), and the level-0 psi equal
to the oracle's (the oracle exposes level 0 only).  The err of the two GPU paths must agree to 1e-12 relative (the same
fp64 sum, whose order may differ); against the oracle, whose sum is sequential, it is held to
test_gpu_parity._check_err's bounds (1e-12 against the pairwise sum of the same arrays, the oracle's own number at its
summation bound), as in the other whole-cycle files.

Every case also reads the "fused_pre_sub" timing kind (the temporally blocked PRE launches of levels >= 1): how many
there were, and the name and grid of the last one.  MGP_FUSED_MIN_CELLS=32768 lets level 1 of the small boxes fuse.

Shapes: 128 x 64 x 32 has the one-tile level 1 64 x 32 x 16 (every face a box face, the shortest chunk: nothing but
face steps); 128 x 64 x 128 a level 1 of four 16-plane chunks (seams; the inner chunks run steady steps only, the last
group partial); 256 x 128 x 64 a level 1 of 2 x 2 tiles (interior tile faces, the corner diagonals on the edge tiles)
and a one-tile level 2; 128^3 with cycle = F or coarse_init = warm revisits level 1 with u != 0, which stays on k_zs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dense_start import dense_start  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
from test_gpu_parity import _check_err  # noqa: E402

SPLIT_CL = "k_zs_split_cl<float>"
KZS_FRESH = "k_zs<float, true, 0, true, false, false>"
KZS_WARM = "k_zs<float, true, 0, false, false, false>"
BASE = dict(dim=3, real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
MIN_CELLS = 32768


def _mg():
    import mgpoisson

    return mgpoisson


def _ctx(**kw):
    mg = _mg()
    return mg.Context(mg.make_opts(**kw))


def _pair(monkeypatch, kw, switch="MGP_ZS_SPLIT_CL"):
    """Contexts with the split kernel on cl != 0 levels and without (the settings are read once, at creation)."""
    monkeypatch.setenv(switch, "1")
    a = _ctx(**kw)
    monkeypatch.setenv(switch, "0")
    b = _ctx(**kw)
    monkeypatch.setenv(switch, "1")
    return a, b


def _fused_env(monkeypatch):
    monkeypatch.setenv("MGP_FUSED", "1")
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", str(MIN_CELLS))
    monkeypatch.setenv("MGP_ZS_SPLIT_CL", "1")  # (off by default on fused levels)


def _grid(level):
    """Work-items of a split launch on a level: 64 x 32 tiles, z-chunks halved while there are fewer than 256
    workgroups and a chunk keeps >= 16 planes (fused_zc), 12 waves each."""
    tiles, chunks = (level["nx"] // 64) * (level["ny"] // 32), 1
    while tiles * chunks < 256 and level["nz_local"] // (2 * chunks) >= 16:
        chunks *= 2
    return tiles * chunks * 768


def _run(x, cycles, start=None, psis=None):
    """`cycles` cycles under timing from the point charge (or start(x)): (errs, timing_read, timing_kernels).
    psis: a list that receives the level-0 psi before the first cycle and after every cycle."""
    if start is None:
        x.init_point_charge()
    else:
        start(x)
    x.timing(True)
    errs = []
    if psis is not None:
        psis.append(x.get_psi())
    for _ in range(cycles):
        errs.append(x.cycle())
        if psis is not None:
            psis.append(x.get_psi())
    t, k = x.timing_read(), x.timing_kernels()
    x.timing(False)
    return errs, t, k


def _same_levels(a, b):
    for level in range(len(a.levels)):
        assert np.array_equal(a.get_psi(level), b.get_psi(level)), f"psi level {level}"
        assert np.array_equal(a.get_f(level), b.get_f(level)), f"f level {level}"


def _oracle_errs(kw, cycles, start=None):
    o = Oracle(threads=8, **kw)
    if start is None:
        o.init_point_charge()
    else:
        start(o)
    return o, [o.step() for _ in range(cycles)]


def _check(a, b, kw, cycles, start=None):
    """Both contexts and the oracle from the same start: psi of level 0 equals the oracle's, every level's psi and f
    are equal between the contexts, the errs agree.  Returns the two (timing_read, timing_kernels)."""
    psis = []
    ea, ta, ka = _run(a, cycles, start, psis)
    eb, tb, kb = _run(b, cycles, start)
    o, eo = _oracle_errs(kw, cycles, start)
    assert np.array_equal(a.get_psi(), o.get(0)), "split psi differs from the oracle"
    assert np.array_equal(b.get_psi(), o.get(0)), "the other path's psi differs from the oracle"
    _same_levels(a, b)
    print("err split", ea, "other", eb, "oracle", eo)
    np.testing.assert_allclose(ea, eb, rtol=1e-12, atol=0)
    for i in range(cycles):
        _check_err(ea[i], eo[i], psis[i + 1], psis[i])
    return (ta, ka), (tb, kb)


V_CASES = [((128, 64, 32), 1), ((128, 64, 128), 1), ((256, 128, 64), 2)]


@pytest.mark.parametrize("box,nsub", V_CASES, ids=["one-tile-16", "four-chunks", "2x2-tiles"])
def test_split_cl_equals_k_zs_and_oracle(box, nsub, monkeypatch):
    """V-cycles from a fresh guess: every fused level below the finest (nsub of them) runs k_zs_split_cl."""
    _fused_env(monkeypatch)
    kw = dict(BASE, n=box)
    a, b = _pair(monkeypatch, kw)
    eng = [lv["engine"] for lv in a.levels]
    assert eng[:nsub + 1] == ["zs"] * (nsub + 1) and eng[nsub + 1] != "zs", eng
    cycles = 2
    (ta, ka), (tb, kb) = _check(a, b, kw, cycles)
    assert ta["fused_pre_sub"][1] == cycles * nsub and tb["fused_pre_sub"][1] == cycles * nsub, (ta, tb)
    assert ta["fused_post_sub"][1] == cycles * nsub, ta
    assert ta["fused_pre"][1] == cycles and ta["fused_post"][1] == cycles, ta  # the level-0 kinds count level 0 only
    assert ka["fused_pre_sub"] == (SPLIT_CL, _grid(a.levels[nsub])), ka
    assert kb["fused_pre_sub"] == (KZS_FRESH, _grid(a.levels[nsub]) // 768 * 448), kb
    assert ka["fused_post_sub"][0].startswith("k_zs<float, false, 1, false, false,"), ka


@pytest.mark.parametrize("extra,per_cycle", [(dict(cycle="F"), 2), (dict(coarse_init="warm"), 1)], ids=["F-cycle", "warm"])
def test_revisits_stay_on_k_zs(extra, per_cycle, monkeypatch):
    """128^3, level 1 = 64^3 fused: an F-cycle's second visit and every visit of a warm hierarchy have u != 0 (or a
    real zero, not a pending one) and take k_zs; the F-cycle's first visit takes the split kernel, and all of it
    still matches MGP_ZS_SPLIT_CL=0 and the oracle."""
    _fused_env(monkeypatch)
    kw = dict(BASE, n=(128, 128, 128), **extra)
    a, b = _pair(monkeypatch, kw)
    eng = [lv["engine"] for lv in a.levels]
    assert eng[:2] == ["zs", "zs"] and eng[2] != "zs", eng
    cycles = 2
    (ta, ka), (tb, kb) = _check(a, b, kw, cycles)
    assert ta["fused_pre_sub"][1] == cycles * per_cycle and tb["fused_pre_sub"][1] == cycles * per_cycle, (ta, tb)
    # the last PRE of level 1 in a cycle is the revisit's
    assert ka["fused_pre_sub"] == (KZS_WARM, _grid(a.levels[1]) // 768 * 448), ka
    assert kb["fused_pre_sub"] == ka["fused_pre_sub"], kb
    if "cycle" in extra:  # the first visit alone (one V-cycle of the same box) is the split kernel's
        v = _ctx(**dict(BASE, n=(128, 128, 128)))
        _, tv, kv = _run(v, 1)
        assert tv["fused_pre_sub"][1] == 1 and kv["fused_pre_sub"] == (SPLIT_CL, _grid(v.levels[1])), (tv, kv)


def test_zpost_level_runs_the_split_pre(monkeypatch):
    """128^3 with level 1 (64^3) as a `zpost` level, as the 256^3 level of the 512^3 box: the engine still reads
    zpost, its PRE is one k_zs_split_cl launch, and psi and f of every level match the per-piece PRE."""
    monkeypatch.setenv("MGP_FUSED", "1")
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", str(1 << 21))
    monkeypatch.setenv("MGP_ZPOST_MIN_CELLS", str(1 << 18))
    kw = dict(BASE, n=(128, 128, 128))
    a, b = _pair(monkeypatch, kw, switch="MGP_ZPOST_PRE")
    for x in (a, b):
        assert [lv["engine"] for lv in x.levels[:2]] == ["zs", "zpost"], x.levels
    cycles = 2
    (ta, ka), (tb, kb) = _check(a, b, kw, cycles)
    assert ta["fused_pre_sub"][1] == cycles and ka["fused_pre_sub"] == (SPLIT_CL, _grid(a.levels[1])), (ta, ka)
    assert tb["fused_pre_sub"][1] == 0 and "fused_pre_sub" not in kb, (tb, kb)
    assert ta["fused_post_sub"][1] == cycles and tb["fused_post_sub"][1] == cycles, (ta, tb)


def test_dense_start(monkeypatch):
    """From seeded dense random psi and f no load reads a zero for a zero: level 1's f is a dense residual."""
    _fused_env(monkeypatch)
    kw = dict(BASE, n=(128, 64, 128))
    a, b = _pair(monkeypatch, kw)
    seen = []

    def start(x):
        psi0, f0 = dense_start(x, 2001)
        seen.append((psi0, f0))

    cycles = 2
    (ta, ka), _ = _check(a, b, kw, cycles, start)
    for psi0, f0 in seen:  # the three runs started from the same fields, with no zero cell
        assert np.array_equal(psi0, seen[0][0]) and np.array_equal(f0, seen[0][1])
        assert np.all(psi0 != 0) and np.all(f0 != 0)
    assert np.all(a.get_f(1) != 0) and np.all(np.isfinite(a.get_psi()))
    assert ka["fused_pre_sub"] == (SPLIT_CL, _grid(a.levels[1])), ka


def test_loopback_slabs(monkeypatch):
    """A world-2 split of 128 x 64 x 64: level 1 (64 x 32 x 32, 16 planes per rank) is a distributed fused cl != 0
    level, whose PRE reads ghost planes.  The gathered psi equals the single domain's on either kernel, and the
    executed exchanges equal the host-only plan (the split changes no ghost plane and no exchange)."""
    from test_gpu_comm import _run as comm_run
    from test_gpu_parity import _loopback_run

    _fused_env(monkeypatch)
    box, gather, cycles = (128, 64, 64), 4096, 2
    cfg = {k: v for k, v in BASE.items() if k != "dim"}
    psi, _, dist = _loopback_run(box, 2, gather, cfg, cycles=cycles)
    assert dist[0] and dist[1]
    kw = dict(BASE, n=box, gather_cells=gather)
    a, b = _pair(monkeypatch, kw)
    assert [lv["engine"] for lv in a.levels[:2]] == ["zs", "zs"]
    (ta, ka), _ = _check(a, b, dict(BASE, n=box), cycles)
    assert ka["fused_pre_sub"][0] == SPLIT_CL, ka
    assert np.array_equal(psi, a.get_psi())
    mg = _mg()
    logs, _ = comm_run(box, 2, dict(cfg, gather_cells=gather), cycles)
    assert logs[0] == logs[1]
    assert logs[0] == mg.plan_comm(mg.make_opts(dim=3, n=box, rank=0, world=2, comm_id=b"\0" * 128, gather_cells=gather,
                                                **cfg), cycles)
    monkeypatch.setenv("MGP_ZS_SPLIT_CL", "0")
    logs0, _ = comm_run(box, 2, dict(cfg, gather_cells=gather), cycles)
    assert logs0[0] == logs[0]
