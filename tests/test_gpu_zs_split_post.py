"""The stage-split POST kernel (k_zs_split_post: fp32, cl = 0, trilinear prolongation, the 128 x 16 tile) against
k_zs and the C oracle.

k_zs_split_post divides k_zs's stages between two groups of waves on 16-byte columns and keeps every expression and
its order, so the bar is bit identity: after each of 3 cycles the level-0 psi equals the oracle's, psi and f of every
level are equal between MGP_ZS_SPLIT_POST=1 and 0 (k_zs), and the errs of the two GPU runs are equal (==): the split
keeps k_zs's per-thread err accumulators and its workgroup sum.  Against the oracle, whose sum is sequential, the err
is held to test_gpu_parity._check_err's bounds.  Every case reads the launched kernel's name and grid: 768 threads per
workgroup, and as many workgroups as k_zs's 832-thread ones.

Every context forces the kernel with MGP_ZS_SPLIT_POST_MIN_CELLS=0 and MGP_FUSED_MIN_CELLS at the box's cell count
(per rank on slabs), so only level 0 is fused unless a case says otherwise.

Shapes: the smallest at which the kernel can go wrong.  The hierarchy takes no 128 x 16 x 32 box (the fused phases
need ny % 32 == 0, PRE's tile height), so the one-tile case is 128 x 32 x 32: 1 x 2 tiles, every x face a box face,
each tile with one y box face, two 16-plane chunks that both touch a z face.  128 x 64 x 32 has 1 x 4 tiles (the two
inner ones with B's d = 1 rows inside the box on both sides); 256 x 32 x 32 has 2 x 2 tiles (the x-halo groups between
tiles); 128 x 32 x 64 has four chunks, the inner two running steady steps through the longer warm-up and drain.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dense_start import dense_start  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
from test_gpu_parity import _check_err  # noqa: E402

SPLIT = "k_zs_split_post<float, true>"
KZS = "k_zs<float, false, 1, true, true, true>"
KZS_SUB = "k_zs<float, false, 1, false, true, false>"
BASE = dict(dim=3, real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", coarse_bc="consistent")
CYCLES = 3
DENSE_SEED = 4107


def _mg():
    import mgpoisson

    return mgpoisson


def _ctx(**kw):
    mg = _mg()
    return mg.Context(mg.make_opts(**kw))


def _cells(box):
    return box[0] * box[1] * box[2]


def _force(monkeypatch, min_cells, split="1", split_min="0"):
    monkeypatch.setenv("MGP_FUSED", "1")
    monkeypatch.setenv("MGP_FUSED_MIN_CELLS", str(min_cells))
    monkeypatch.setenv("MGP_ZS_SPLIT_POST", split)
    monkeypatch.setenv("MGP_ZS_SPLIT_POST_MIN_CELLS", split_min)


def _pair(monkeypatch, kw, min_cells=None):
    """Contexts on the split kernel and on k_zs (the settings are read once, at creation)."""
    _force(monkeypatch, _cells(kw["n"]) if min_cells is None else min_cells)
    a = _ctx(**kw)
    monkeypatch.setenv("MGP_ZS_SPLIT_POST", "0")
    b = _ctx(**kw)
    monkeypatch.setenv("MGP_ZS_SPLIT_POST", "1")
    assert a.levels[0]["engine"] == "zs" and b.levels[0]["engine"] == "zs"
    return a, b


def _workgroups(level):
    """POST's workgroups on a level: 128 x 16 tiles, z-chunks halved while there are fewer than 256 workgroups and a
    chunk keeps >= 16 planes (fused_zc)."""
    tiles, chunks = (level["nx"] // 128) * (level["ny"] // 16), 1
    while tiles * chunks < 256 and level["nz_local"] // (2 * chunks) >= 16:
        chunks *= 2
    return tiles * chunks


def _start(x, start):
    if start is None:
        x.init_point_charge()
    else:
        start(x)


def _run(x, start=None):
    """CYCLES cycles under timing: (errs, the level-0 psi before the first cycle and after every cycle, timing_read,
    timing_kernels)."""
    _start(x, start)
    x.timing(True)
    errs, psis = [], [x.get_psi()]
    for _ in range(CYCLES):
        errs.append(x.cycle())
        psis.append(x.get_psi())
    t, k = x.timing_read(), x.timing_kernels()
    x.timing(False)
    return errs, psis, t, k


def _same_levels(a, b):
    for level in range(len(a.levels)):
        assert np.array_equal(a.get_psi(level), b.get_psi(level)), f"psi level {level}"
        assert np.array_equal(a.get_f(level), b.get_f(level)), f"f level {level}"


def _check(a, b, kw, start=None):
    """The split context, the k_zs context and the oracle from the same start.  Returns the two timing_kernels."""
    ea, pa, _, ka = _run(a, start)
    eb, pb, _, kb = _run(b, start)
    o = Oracle(threads=8, **kw)
    _start(o, start)
    eo = []
    for i in range(CYCLES):
        eo.append(o.step())
        assert np.array_equal(pa[i + 1], o.get(0)), f"split psi differs from the oracle after cycle {i + 1}"
        assert np.array_equal(pb[i + 1], o.get(0)), f"k_zs psi differs from the oracle after cycle {i + 1}"
    _same_levels(a, b)
    print("err split", ea, "k_zs", eb, "oracle", eo)
    assert ea == eb
    for i in range(CYCLES):
        _check_err(ea[i], eo[i], pa[i + 1], pa[i])
    wg = _workgroups(a.levels[0])
    assert ka["fused_post"] == (SPLIT, wg * 768), ka
    assert kb["fused_post"] == (KZS, wg * 832), kb
    return ka, kb


V_CASES = [(128, 32, 32), (128, 64, 32), (256, 32, 32), (128, 32, 64)]


@pytest.mark.parametrize("box", V_CASES, ids=["one-tile-column", "tiles-in-y", "2x2-tiles", "four-chunks"])
def test_split_post_equals_k_zs_and_oracle(box, monkeypatch):
    kw = dict(BASE, n=box)
    a, b = _pair(monkeypatch, kw)
    _check(a, b, kw)


@pytest.mark.parametrize("extra", [dict(cycle="F"), dict(coarse_init="warm")], ids=["F-cycle", "warm"])
def test_split_post_cycle_kinds(extra, monkeypatch):
    kw = dict(BASE, n=(128, 64, 32), **extra)
    a, b = _pair(monkeypatch, kw)
    _check(a, b, kw)


def test_split_post_dense_start(monkeypatch):
    """From seeded dense random psi and f no load reads a zero for a zero."""
    kw = dict(BASE, n=(128, 64, 32))
    a, b = _pair(monkeypatch, kw)
    seen = []

    def start(x):
        seen.append(dense_start(x, DENSE_SEED))

    _check(a, b, kw, start)
    for psi0, f0 in seen:  # the three runs started from the same fields, with no zero cell
        assert np.array_equal(psi0, seen[0][0]) and np.array_equal(f0, seen[0][1])
        assert np.all(psi0 != 0) and np.all(f0 != 0)
    assert np.all(np.isfinite(a.get_psi()))


def test_split_post_zero_bc_sub_level(monkeypatch):
    """128^3 with coarse_bc = zero: every level has cl = 0 and the 64^3 level is fused too.  The wide tile does not
    divide it, so its POST (fused_post_sub) stays on k_zs while level 0 takes the split kernel."""
    kw = dict(BASE, n=(128, 128, 128), coarse_bc="zero")
    a, b = _pair(monkeypatch, kw, min_cells=64 ** 3)
    assert [lv["engine"] for lv in a.levels[:2]] == ["zs", "zs"]
    ka, kb = _check(a, b, kw)
    # 64 x 32 tiles in four 16-plane chunks, 18 x 40 threads in 12 waves
    assert ka["fused_post_sub"] == (KZS_SUB, (64 // 64) * (64 // 32) * 4 * 768), ka
    assert kb["fused_post_sub"] == ka["fused_post_sub"], kb


def _loopback(box, world, gather, cfg, cycles):
    """`world` loopback ranks: (the slabs' psi joined, the errs, timing_kernels of every rank)."""
    import threading

    mg = _mg()
    lb = mg.Loopback(world)
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(dim=3, n=box, rank=r, world=world, gather_cells=gather, device=0,
                                          comm_id=b"\0" * 128, **cfg), loopback=lb)
            ctx.init_point_charge()
            ctx.timing(True)
            errs = [ctx.cycle() for _ in range(cycles)]
            k = ctx.timing_kernels()
            ctx.timing(False)
            out[r] = (ctx.get_psi(), errs, k)
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
    assert all(o[1] == out[0][1] for o in out)  # every rank holds the global err
    return np.concatenate([o[0] for o in out], axis=0), out[0][1], [o[2] for o in out]


def test_split_post_loopback_slabs(monkeypatch):
    """A world-2 split of 128 x 64 x 64 (ghost planes as the z-halo of every slab's level 0): the gathered psi and the
    errs equal the single domain's on either kernel, and equal the slabs' on k_zs."""
    from test_gpu_parity import _loopback_run

    box, gather = (128, 64, 64), 4096
    cfg = {k: v for k, v in BASE.items() if k != "dim"}
    _force(monkeypatch, _cells(box) // 2)
    psi, errs, ks = _loopback(box, 2, gather, cfg, CYCLES)
    wg = 4 * 2  # 1 x 4 tiles, 32 planes per rank in two chunks
    for k in ks:
        assert k["fused_post"] == (SPLIT, wg * 768), k
    monkeypatch.setenv("MGP_ZS_SPLIT_POST", "0")
    psi0, errs0, ks0 = _loopback(box, 2, gather, cfg, CYCLES)
    assert ks0[0]["fused_post"] == (KZS, wg * 832), ks0
    assert np.array_equal(psi, psi0) and errs == errs0
    monkeypatch.setenv("MGP_ZS_SPLIT_POST", "1")
    psi_h, _, dist = _loopback_run(box, 2, gather, cfg, cycles=CYCLES)  # the shared helper: the same answer
    assert dist[0] and np.array_equal(psi, psi_h)
    kw = dict(BASE, n=box, gather_cells=gather)
    a, b = _pair(monkeypatch, kw, min_cells=_cells(box) // 2)
    _check(a, b, dict(BASE, n=box))
    assert np.array_equal(psi, a.get_psi())


def _post_name(kw):
    x = _ctx(**kw)
    x.init_point_charge()
    x.timing(True)
    x.cycle()
    name = x.timing_kernels()["fused_post"][0]
    x.timing(False)
    return name


def test_split_post_selection(monkeypatch):
    """MGP_ZS_SPLIT_POST_MIN_CELLS is a level-size threshold; the default leaves a small box on k_zs."""
    box = (128, 64, 32)
    kw = dict(BASE, n=box)
    _force(monkeypatch, _cells(box), split_min=str(_cells(box)))
    assert _post_name(kw) == SPLIT
    _force(monkeypatch, _cells(box), split_min=str(_cells(box) + 1))
    assert _post_name(kw) == KZS
    _force(monkeypatch, _cells(box), split="0", split_min="0")
    assert _post_name(kw) == KZS
    monkeypatch.delenv("MGP_ZS_SPLIT_POST")
    monkeypatch.delenv("MGP_ZS_SPLIT_POST_MIN_CELLS")
    assert _post_name(kw) == KZS
