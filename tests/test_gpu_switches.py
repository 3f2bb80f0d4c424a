"""GPU: the switches README promises identical bits for, and the kernel forms a level's size selects, that no other
fast test runs.

Every whole-cycle case starts from dense_start() (test_gpu_dense.py's pattern: _Run / _compare, psi bit-identical to the
C oracle after every cycle, psi and f of every level bit-identical to the reference run, err by
test_gpu_parity._check_err); every case is in dense_start.CASES, so test_dense_inputs.py holds the reference to its
conditions on it.

  1. The tile-patch order of the fused phases (zs_patch on the host, zs_tile_xy on the device, mgp_zs.h): launches of
     1024 workgroups, patched on k_zs_split PRE and k_zs_split_post, k_zs POST on the wide and on the narrow tile, k_zs
     PRE, the PRE with the full weighting fused, and fp64 PRE and POST.  A wrong patch map runs one tile twice and
     another never; from the dense start no tile is all zeros.  The patches of the cl != 0 kernels (k_zs_split_cl,
     k_zs<..., false>) would need a level 1 of more than 512 workgroups, that is a level 0 of 2^28 cells: not run here.
     They go through the same zs_tile_xy.
  2. MGP_ZS_POST_ZC, the only rule that gives POST another z-chunk count than PRE.
  3. MGP_PLANE_PAD: Geo::P != nx * ny on level 0, on every level-0 engine, and in the reductions, plane transfers and
     the refinement step.
  4. The host-path switches MGP_LAZY_ZERO_FUSED, MGP_ERRS_HOST, MGP_PRECAPTURE, MGP_TAIL_CELLS, MGP_BLK_CELLS.
  5. The per-piece kernel forms a context reads at creation: MGP_RR_SCALAR_CELLS (the vector residual + restriction),
     MGP_RR_PAIR_CELLS (the pair form), MGP_BRES_VN, MGP_NT.  The library keeps no launch record of per-piece kernels
     below the finest level; that these settings select the forms is shown by a kernel trace of this file, not here.
  6. mgp_residual_restrict called directly on the scalar, pair and vector forms at their edge shapes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dense_start import RESET_SEED_OFFSET, case, dense_fields, dense_start, oracle_kw  # noqa: E402
from oracle_lib import Oracle, coarse_coef, residual_arr, restrict_arr  # noqa: E402
from test_gpu_dense import SPLIT_NAME, _compare, _env, _loopback_dense, _mg, _Run, _timed_check  # noqa: E402
from test_gpu_parity import _check_err  # noqa: E402

KZS_PRE = "k_zs<float, true, 0, false, true, false>"
KZS_PRE_FWF = "k_zs<float, true, 2, false, true, false>"
KZS_POST_WIDE = "k_zs<float, false, 1, true, true, true>"
KZS_POST_NARROW = "k_zs<float, false, 1, true, true, false>"
SPLIT_POST = "k_zs_split_post<float, true>"
KZS_PRE_F64 = "k_zs<double, true, 0, false, true, false>"
KZS_POST_F64 = "k_zs<double, false, 1, true, true, false>"

PIECES = dict(MGP_TAIL=0, MGP_BLK=0, MGP_FUSED=0)  # every level runs one launch per piece


def _close(*runs):
    for r in runs:
        r.ctx.close()


# ---- 1. the tile-patch order ----

@pytest.fixture(scope="module")
def patch_refs():
    """Per case, computed once and shared unchanged: the oracle's psi before and after each of 2 cycles with its errs,
    and every level's psi and f (and the errs) of the patch-off GPU run after those 2 cycles."""
    cache = {}

    def get(cid, base):
        if cid not in cache:
            kw, seed = case(cid)
            o = Oracle(threads=8, **oracle_kw(kw))
            psis, errs = [dense_start(o, seed)[0]], []
            for _ in range(2):
                errs.append(o.step())
                psis.append(o.get(0))
            del o
            with pytest.MonkeyPatch.context() as mp:
                off = _Run(mp, kw, dict(base, MGP_ZS_PATCH=0))
                dense_start(off.ctx, seed)
                off_errs = [off.cycle() for _ in range(2)]
                assert np.array_equal(off.ctx.get_psi(), psis[2]), "patch-off psi differs from the oracle"
                levels = [(off.ctx.get_psi(l), off.ctx.get_f(l)) for l in range(len(off.levels))]
                _close(off)
            cache[cid] = (psis, errs, levels, off_errs)
        return cache[cid]

    yield get
    cache.clear()


def _workgroups(monkeypatch, env, small, kernels, grids):
    """The launches' workgroup counts: each phase's grid over the same kernel's grid per workgroup, which a small box
    of a known workgroup count gives under the same switches.  small: (case, workgroups) for PRE and for POST."""
    out = []
    for kind, (cid, wgs), name, grid in zip(("fused_pre", "fused_post"), small, kernels, grids):
        kw, seed = case(cid)
        s = _Run(monkeypatch, kw, dict(env, MGP_FUSED_MIN_CELLS=kw["n"][0] * kw["n"][1] * kw["n"][2]))
        assert s.engines()[0] == "zs"
        dense_start(s.ctx, seed)
        k = s.timed_cycle()[2]
        _close(s)
        assert k[kind][0] == name, (k, name)
        assert k[kind][1] % (64 * wgs) == 0, k
        out.append(grid / (k[kind][1] // wgs))
    return out


# PRE's one tile of 64 x 32 x 16; POST's wide tile needs nx % 128 == 0: 128 x 64 x 32 in 16-plane chunks has
# 1 x 4 x 2 = 8 wide (128 x 16) and 2 x 2 x 2 = 8 narrow (64 x 32) workgroups
SMALL_F32 = (("zs-64x32x16", 1), ("zs-128x64x32", 8))
SMALL_FW = (("fw-zs-64x32x16", 1), ("fw-zs-128x64x32", 8))
SMALL_F64 = (("zs-f64-64x32x16", 2), ("zs-f64-64x32x16", 2))  # fp64 tiles: PRE 32 x 32 (2 x 1), POST 64 x 16 (1 x 2)


def _patched(patch_refs, monkeypatch, cid, base, env, pre, post, small=SMALL_F32):
    kw, seed = case(cid)
    psis, oerrs, levels, off_errs = patch_refs(cid, base)
    r = _Run(monkeypatch, kw, dict(base, **env))
    assert r.engines()[0] == "zs"
    dense_start(r.ctx, seed)
    e1 = r.cycle()  # graph replay
    assert np.array_equal(r.ctx.get_psi(), psis[1]), f"{env}: psi differs after cycle 1"
    e2, t, k = r.timed_cycle()  # eager, timed
    assert np.array_equal(r.ctx.get_psi(), psis[2]), f"{env}: psi differs after cycle 2"
    for it, e in enumerate((e1, e2)):
        print(f"{cid} {env}: err {e!r}, oracle {oerrs[it]!r}, patch off {off_errs[it]!r}")
        _check_err(e, oerrs[it], psis[it + 1], psis[it])
        assert abs(e - off_errs[it]) <= 1e-12 * abs(off_errs[it])
    assert t["fused_pre"][1] == 1 and t["fused_post"][1] == 1 and t["half_sweep"][1] == 0, t
    assert k["fused_pre"][0] == pre and k["fused_post"][0] == post, k
    assert len(r.levels) == len(levels)
    for l, (psi, f) in enumerate(levels):
        assert np.array_equal(r.ctx.get_psi(l), psi), f"{env}: psi level {l}"
        assert np.array_equal(r.ctx.get_f(l), f), f"{env}: f level {l}"
    _close(r)
    wg = _workgroups(monkeypatch, dict(base, **env), small, (pre, post), (k["fused_pre"][1], k["fused_post"][1]))
    assert wg == [1024, 1024], (wg, k)  # zs_patch needs more than 512


# 16-plane chunks and 1024 workgroups on the 64 x 32 tile (8 x 16 tiles) and on the 128 x 16 tile (4 x 32 tiles)
F32_BASE = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536, MGP_ZS_WGS=1024)
F32_TILES = {SPLIT_NAME: (8, 16), KZS_PRE: (8, 16), KZS_PRE_FWF: (8, 16), KZS_POST_NARROW: (8, 16),
             KZS_POST_WIDE: (4, 32), SPLIT_POST: (4, 32)}


def _parse(v):
    return tuple(int(x) for x in v.split(","))


@pytest.mark.parametrize("env,pre,post,divides", [
    (dict(MGP_ZS_PATCH="4,8", MGP_ZS_SPLIT_POST_MIN_CELLS=0), SPLIT_NAME, SPLIT_POST, True),
    (dict(MGP_ZS_PATCH_POST="2,2", MGP_ZS_SPLIT_POST=0), SPLIT_NAME, KZS_POST_WIDE, True),
    (dict(MGP_ZS_WIDE=0, MGP_ZS_PATCH_POST="4,8"), SPLIT_NAME, KZS_POST_NARROW, True),
    (dict(MGP_ZS_SPLIT=0, MGP_ZS_PATCH_PRE="2,2"), KZS_PRE, KZS_POST_WIDE, True),
    # 3 x 3 divides neither tile count: zs_patch falls back to tile rows
    (dict(MGP_ZS_PATCH="3,3"), SPLIT_NAME, KZS_POST_WIDE, False),
], ids=["split-pre-and-split-post-4x8", "k_zs-post-wide-2x2", "k_zs-post-narrow-4x8", "k_zs-pre-2x2", "3x3-falls-back"])
def test_patch_order_fp32(env, pre, post, divides, patch_refs, monkeypatch):
    for key, name in (("MGP_ZS_PATCH_PRE", pre), ("MGP_ZS_PATCH_POST", post)):
        v = env.get(key, env.get("MGP_ZS_PATCH"))
        if v is not None:
            px, py = _parse(v)
            tx, ty = F32_TILES[name]
            assert (tx % px == 0 and ty % py == 0) == divides, (name, v)
    _patched(patch_refs, monkeypatch, "patch-512x512x128-f32", F32_BASE, env, pre, post)


def test_patch_order_fused_full_weighting(patch_refs, monkeypatch):
    assert F32_TILES[KZS_PRE_FWF][0] % 2 == 0 and F32_TILES[KZS_PRE_FWF][1] % 2 == 0
    _patched(patch_refs, monkeypatch, "patch-fw-512x512x128-f32", F32_BASE, dict(MGP_ZS_PATCH="2,2"), KZS_PRE_FWF,
             KZS_POST_WIDE, small=SMALL_FW)


@pytest.mark.parametrize("patch", ["2,2", "4,8"])
def test_patch_order_fp64(patch, patch_refs, monkeypatch):
    """fp64 256^3 in 16-plane chunks: PRE has 8 x 8 tiles of 32 x 32, POST 4 x 16 tiles of 64 x 16, 1024 workgroups
    each; both patches divide both.  (64 x 32 x 16 has 2 x 1 and 1 x 2 of those tiles.)"""
    px, py = _parse(patch)
    assert 8 % px == 0 and 8 % py == 0 and 4 % px == 0 and 16 % py == 0
    base = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=1 << 24, MGP_ZS_WGS=1024)
    _patched(patch_refs, monkeypatch, "patch-256-f64", base, dict(MGP_ZS_PATCH=patch), KZS_PRE_F64, KZS_POST_F64,
             small=SMALL_F64)


# ---- 2. MGP_ZS_POST_ZC ----

def test_post_zc_chunks_post_apart_from_pre(monkeypatch):
    """64 x 32 x 64 with MGP_ZS_WGS=1: PRE runs its one tile as one 64-plane chunk, and POST's one tile as 4, 2, 1 and
    (unset: 256 planes) 1 chunks."""
    kw, seed = case("zs-64x32x64")
    base = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536, MGP_ZS_WGS=1)
    runs = [_Run(monkeypatch, kw, dict(base, MGP_ZS_POST_ZC=v)) for v in (16, 32, 0)] + [_Run(monkeypatch, kw, base)]
    assert all(r.engines()[0] == "zs" for r in runs)
    o = _compare(kw, seed, runs, cycles=3)
    ks = _timed_check(kw, o, *[(r, SPLIT_NAME, KZS_POST_NARROW) for r in runs])
    pre = [k["fused_pre"][1] for k in ks]
    post = [k["fused_post"][1] for k in ks]
    print("fused_pre grids", pre, "fused_post grids", post)
    assert pre == [768] * 4  # one workgroup of k_zs_split's 12 waves: one chunk
    assert post[3] > 0 and post[:3] == [4 * post[3], 2 * post[3], post[3]], post
    _close(*runs)


# ---- 3. MGP_PLANE_PAD ----

PAD = 4352
ZS = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536)


@pytest.mark.parametrize("cid,env,kernels", [
    ("pad-256x256x16-f32", dict(ZS, MGP_ZS_SPLIT=1), (SPLIT_NAME, KZS_POST_WIDE)),
    ("pad-256x256x16-f32", dict(ZS, MGP_ZS_SPLIT=0), (KZS_PRE, KZS_POST_WIDE)),
    ("pad-256x256x16-f64", ZS, (KZS_PRE_F64, KZS_POST_F64)),
    ("pad-256x256x16-f32", dict(MGP_FUSED=0), None),
    ("pad-256x256x16-f64", dict(MGP_FUSED=0), None),
    ("pad-256x256x16-f64-jacobi", dict(), None),
    ("pad-256x256x16-f32-fw", ZS, (KZS_PRE_FWF, KZS_POST_WIDE)),
    ("pad-256x256x16-f32-fw", dict(MGP_FUSED=0), None),
    ("pad-256x256x16-f32-fw", dict(MGP_FUSED=0, MGP_RESFW=0), None),
    ("pad-256x256x16-f64-gslex", dict(), None),
], ids=["k_zs_split", "k_zs-f32", "k_zs-f64", "piece-rb-f32", "piece-rb-f64", "piece-jacobi-f64", "fw-fused", "fw-k_resfw",
        "fw-two-pass", "gs_lex"])
def test_plane_pad_level0_engines(cid, env, kernels, monkeypatch):
    """Level 0's planes hold 2^16 slots, so MGP_PLANE_PAD makes its plane stride nx * ny + 4352 / sizeof(real): the
    padded and the unpadded context both equal the oracle."""
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(env, MGP_PLANE_PAD=PAD))
    p = _Run(monkeypatch, kw, env)
    assert a.engines() == p.engines() and a.engines()[0] == ("zs" if kernels else "piece"), a.engines()
    o = _compare(kw, seed, [a, p], cycles=2)
    assert a.errs == p.errs  # the same sums in the same order: the pad slots are no part of them
    if kernels:
        _timed_check(kw, o, (a, *kernels), (p, *kernels))
    _close(a, p)


@pytest.mark.parametrize("cid", ["pad-256x256x16-f32", "pad-256x256x16-f64"])
def test_plane_pad_reductions_and_plane_transfers(cid, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(MGP_PLANE_PAD=PAD))
    p = _Run(monkeypatch, kw, dict())
    psi0, f0 = dense_start(a.ctx, seed)
    dense_start(p.ctx, seed)
    for which in (0, 1):
        assert a.ctx.field_stats(which) == p.ctx.field_stats(which)
    assert a.ctx.residual_norm() == p.ctx.residual_norm()
    assert a.cycle() == p.cycle()
    assert np.array_equal(a.ctx.get_psi(), p.ctx.get_psi())
    assert a.ctx.metrics() == p.ctx.metrics()
    assert a.ctx.field_stats() == p.ctx.field_stats() and a.ctx.residual_norm() == p.ctx.residual_norm()
    # planes 3 .. 7 set, planes 2 .. 8 read back: the planes set between their untouched neighbours
    new = dense_fields((5,) + psi0.shape[1:], psi0.dtype, seed + 2)[0]
    for r in (a, p):
        before = r.ctx.get_psi()
        r.ctx.set_planes(0, 3, new)
        want = before.copy()
        want[3:8] = new
        assert np.array_equal(r.ctx.get_planes(0, 2, 7), want[2:9])
        assert np.array_equal(r.ctx.get_psi(), want)
        assert np.array_equal(r.ctx.get_planes(1, 0, 16), f0) and np.array_equal(r.ctx.get_f(), f0)
    assert a.ctx.field_stats() == p.ctx.field_stats()
    _close(a, p)


def test_plane_pad_refine_step(monkeypatch):
    mg = _mg()
    kw, seed = case("pad-256x256x16-f32")
    a = _Run(monkeypatch, kw, dict(MGP_PLANE_PAD=PAD))
    p = _Run(monkeypatch, kw, dict())
    out = []
    for r in (a, p):
        dense_start(r.ctx, seed)
        _env(monkeypatch, r.env)
        r.ctx.refine_begin()
        step = r.ctx.refine_step(2)
        out.append((step, r.ctx.refine_get(mg._lib.REFINE_PSI), r.ctx.refine_residual()))
        r.ctx.refine_end()
    print("refine_step padded", out[0][0], "unpadded", out[1][0])
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2]
    assert np.array_equal(out[0][1], out[1][1])
    assert np.all(np.isfinite(out[0][1])) and not np.array_equal(out[0][1], dense_fields(out[0][1].shape, np.float32, seed)[0])
    _close(a, p)


@pytest.mark.parametrize("pad", [PAD, None], ids=["padded", "unpadded"])
def test_plane_pad_loopback_slabs(pad, monkeypatch):
    """World 2 on 256 x 256 x 32: each rank's 16 planes of level 0 take the padded stride, ghost planes included."""
    kw, seed = case("pad-slab-256x256x32-f32")
    env = dict(ZS) if pad is None else dict(ZS, MGP_PLANE_PAD=pad)
    _env(monkeypatch, env)
    psi, errs = _loopback_dense(kw["n"], 2, 4096, {k: v for k, v in kw.items() if k != "n"}, seed, cycles=2,
                                expect_fused=True)
    o = Oracle(threads=8, **oracle_kw(kw))
    dense_start(o, seed)
    es = []
    for _ in range(2):
        old = o.get(0)
        eo = o.step()
        es.append(eo)
        for e in errs:
            _check_err(e[len(es) - 1], eo, o.get(0), old)
    assert np.array_equal(psi, o.get(0)), "gathered slab psi differs from the oracle"


# ---- 4. the host-path switches ----

def test_lazy_zero_fused_off(monkeypatch):
    kw, seed = case("zs-128")
    zz = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536, MGP_ZPOST_MIN_CELLS=1 << 40)
    a = _Run(monkeypatch, kw, dict(zz, MGP_LAZY_ZERO_FUSED=0))
    d = _Run(monkeypatch, kw, zz)
    assert a.engines()[:2] == ["zs", "zs"] and d.engines()[:2] == ["zs", "zs"], a.levels
    _compare(kw, seed, [a, d])
    assert a.errs == d.errs
    _close(a, d)


@pytest.mark.parametrize("cid,env", [("zs-64x32x16", dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=32768)),
                                     ("bres-128x64-f64", dict())])
def test_errs_in_device_memory(cid, env, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(env, MGP_ERRS_HOST=0))
    d = _Run(monkeypatch, kw, env)
    o = Oracle(threads=8, **oracle_kw(kw))
    psis, oerrs = [dense_start(o, seed)[0]], []
    for _ in range(4):
        oerrs.append(o.step())
        psis.append(o.get(0))
    out = []
    for r in (a, d):
        dense_start(r.ctx, seed)
        _env(monkeypatch, r.env)
        out.append(r.ctx.cycles(4))
        assert np.array_equal(r.ctx.get_psi(), psis[4])
    assert np.array_equal(out[0], out[1]), out
    for it in range(4):
        _check_err(out[0][it], oerrs[it], psis[it + 1], psis[it])
    _close(a, d)


def test_graphs_captured_on_first_use(monkeypatch):
    """MGP_PRECAPTURE=0 with level 0 set again between cycles (test_dense_level0_set_again_between_cycles' flow): the
    graphs are then captured per pointer state as the cycles meet them."""
    kw, seed = case("reset-zs-64")
    zs = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536)
    runs = [_Run(monkeypatch, kw, dict(zs, MGP_PRECAPTURE=0)), _Run(monkeypatch, kw, zs)]
    assert all(r.engines()[0] == "zs" for r in runs)
    o = Oracle(threads=8, **oracle_kw(kw))
    psi0, f0 = dense_start(o, seed)
    for r in runs:
        dense_start(r.ctx, seed)

    def cycles(k):
        for it in range(k):
            old = o.get(0)
            eo = o.step()
            new = o.get(0)
            es = [r.cycle() for r in runs]
            for r, e in zip(runs, es):
                assert np.array_equal(r.ctx.get_psi(), new), f"{r.env}: psi differs after cycle {it + 1}"
                _check_err(e, eo, new, old)
            assert es[0] == es[1], es

    cycles(2)
    psi1, f1 = dense_fields(psi0.shape, psi0.dtype, seed + RESET_SEED_OFFSET)
    for r in runs:
        r.ctx.set_psi(psi1)
        r.ctx.set_f(f1)
    o.set(0, psi1)
    o.set(1, f1)
    cycles(3)
    for level in range(len(runs[1].levels)):
        assert np.array_equal(runs[0].ctx.get_psi(level), runs[1].ctx.get_psi(level)), level
        assert np.array_equal(runs[0].ctx.get_f(level), runs[1].ctx.get_f(level)), level
    _close(*runs)


def _first_tail(r):
    return [lv["tail"] for lv in r.levels].index(True)


def test_tail_cells_moves_the_tail(monkeypatch):
    """512 x 256 fp32: by default (4096 cells) the tail starts at level 3 (64 x 32); 8192 moves level 2 (128 x 64) from
    k_blk into it, 2047 moves level 3 out of it."""
    kw, seed = case("blk2-512x256-f32")
    up = _Run(monkeypatch, kw, dict(MGP_TAIL_CELLS=8192))
    down = _Run(monkeypatch, kw, dict(MGP_TAIL_CELLS=2047))
    d = _Run(monkeypatch, kw, dict())
    assert (_first_tail(up), _first_tail(d), _first_tail(down)) == (2, 3, 4)
    assert d.engines()[2] == "blk" and up.engines()[2] == "tail" and down.engines()[3] == "blk", (up.engines(), down.engines())
    _compare(kw, seed, [up, down, d])
    _close(up, down, d)


def test_blk_cells_moves_levels_between_k_blk_and_the_pieces(monkeypatch):
    """fp64 256^3: by default (2^18 cells) level 1 (128^3) runs per piece and level 2 (64^3) on k_blk; 2^21 moves
    level 1 onto k_blk, 2^17 level 2 off it."""
    kw, seed = case("patch-256-f64")
    up = _Run(monkeypatch, kw, dict(MGP_BLK_CELLS=1 << 21))
    down = _Run(monkeypatch, kw, dict(MGP_BLK_CELLS=1 << 17))
    d = _Run(monkeypatch, kw, dict())
    assert d.engines()[:4] == ["piece", "piece", "blk", "blk"], d.engines()
    assert up.engines()[:4] == ["piece", "blk", "blk", "blk"], up.engines()
    assert down.engines()[:4] == ["piece", "piece", "piece", "blk"], down.engines()
    _compare(kw, seed, [up, down, d], cycles=2)
    _close(up, down, d)


# ---- 5. the per-piece kernel forms ----

RR_CASES = ["zs-64x32x16", "bres-64x32x16-f64", "blk2-512x256-f32", "bres-128x64-f64", "jacobi-32-f64-pc", "jacobi-256-f64"]


def _piece_pair(monkeypatch, cid, env, ref_env):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(PIECES, **env))
    p = _Run(monkeypatch, kw, dict(PIECES, **ref_env))
    assert set(a.engines()) == {"piece"} and set(p.engines()) == {"piece"}
    _compare(kw, seed, [a, p])
    if kw["smoother"] == "rbgs":
        assert a.errs == p.errs  # the same err kernels in the same order
    _close(a, p)
    return kw


@pytest.mark.parametrize("cid", RR_CASES)
def test_vector_residual_restrict_on_every_level(cid, monkeypatch):
    """MGP_RR_SCALAR_CELLS=0: k_resrestrict<T, D> on every level with nx / 2 >= 16 / sizeof(T), with and without the
    boundary-modified operator (coarse_bc consistent / zero), down to one vector group per row."""
    kw = _piece_pair(monkeypatch, cid, dict(MGP_RR_SCALAR_CELLS=0, MGP_BRES=0), dict(MGP_BRES=0))
    assert kw["n"][0] // 2 >= 16 // (8 if kw["real"] == "double" else 4)


@pytest.mark.parametrize("cid", ["zs-64x32x16", "blk2-512x256-f32", "fresh-32x64x128-f32"])
def test_pair_residual_restrict_on_every_level(cid, monkeypatch):
    """MGP_RR_PAIR_CELLS=0: k_resrestrict<float, D, 2> on every fp32 level with nx >= 4, in 2D and 3D."""
    kw = _piece_pair(monkeypatch, cid, dict(MGP_RR_PAIR_CELLS=0, MGP_BRES=0), dict(MGP_BRES=0))
    assert kw["real"] == "float"


@pytest.mark.parametrize("vn", [0, 1, 2, 4])
@pytest.mark.parametrize("cid", ["zs-64x32x16", "bres-64x32x16-f64", "bres-128x64-f64", "blk2-512x256-f32"])
def test_bres_cells_per_thread(cid, vn, monkeypatch):
    """MGP_BRES_VN: k_bres (0) and k_bres_v with 1, 2 and 4 (fp32) cells per thread against the two launches."""
    kw = _piece_pair(monkeypatch, cid, dict(MGP_BRES_VN=vn), dict(MGP_BRES=0))
    assert kw["smoother"] == "rbgs" and kw["nu1"] >= 2 and kw.get("restriction", "average") == "average"


@pytest.mark.parametrize("cid", ["zs-64x32x16", "jacobi-32-f64-pc"])
def test_nontemporal_finest_half_sweep(cid, monkeypatch):
    _piece_pair(monkeypatch, cid, dict(MGP_NT=1), dict())


# ---- 6. mgp_residual_restrict on each form ----

RR_FORMS = {
    "scalar": dict(MGP_RR_SCALAR_CELLS=1 << 40, MGP_RR_PAIR_CELLS=1 << 40),
    "pair": dict(MGP_RR_SCALAR_CELLS=1 << 40, MGP_RR_PAIR_CELLS=0),
    "vector": dict(MGP_RR_SCALAR_CELLS=0),
}
# (nx, ny[, nz]), real.  8 x 8 x 8 fp32, 4 x 8 x 4 fp64 and 8 x 8 fp32 have one vector group per coarse row, so xlo and
# xhi fall in one thread; 16 x 8 x 4 has a vector level 1 (8 x 4 x 2: the boundary-modified branch with coarse_bc =
# consistent); 64 x 16 x 2 has one coarse plane; 32 x 16 fp64 has vector levels 0, 1 and 2.
RR_BOXES = [((8, 8, 8), "float"), ((4, 8, 4), "double"), ((16, 8, 4), "float"), ((64, 16, 2), "float"),
            ((8, 8), "float"), ((32, 16), "double")]


@pytest.mark.parametrize("bc", ["zero", "consistent"])
@pytest.mark.parametrize("form", list(RR_FORMS))
@pytest.mark.parametrize("box,real", RR_BOXES, ids=["x".join(map(str, b)) + "-" + r for b, r in RR_BOXES])
def test_residual_restrict_forms(box, real, form, bc, monkeypatch):
    dim = len(box)
    kw = dict(dim=dim, n=tuple(box) + (1,) * (3 - dim), real=real, coarse_bc=bc)
    r = _Run(monkeypatch, kw, dict(PIECES, **RR_FORMS[form]))
    ran = 0
    for level in (0, 1, 2):
        shp = r.ctx.shape(level) if level < len(r.levels) else None
        if shp is None or len(r.levels) <= level + 1 or min(shp) < 2:
            continue
        u, f = dense_fields(shp, r.ctx.dtype, 2001 + 2 * level)
        r.ctx.set_psi(u, level)
        r.ctx.set_f(f, level)
        _env(monkeypatch, r.env)
        r.ctx.residual_restrict(level)
        ref = restrict_arr(dim, residual_arr(dim, u, f, (2.0 ** level) / box[0], coarse_coef(bc, level)))
        assert np.array_equal(r.ctx.get_f(level + 1), ref), f"level {level}"
        assert np.array_equal(r.ctx.get_psi(level), u) and np.array_equal(r.ctx.get_f(level), f)
        ran += 1
    assert ran >= 1
    _close(r)
