"""GPU: whole cycles from dense random psi and f with the full weighting and with cpu-raw.lua's float arithmetic.

test_gpu_dense.py starts every cycle engine from dense_start() with the 2^d-average restriction and the real type's
own arithmetic.  Two families of kernels have load paths of their own and were still started from the point charge
alone (test_gpu_fw.py, test_gpu_rawfloat.py), where a load of the wrong cell reads the zero the right load would
have read:

  - restriction = full_weighting: k_resfw (mgp_fw.hip: a 64 x 16 / 64 x 32 tile, a 2-cell u halo and a 1-cell r
    ring, the 3-plane ring, z-chunks, face weights 3 - c per thread), the two passes k_resfield_v + k_fw_v
    (MGP_RESFW=0, and every level k_resfw does not support), the full weighting fused into k_zs PRE (LINEAR 2;
    MGP_ZS_FWF=0: LINEAR 1, then k_resfw), the restriction inside k_blk's PRE and inside both coarse tails, after
    k_ys, and on slabs (u exchanged two planes deep and f's ghost planes before k_resfw);
  - arith = double (float buffers, double expressions): one launch per piece on every level, kernels of its own.

Every whole-cycle case asserts what test_gpu_dense.py's cases assert, through its helpers: psi bit-identical to the
oracle after each of 3 cycles; psi and f of every level bit-identical to the reference path, the last of `runs`; err
against the oracle and to 1e-12 relative between the GPU paths; and that the engine under test ran (the levels'
engines, the level-0 PRE symbol under mgp_timing, or the shape condition under which the host picks the kernel).
The last section holds mgp_residual_restrict with the full weighting to the oracle's r -> R on the non-cubic boxes
test_gpu_fw.py's cubic ones miss.  The CPU side (test_dense_inputs.py) holds the reference to be well conditioned on
exactly these inputs.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_gpu_dense as D  # noqa: E402
from dense_start import RESET_SEED_OFFSET, case, dense_fields, dense_start, oracle_kw  # noqa: E402
from oracle_lib import Oracle, coarse_coef, residual_arr, restrict_fw_arr  # noqa: E402
from test_gpu_dense import _compare, _env, _loopback_dense, _mg, _Run, _timed_check  # noqa: E402
from test_gpu_parity import _check_err  # noqa: E402
from test_gpu_rawfloat import _err_ok  # noqa: E402

REAL = {"double": np.float64, "float": np.float32}
PIECES = dict(MGP_TAIL=0, MGP_BLK=0, MGP_FUSED=0)  # every level runs its own pieces


def _resfw_shape_ok(dim, nx, ny, nz):
    """mgp::resfw_supported on a replicated level: whole 64 x 16 (3D) / 64 x 32 (2D) tiles, whole coarse planes."""
    return nx % 64 == 0 and ny % (16 if dim == 3 else 32) == 0 and (dim == 2 or (nz >= 2 and nz % 2 == 0))


def _resfw_levels(run, dim):
    """The levels of a run that restrict (all but the coarsest) on which k_resfw is supported."""
    return [l for l, lv in enumerate(run.levels[:-1]) if _resfw_shape_ok(dim, lv["nx"], lv["ny"], lv["nz_local"])]


# ---- 1. the full weighting fused into k_zs PRE (LINEAR 2: fp32, cl = 0) ----

@pytest.mark.parametrize("cid,min_cells", [
    ("fw-zs-64x32x16", 32768),    # one tile, every face a box face (the box has 32768 cells: its own threshold)
    ("fw-zs-128x64x32", 65536),   # 2 x 2 PRE tiles
    ("fw-zs-128-pc-zero", 65536),  # level 1 (64^3, cl = 0, a fresh guess) runs the fused full weighting too
    ("fw-zs-64-F", 65536),
], ids=["one-tile", "2x2-tiles", "two-fused-levels-pc-zero", "F"])
def test_dense_fw_fused_into_k_zs_pre(cid, min_cells, monkeypatch):
    kw, seed = case(cid)
    base = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=min_cells)
    a = _Run(monkeypatch, kw, dict(base, MGP_ZS_FWF=1))
    b = _Run(monkeypatch, kw, dict(base, MGP_ZS_FWF=0))  # PRE smooths only; k_resfw restricts after it
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert a.engines()[0] == "zs" and b.engines()[0] == "zs" and "zs" not in p.engines()
    if cid == "fw-zs-128-pc-zero":
        assert a.engines()[:2] == ["zs", "zs"] and b.engines()[:2] == ["zs", "zs"], a.levels
    assert 0 in _resfw_levels(b, 3)
    o = _compare(kw, seed, [a, b, p])
    _timed_check(kw, o, (a, "k_zs<float, true, 2, false, true, false>", None),
                 (b, "k_zs<float, true, 1, false, true, false>", None))


# ---- 2. fp64: k_zs PRE (LINEAR 1), then k_resfw or the two passes ----

@pytest.mark.parametrize("cid", ["fw-zs-f64-128x64x32", "fw-zs-f64-128x64x32-zero"])
def test_dense_fw_k_zs_f64_then_resfw(cid, monkeypatch):
    kw, seed = case(cid)
    base = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536)
    a = _Run(monkeypatch, kw, base)
    b = _Run(monkeypatch, kw, dict(base, MGP_RESFW=0))
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert a.engines()[0] == "zs" and b.engines()[0] == "zs" and "zs" not in p.engines()
    assert 0 in _resfw_levels(a, 3)  # k_resfw runs level 0 unless switched off: 2 x 4 tiles, z-chunks
    o = _compare(kw, seed, [a, b, p])
    pre = "k_zs<double, true, 1, false, true, false>"
    _timed_check(kw, o, (a, pre, None), (b, pre, None))


# ---- 3. k_resfw on per-piece levels against the two passes ----

@pytest.mark.parametrize("cid", ["fw-resfw-128x32x16-f64", "fw-resfw-128x32x16-f32-jacobi", "fw-resfw-128x64-f64",
                                 "fw-resfw-128x64-f32-zero"])
def test_dense_fw_resfw_against_two_passes(cid, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(PIECES, MGP_RESFW=1))
    p = _Run(monkeypatch, kw, dict(PIECES, MGP_RESFW=0))
    assert set(a.engines()) == {"piece"} and set(p.engines()) == {"piece"}
    # k_resfw is the host's choice on levels 0 and 1 (more than one tile on level 0), the two passes below them
    assert _resfw_levels(a, kw["dim"]) == [0, 1], a.levels
    lv = a.levels[0]
    assert (lv["nx"] // 64) * (lv["ny"] // (16 if kw["dim"] == 3 else 32)) >= 4
    _compare(kw, seed, [a, p])


def test_dense_fw_two_passes_on_every_level(monkeypatch):
    kw, seed = case("fw-two-32x16x8-f32")
    a = _Run(monkeypatch, kw, dict(PIECES))
    assert set(a.engines()) == {"piece"}
    # no level has whole k_resfw tiles, so k_resfield_v + k_fw_v run all of them and MGP_RESFW changes nothing
    assert all(lv["nx"] % 64 != 0 for lv in a.levels) and _resfw_levels(a, 3) == []
    _compare(kw, seed, [a])


# ---- 4. k_blk's PRE, the coarse tails, k_ys ----

@pytest.mark.parametrize("cid", ["fw-blk-64x16x32-f64", "fw-blk-128-f64"])
def test_dense_fw_k_blk(cid, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(MGP_TAIL=0, MGP_BLK=1, MGP_BLK2=0))
    p = _Run(monkeypatch, kw, dict(MGP_TAIL=0, MGP_BLK=0))
    assert a.engines()[0] == "piece" and a.engines()[1] == "blk", a.levels
    assert "blk" not in p.engines()
    _compare(kw, seed, [a, p])


def test_dense_fw_k_tail(monkeypatch):
    kw, seed = case("fw-tail-64x32x16-f32")
    a = _Run(monkeypatch, kw, dict(MGP_TAIL=1))
    p = _Run(monkeypatch, kw, dict(MGP_TAIL=0))
    assert any(lv["tail"] for lv in a.levels) and not any(lv["tail"] for lv in p.levels)
    assert not a.levels[0]["tail"]
    _compare(kw, seed, [a, p])


def test_dense_fw_k_tail_c(monkeypatch):
    kw, seed = case("fw-tailc-32x32x64-f64")
    a = _Run(monkeypatch, kw, dict(MGP_TAIL=1))
    g = _Run(monkeypatch, kw, dict(MGP_TAIL=1, MGP_TAIL_CUBIC=0))  # the generic k_tail
    p = _Run(monkeypatch, kw, dict(MGP_TAIL=0))
    # the tail's levels are k_tail_c's compile-time shape 8 x 8 x 16 (and red/black): it runs unless switched off
    tl = [(lv["nx"], lv["ny"], lv["nz_global"]) for lv in a.levels if lv["tail"]]
    assert tl == [(8, 8, 16), (4, 4, 8), (2, 2, 4), (1, 1, 2)], tl
    assert [lv["tail"] for lv in g.levels] == [lv["tail"] for lv in a.levels]
    assert kw["smoother"] == "rbgs" and not any(lv["tail"] for lv in p.levels)
    _compare(kw, seed, [a, g, p])


@pytest.mark.parametrize("cid", ["fw-ys-1024-f32", "fw-ys-1024x512-f64"])
def test_dense_fw_k_ys_then_resfw(cid, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(MGP_FUSED=1, MGP_YS_MIN_CELLS=65536))
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert a.engines()[0] == "zs" and p.engines()[0] != "zs"
    assert 0 in _resfw_levels(a, 2)
    o = _compare(kw, seed, [a, p])
    k, = _timed_check(kw, o, (a, None, None))
    real = kw["real"]
    # PRE smooths only (LINEAR 1: both colours stored), the full weighting follows it
    assert k["fused_pre"][0].startswith(f"k_ys<{real}, true, 1,") and k["fused_post"][0].startswith(f"k_ys<{real}, false,"), k


# ---- 5. loopback slabs ----

def _single_and_oracle(monkeypatch, kw, env, seed, fused):
    s = _Run(monkeypatch, dict(kw, gather_cells=4096), env)
    assert (s.engines()[0] == "zs") == fused
    o = Oracle(threads=8, **oracle_kw(kw))
    dense_start(o, seed)
    dense_start(s.ctx, seed)
    return s, o


def _cycles_against_oracle(s, o, k):
    es = []
    for _ in range(k):
        old = o.get(0)
        eo = o.step()
        es.append(s.cycle())
        _check_err(es[-1], eo, o.get(0), old)
    assert np.array_equal(s.ctx.get_psi(), o.get(0)), "single-domain psi differs from the oracle"
    return es


def test_dense_fw_loopback_slabs_k_zs(monkeypatch):
    """World 2, fp32: k_zs PRE (LINEAR 1 on a slab), then k_resfw on u exchanged two planes deep and f's ghost planes,
    all holding generic data.  Gathered psi == the single domain == the oracle, bit for bit."""
    kw, seed = case("fw-slab-zs-64")
    env = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536)
    _env(monkeypatch, env)
    psi, errs = _loopback_dense(kw["n"], 2, 4096, {k: v for k, v in kw.items() if k != "n"}, seed, cycles=2,
                                expect_fused=True)
    s, o = _single_and_oracle(monkeypatch, kw, env, seed, True)
    es = _cycles_against_oracle(s, o, 2)
    assert np.array_equal(psi, o.get(0)), "gathered slab psi differs from the oracle"
    for e in errs:
        np.testing.assert_allclose(e, es, rtol=1e-12, atol=0)


def _loopback_dense_reset(box, world, gather, cfg, seed, cycles=2):
    """_loopback_dense with one more step: after `cycles` cycles every rank sets its own planes of the second pair
    of dense fields (seed + RESET_SEED_OFFSET) and runs `cycles` more.  Returns the gathered psi after each half and
    the per-rank errs of each."""
    mg = _mg()
    lb = mg.Loopback(world)
    out, errors = [None] * world, []
    gate = threading.Barrier(world, timeout=300)

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(n=box, rank=r, world=world, gather_cells=gather, device=0,
                                          comm_id=b"\0" * 128, **cfg), loopback=lb)
            lv = ctx.levels[0]
            assert lv["distributed"] and lv["nz_local"] * world == box[2] and lv["z0"] == r * lv["nz_local"]
            # the slab's level 0 is one k_resfw runs (ghost planes two deep: the deep-halo sweeps' depth)
            assert _resfw_shape_ok(3, lv["nx"], lv["ny"], lv["nz_local"])
            z = slice(lv["z0"], lv["z0"] + lv["nz_local"])
            ctx.timing(True)
            got = []
            for half in range(2):
                psi0, f0 = dense_start(ctx, seed + half * RESET_SEED_OFFSET)
                assert np.array_equal(ctx.get_psi(), psi0[z]) and np.array_equal(ctx.get_f(), f0[z])
                errs = ctx.cycles(cycles)
                got.append((ctx.get_psi(), errs))
                gate.wait()  # no rank sets its planes while another still reads them
            t = ctx.timing_read()
            ctx.timing(False)
            assert t["fused_pre"][1] == 0 and t["fused_post"][1] == 0 and t["half_sweep"][1] > 0, t
            assert t["exchange"][1] > 0, t
            out[r] = got
            ctx.close()
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))
            gate.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    lb.close()
    assert not errors, errors
    return [(np.concatenate([out[r][h][0] for r in range(world)], axis=0), [out[r][h][1] for r in range(world)])
            for h in range(2)]


def test_dense_fw_loopback_slabs_per_piece_and_f_set_again(monkeypatch):
    """World 2, fp64, one launch per piece: k_resfw reads f one ghost plane deep, and the host exchanges f's ghost
    planes only when they are stale.  After 2 cycles every rank sets its planes of a second pair of dense fields
    (set_planes of psi and f): the next restriction must see the neighbours' new f.  Gathered psi == the single
    domain == the oracle after each half, bit for bit."""
    kw, seed = case("fw-slab-piece-64-f64")
    env = dict(MGP_FUSED=0)
    _env(monkeypatch, env)
    halves = _loopback_dense_reset(kw["n"], 2, 4096, {k: v for k, v in kw.items() if k != "n"}, seed, cycles=2)
    s, o = _single_and_oracle(monkeypatch, kw, env, seed, False)
    for half, (psi, errs) in enumerate(halves):
        if half:
            psi1, f1 = dense_fields(psi.shape, psi.dtype, seed + RESET_SEED_OFFSET)
            for x in (s.ctx, o):
                dense_start(x, seed + RESET_SEED_OFFSET)
            assert np.array_equal(s.ctx.get_psi(), psi1) and np.array_equal(o.get(1), f1)
        es = _cycles_against_oracle(s, o, 2)
        assert np.array_equal(psi, o.get(0)), f"gathered slab psi differs from the oracle (half {half})"
        for e in errs:
            np.testing.assert_allclose(e, es, rtol=1e-12, atol=0)


# ---- 6. cpu-raw.lua's float arithmetic ----

def _check_err_raw(e_gpu, e_oracle, psi_new, psi_old):
    """_check_err for arith = double: err sums the float-rounded squares of the double differences
    (cpu-raw.lua:96-100, 249-254), so the pairwise reference is test_gpu_rawfloat._err_ok's, at the same 1e-12;
    against the oracle's sequential sum, its summation bound (as test_rawfloat_cycles_match_oracle)."""
    _err_ok(e_gpu, psi_new, psi_old)
    assert abs(e_gpu - e_oracle) <= max(1e-12, 4 * psi_new.size * 2.0 ** -53) * abs(e_oracle), (e_gpu, e_oracle)


@pytest.mark.parametrize("cid,graph", [
    ("raw-64-jacobi", None), ("raw-64-jacobi", "0"), ("raw-32x16x8-rbgs", None), ("raw-64x32-gslex", None),
    ("raw-32-fw", None), ("raw-16x32x16-F-warm", None),
], ids=["jacobi-reference-config", "jacobi-reference-config-eager", "rbgs-32x16x8", "gslex-64x32", "fw-32",
        "jacobi-F-warm-16x32x16"])
def test_dense_rawfloat(cid, graph, monkeypatch):
    kw, seed = case(cid)
    assert kw["real"] == "float" and kw["arith"] == "double"
    a = _Run(monkeypatch, kw, dict() if graph is None else dict(MGP_GRAPH=graph))
    assert set(a.engines()) == {"piece"}  # one launch per piece on every level: there is no other path
    # _compare with the err reference of this arithmetic (it reads the module's _check_err when it runs)
    monkeypatch.setattr(D, "_check_err", _check_err_raw)
    o = _compare(kw, seed, [a])
    # it is the double arithmetic: the same cycles with every operation rounded to float differ
    g = Oracle(**dict(oracle_kw(kw), arith="real"))
    dense_start(g, seed)
    for _ in range(3):
        g.step()
    assert not np.array_equal(g.get(0), o.get(0))


# ---- 7. mgp_residual_restrict with the full weighting on non-cubic boxes ----

FW_PIECE_BOXES = [
    (3, (128, 32, 16), 0),  # two x tiles, two y tiles, four z-chunks of 2 coarse planes
    (3, (128, 32, 16), 1),  # 64 x 16 x 8, cl != 0 under coarse_bc = consistent: one tile, two z-chunks
    (3, (256, 32, 8), 0),   # four x tiles, cz = 4: two z-chunks of 2
    (3, (64, 16, 2), 0),    # the smallest box k_resfw takes: one coarse plane, every face weight in play
    (2, (128, 64, 1), 0),   # 2 x 2 tiles of the 2D kernel
    (2, (128, 64, 1), 1),   # 64 x 32: one tile, cl != 0
    (2, (64, 32, 1), 0),    # one tile
]


@pytest.mark.parametrize("bc", ["zero", "consistent"])
@pytest.mark.parametrize("real", ["double", "float"])
@pytest.mark.parametrize("dim,n,level", FW_PIECE_BOXES,
                         ids=["x".join(str(v) for v in n[:dim]) + f"-L{level}" for dim, n, level in FW_PIECE_BOXES])
def test_fw_residual_restrict_non_cubic(dim, n, level, real, bc, monkeypatch):
    """k_resfw (MGP_RESFW=1) and k_resfield_v + k_fw_v (MGP_RESFW=0) == the oracle's r -> R, and each other, bit for
    bit, from random u and f on the level."""
    out = {}
    for resfw in ("1", "0"):
        _env(monkeypatch, dict(MGP_RESFW=resfw))
        mg = _mg()
        ctx = mg.Context(mg.make_opts(dim=dim, n=n, real=real, coarse_bc=bc, restriction="full_weighting"))
        assert level + 1 < len(ctx.levels)
        shp = ctx.shape(level)
        assert shp == tuple(v >> level for v in reversed(n[:dim]))
        assert _resfw_shape_ok(dim, shp[-1], shp[-2], shp[0] if dim == 3 else 1)  # k_resfw's unless switched off
        rng = np.random.default_rng(1201 + level)
        u = rng.uniform(-1, 1, shp).astype(REAL[real])
        f = rng.uniform(-1, 1, shp).astype(REAL[real])
        ctx.set_psi(u, level)
        ctx.set_f(f, level)
        ctx.residual_restrict(level)
        out[resfw] = ctx.get_f(level + 1)
        ctx.close()
    h = (2.0 ** level) / n[0]
    ref = restrict_fw_arr(dim, residual_arr(dim, u, f, h, coarse_coef(bc, level)), coarse_coef(bc, level + 1))
    assert np.count_nonzero(ref) == ref.size
    for resfw, R in out.items():
        assert np.array_equal(R, ref), (f"MGP_RESFW={resfw}", np.argwhere(R != ref)[:4])
    assert np.array_equal(out["1"], out["0"])
