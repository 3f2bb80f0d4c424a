"""GPU: whole cycles from dense random psi and f on every cycle engine, against the C oracle.

Every other whole-cycle test starts from init_point_charge(): one non-zero cell in level 0's f and psi.  A level-0
load of the wrong f cell, row, plane or colour (k_zs's y-halo rows that skip f loads, its clamped out-of-box
columns, the z-chunk seams, k_ys's segment halos, k_bres on a per-piece level 0), and every load of u in the first
cycle, then reads a zero where it should have read a zero.  Here the same engines start from dense_start(): uniform
random fields without a zero cell, the same in the context, the oracle and every slab rank.

Every case checks, with the tolerances the mirrored tests use:
  - psi bit-identical to the oracle after each of 3 cycles (run as the product runs them: graph replay on one GPU);
  - psi and f of every level bit-identical to the same options with the engine switched off;
  - err against the oracle by test_gpu_parity._check_err, and between the two GPU paths to 1e-12 relative;
  - that the engine ran: levels[i]["engine"] / ["tail"], and for the level-0 kernels the symbol and the launch
    counts of one more cycle under mgp_timing (timed cycles run eagerly, so that cycle also checks the eager path
    against the oracle).  k_bres shows in level 0's half-sweep launch count.  k_blk2 and k_fresh run below the
    finest level only and have no launch record in the API; their cases assert every condition under which the
    host picks them that a context exposes (the engines of the levels involved, the options), with the switch
    that turns them off as the only difference between the two runs.
The CPU side (test_dense_inputs.py) holds the reference to be well conditioned on exactly these inputs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dense_start import RESET_SEED_OFFSET, case, dense_fields, dense_start, oracle_kw  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
from test_gpu_parity import _check_err  # noqa: E402

SPLIT_NAME = "k_zs_split<float, false>"

# every switch a case may set; a variant's environment is these cleared, then its own
SWITCHES = ("MGP_FUSED", "MGP_FUSED_MIN_CELLS", "MGP_ZPOST_MIN_CELLS", "MGP_ZS_SPLIT", "MGP_ZS_WIDE", "MGP_LAZY_ZERO",
            "MGP_YS_MIN_CELLS", "MGP_YS_HALF", "MGP_BLK", "MGP_BLK2", "MGP_BRES", "MGP_TAIL", "MGP_TAIL_CUBIC",
            "MGP_FRESH", "MGP_GRAPH", "MGP_RESFW", "MGP_ZS_FWF",
            # test_gpu_switches.py's
            "MGP_ZS_WGS", "MGP_ZS_PATCH", "MGP_ZS_PATCH_PRE", "MGP_ZS_PATCH_POST", "MGP_ZS_SPLIT_POST",
            "MGP_ZS_SPLIT_POST_MIN_CELLS", "MGP_ZS_POST_ZC", "MGP_PLANE_PAD", "MGP_LAZY_ZERO_FUSED", "MGP_ERRS_HOST",
            "MGP_PRECAPTURE", "MGP_TAIL_CELLS", "MGP_BLK_CELLS", "MGP_BRES_VN", "MGP_RR_SCALAR_CELLS",
            "MGP_RR_PAIR_CELLS", "MGP_NT")


def _mg():
    import mgpoisson

    return mgpoisson


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in SWITCHES, k
        monkeypatch.setenv(k, str(v))


class _Run:
    """A context with the environment it was created under (some switches are read at launch or capture time, so
    every call runs under it again)."""

    def __init__(self, monkeypatch, kw, env):
        self.mp, self.env = monkeypatch, dict(env)
        _env(monkeypatch, self.env)
        mg = _mg()
        self.ctx = mg.Context(mg.make_opts(**kw))
        self.levels = self.ctx.levels
        self.errs = []  # of _compare's cycles

    def engines(self):
        return [lv["engine"] for lv in self.levels]

    def cycle(self):
        _env(self.mp, self.env)
        return self.ctx.cycle()

    def timed_cycle(self):
        """One cycle under mgp_timing: (err, timing_read(), timing_kernels())."""
        _env(self.mp, self.env)
        self.ctx.timing(True)
        e = self.ctx.cycle()
        t, k = self.ctx.timing_read(), self.ctx.timing_kernels()
        self.ctx.timing(False)
        return e, t, k


def _compare(kw, seed, runs, cycles=3):
    """runs: the engine under test first (one or more), the per-piece path (its off switch) last.  All start from
    the dense fields of `seed`; returns the oracle (after `cycles` steps)."""
    o = Oracle(threads=8, **oracle_kw(kw))
    psi0, _ = dense_start(o, seed)
    for r in runs:
        dense_start(r.ctx, seed)
        assert np.array_equal(r.ctx.get_psi(), psi0)
    want_err = kw.get("err_mode", 1)
    for it in range(cycles):
        old = o.get(0)
        eo = o.step()
        new = o.get(0)
        errs = [r.cycle() for r in runs]
        for i, r in enumerate(runs):
            r.errs.append(errs[i])
            assert np.array_equal(r.ctx.get_psi(), new), f"run {i} {r.env}: psi differs after cycle {it + 1}"
            if want_err:
                _check_err(errs[i], eo, new, old)
                assert abs(errs[i] - errs[-1]) <= 1e-12 * abs(errs[-1]), (i, errs)
    ref = runs[-1].ctx
    for i, r in enumerate(runs[:-1]):
        assert len(r.levels) == len(ref.levels)
        for level in range(len(ref.levels)):
            assert np.array_equal(r.ctx.get_psi(level), ref.get_psi(level)), f"run {i} {r.env}: psi level {level}"
            assert np.array_equal(r.ctx.get_f(level), ref.get_f(level)), f"run {i} {r.env}: f level {level}"
    return o


def _timed_check(kw, o, *runs):
    """One more cycle under mgp_timing on level-0 fused runs, each given as (run, PRE kernel, POST kernel) with
    None for a name not held: the phases ran as one launch each (no half-sweep launches on level 0) on the kernels
    named, and psi still equals the oracle's.  Returns each run's timing_kernels()."""
    old = o.get(0)
    eo = o.step()
    new = o.get(0)
    out = []
    for run, pre_name, post_name in runs:
        e, t, k = run.timed_cycle()
        assert np.array_equal(run.ctx.get_psi(), new), f"{run.env}: psi differs after the timed (eager) cycle"
        if kw.get("err_mode", 1):
            _check_err(e, eo, new, old)
        assert t["fused_pre"][1] == 1 and t["fused_post"][1] == 1 and t["half_sweep"][1] == 0, t
        assert pre_name is None or k["fused_pre"][0] == pre_name, k
        assert post_name is None or k["fused_post"][0] == post_name, k
        out.append(k)
    return out


# ---- 1. k_zs_split and k_zs, fp32, cl = 0 ----

@pytest.mark.parametrize("cid,min_cells,wide", [
    ("zs-64x32x16", 32768, "1"),    # one tile, every face a box face, one 16-plane chunk
    ("zs-64x32x64", 65536, "1"),    # four 16-plane chunks
    ("zs-128x64x32", 65536, "1"),   # 2 x 2 PRE tiles; POST's wide 128 x 16 tile: four tiles in y
    ("zs-128x64x32", 65536, "0"),   # POST's 64 x 32 tile: 2 x 2
], ids=["one-tile-16", "one-tile-4-chunks", "2x2-tiles-wide", "2x2-tiles-narrow"])
def test_dense_zs_split_and_k_zs(cid, min_cells, wide, monkeypatch):
    kw, seed = case(cid)
    base = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=min_cells, MGP_ZS_WIDE=wide)
    a = _Run(monkeypatch, kw, dict(base, MGP_ZS_SPLIT=1))
    b = _Run(monkeypatch, kw, dict(base, MGP_ZS_SPLIT=0))
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert a.engines()[0] == "zs" and b.engines()[0] == "zs" and p.engines()[0] == "piece"
    o = _compare(kw, seed, [a, b, p])
    is_wide = wide == "1" and kw["n"][0] % 128 == 0
    post = f"k_zs<float, false, 1, true, true, {'true' if is_wide else 'false'}>"
    ka, kb = _timed_check(kw, o, (a, SPLIT_NAME, post), (b, "k_zs<float, true, 0, false, true, false>", post))
    assert ka["fused_pre"][1] // 768 == kb["fused_pre"][1] // 448  # the same workgroups, 12 waves against 7


# ---- 2. k_zs fp64, 3. F-cycle and err_mode = 0 ----

@pytest.mark.parametrize("cid,pre,post", [
    ("zs-f64-128x64x32-pc-zero", "k_zs<double, true, 0, false, true, false>", "k_zs<double, false, 0, true, true, false>"),
    ("zs-f64-64x128x64-warm", "k_zs<double, true, 0, false, true, false>", "k_zs<double, false, 1, true, true, false>"),
    ("zs-64-F", SPLIT_NAME, "k_zs<float, false, 1, true, true, false>"),
    ("zs-64x32x128-noerr", SPLIT_NAME, "k_zs<float, false, 0, false, true, false>"),
], ids=["f64-pc-zero", "f64-linear-warm", "f32-F", "f32-err_mode0"])
def test_dense_k_zs(cid, pre, post, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536))
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert a.engines()[0] == "zs" and "zs" not in p.engines()
    o = _compare(kw, seed, [a, p])
    _timed_check(kw, o, (a, pre, post))


# ---- 4. two fused levels, zpost, the lazy zero ----

def test_dense_two_fused_levels_zpost_and_lazy_zero(monkeypatch):
    kw, seed = case("zs-128")
    zz = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536, MGP_ZPOST_MIN_CELLS=1 << 40)
    a = _Run(monkeypatch, kw, zz)
    m = _Run(monkeypatch, kw, dict(zz, MGP_LAZY_ZERO=0))
    z = _Run(monkeypatch, kw, dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=1 << 21, MGP_ZPOST_MIN_CELLS=1 << 18))
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert a.engines()[:2] == ["zs", "zs"] and m.engines()[:2] == ["zs", "zs"], a.levels
    assert z.engines()[:2] == ["zs", "zpost"], z.levels
    assert not {"zs", "zpost"} & set(p.engines())
    # (_compare holds a, m and z to the same psi and f on every level as p, so MGP_LAZY_ZERO=0 equals the default
    # bit for bit; their errs are the same sums in the same order)
    o = _compare(kw, seed, [a, m, z, p])
    assert a.errs == m.errs
    _timed_check(kw, o, (a, SPLIT_NAME, "k_zs<float, false, 1, true, true, true>"))


# ---- 5. k_ys ----

@pytest.mark.parametrize("cid,half", [
    ("ys-1024-f32", "0"),
    ("ys-1024x512-f64-zero", "0"),
    ("ys-1024-f64-pc", "1"),
    ("ys-2048x1024-f64-F", None),  # the default rule: half segments below 256 workgroups
], ids=["f32-full", "f64-zero-full", "f64-pc-half", "f64-F-default"])
def test_dense_k_ys(cid, half, monkeypatch):
    kw, seed = case(cid)
    env = dict(MGP_FUSED=1, MGP_YS_MIN_CELLS=65536)
    if half is not None:
        env["MGP_YS_HALF"] = half
    a = _Run(monkeypatch, kw, env)
    p = _Run(monkeypatch, kw, dict(MGP_FUSED=0))
    assert a.engines()[0] == "zs" and p.engines()[0] != "zs"
    o = _compare(kw, seed, [a, p])
    k, = _timed_check(kw, o, (a, None, None))
    real = kw["real"]
    assert k["fused_pre"][0].startswith(f"k_ys<{real}, true,") and k["fused_post"][0].startswith(f"k_ys<{real}, false,"), k
    if half is not None:  # the segment width is the kernel's last template argument: the other setting's differs
        other = _Run(monkeypatch, kw, dict(env, MGP_YS_HALF="1" if half == "0" else "0"))
        dense_start(other.ctx, seed)
        ko = other.timed_cycle()[2]
        wa, wo = (int(x["fused_pre"][0].rstrip(">").split(",")[-1]) for x in (k, ko))
        assert (wa == 2 * wo) if half == "0" else (2 * wa == wo), (k, ko)


# ---- 6. k_blk, k_blk2, k_bres, the coarse tail (k_tail, k_tail_c), k_fresh ----

@pytest.mark.parametrize("cid", ["blk-64x16x32-f64", "blk-128-f64"])
def test_dense_k_blk(cid, monkeypatch):
    kw, seed = case(cid)
    # (both configurations run without the coarse tail in test_gpu_block.py; MGP_BLK2=0: one k_blk launch per
    # level, the pairs are test_dense_k_blk2's)
    a = _Run(monkeypatch, kw, dict(MGP_TAIL=0, MGP_BLK=1, MGP_BLK2=0))
    p = _Run(monkeypatch, kw, dict(MGP_TAIL=0, MGP_BLK=0))
    assert a.engines()[0] == "piece" and a.engines()[1] == "blk", a.levels
    assert "blk" not in p.engines()
    _compare(kw, seed, [a, p])


def test_dense_k_blk2(monkeypatch):
    kw, seed = case("blk2-512x256-f32")
    a = _Run(monkeypatch, kw, dict(MGP_BLK2=1))
    p = _Run(monkeypatch, kw, dict(MGP_BLK2=0))
    # the host pairs two consecutive tiled 2D levels of a V-cycle (red/black, average restriction), the second
    # not the tail's first: levels 1 and 2 here.  Both contexts plan the same engines; MGP_BLK2 alone differs.
    e = a.engines()
    assert e == p.engines() and e[:4] == ["piece", "blk", "blk", "tail"], e
    assert kw["dim"] == 2 and kw.get("cycle", "V") == "V" and kw["smoother"] == "rbgs"
    _compare(kw, seed, [a, p])


@pytest.mark.parametrize("cid", ["bres-64x32x16-f64", "bres-128x64-f64"])
def test_dense_k_bres(cid, monkeypatch):
    kw, seed = case(cid)
    off = dict(MGP_TAIL=0, MGP_BLK=0, MGP_FUSED=0)  # every level runs its own pieces, level 0 (dense f) included
    a = _Run(monkeypatch, kw, dict(off, MGP_BRES=1))
    p = _Run(monkeypatch, kw, dict(off, MGP_BRES=0))
    # k_bres replaces the last pre black half-sweep + residual + restriction of a per-piece red/black level with
    # nu1 >= 2 and the average restriction
    assert set(a.engines()) == {"piece"} and set(p.engines()) == {"piece"}
    assert kw["smoother"] == "rbgs" and kw["nu1"] >= 2 and kw.get("restriction", "average") == "average"
    _compare(kw, seed, [a, p])
    # on level 0 it shows in the launch record: one plain half-sweep launch fewer per cycle than with MGP_BRES=0
    (_, ta, _), (_, tp, _) = a.timed_cycle(), p.timed_cycle()
    assert tp["half_sweep"][1] - ta["half_sweep"][1] == 1, (ta["half_sweep"], tp["half_sweep"])
    assert np.array_equal(a.ctx.get_psi(), p.ctx.get_psi())


@pytest.mark.parametrize("cid", ["tail-64x32x16-f32", "tail-64-f64"])
def test_dense_k_tail(cid, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(MGP_TAIL=1))
    p = _Run(monkeypatch, kw, dict(MGP_TAIL=0))
    assert any(lv["tail"] for lv in a.levels) and not any(lv["tail"] for lv in p.levels)
    assert not a.levels[0]["tail"]
    _compare(kw, seed, [a, p])


@pytest.mark.parametrize("cid,top", [("tailc-32x32x64-f64", (8, 8, 16)), ("tailc-128-f64", (64, 64, 1))])
def test_dense_k_tail_c(cid, top, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(MGP_TAIL_CUBIC=1))
    g = _Run(monkeypatch, kw, dict(MGP_TAIL_CUBIC=0))  # the generic k_tail
    p = _Run(monkeypatch, kw, dict(MGP_TAIL=0))
    # the tail's levels are one of k_tail_c's compile-time shapes (and red/black): it runs unless switched off
    dim = kw["dim"]
    tl = [(lv["nx"], lv["ny"], lv["nz_global"]) for lv in a.levels if lv["tail"]]
    nl = min(top[:dim]).bit_length()
    assert tl == [tuple(max(1, t >> l) if d < dim else 1 for d, t in enumerate(top)) for l in range(nl)], tl
    assert kw["smoother"] == "rbgs" and not any(lv["tail"] for lv in p.levels)
    _compare(kw, seed, [a, g, p])


@pytest.mark.parametrize("cid", ["fresh-32x64x128-f32", "fresh-256-f64"])
def test_dense_k_fresh(cid, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict(MGP_BLK=0, MGP_FRESH=1))
    p = _Run(monkeypatch, kw, dict(MGP_BLK=0, MGP_FRESH=0))
    # k_fresh is the first red/black sweep of a fresh (lazily zeroed) coarse guess on a per-piece level below
    # the finest: there is one (tiled phases off), and the coarse guesses are fresh
    e = a.engines()
    assert e == p.engines() and e[0] == "piece" and "piece" in e[1:], e
    assert kw["smoother"] == "rbgs" and kw.get("coarse_init", "fresh") == "fresh"
    _compare(kw, seed, [a, p])


# ---- 7. Jacobi 7 + 7 and the lexicographic Gauss-Seidel ----

@pytest.mark.parametrize("cid", ["jacobi-256-f64", "jacobi-32-f64-pc"])
def test_dense_jacobi(cid, monkeypatch):
    kw, seed = case(cid)
    a = _Run(monkeypatch, kw, dict())
    p = _Run(monkeypatch, kw, dict(MGP_TAIL=0))
    # Jacobi runs one launch per piece above the generic coarse tail and nothing else
    assert set(a.engines()) == {"piece", "tail"} and set(p.engines()) == {"piece"}
    _compare(kw, seed, [a, p])


def test_dense_gslex(monkeypatch):
    kw, seed = case("gslex-64-f64")
    a = _Run(monkeypatch, kw, dict())
    assert all(e == "piece" for e in a.engines())  # k_gslex per sweep on every level: there is no other path
    o = _compare(kw, seed, [a])
    # it is the lexicographic sweep: the red/black cycle of the same start differs
    rb = Oracle(**dict(oracle_kw(kw), smoother="rbgs"))
    dense_start(rb, seed)
    for _ in range(3):
        rb.step()
    assert not np.array_equal(rb.get(0), o.get(0))


# ---- 8. level 0 set again in mid-run ----

@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph-replay", "eager"])
@pytest.mark.parametrize("cid,env,engine", [
    ("reset-zs-64", dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536), "zs"),
    ("reset-piece-256-f64", dict(MGP_TAIL=0), "piece"),
], ids=["k_zs-f32", "per-piece-f64"])
def test_dense_level0_set_again_between_cycles(cid, env, engine, graph, monkeypatch):
    """The finest level rotates u with psiOld (and POST's output buffer) from cycle to cycle, and the cycle graphs
    are captured per pointer state when the context is created.  set_psi / set_f between cycles write the buffer
    that is u at that moment: the next cycle, replayed or eager, must start from the fields set and take its psiOld
    (err) from them."""
    kw, seed = case(cid)
    r = _Run(monkeypatch, kw, dict(env, MGP_GRAPH=graph))
    assert r.engines()[0] == engine and (engine == "zs" or set(r.engines()) == {"piece"})
    o = Oracle(threads=8, **oracle_kw(kw))
    psi0, f0 = dense_start(o, seed)
    dense_start(r.ctx, seed)
    assert np.array_equal(r.ctx.get_psi(), psi0) and np.array_equal(r.ctx.get_f(), f0)

    def cycles(k, first_old=None):
        for it in range(k):
            old = o.get(0)
            if it == 0 and first_old is not None:
                assert np.array_equal(old, first_old)
            e, eo = r.cycle(), o.step()
            new = o.get(0)
            assert np.array_equal(r.ctx.get_psi(), new), f"psi differs after cycle {it + 1}"
            _check_err(e, eo, new, old)

    cycles(2)
    psi1, f1 = dense_fields(psi0.shape, psi0.dtype, seed + RESET_SEED_OFFSET)
    r.ctx.set_psi(psi1)
    r.ctx.set_f(f1)
    assert np.array_equal(r.ctx.get_psi(), psi1) and np.array_equal(r.ctx.get_f(), f1)
    o.set(0, psi1)
    o.set(1, f1)
    cycles(3, first_old=psi1)  # the cycle right after the set: its err is against psiOld = psi1
    if engine == "zs":
        _timed_check(kw, o, (r, SPLIT_NAME, None))


# ---- 9. loopback slabs ----

def _loopback_dense(box, world, gather, cfg, seed, cycles=2, expect_fused=False):
    """`world` loopback ranks (after test_gpu_parity._loopback_run), each setting its own planes of the dense
    global fields; returns the gathered psi and the per-rank errs."""
    import threading

    mg = _mg()
    lb = mg.Loopback(world)
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(n=box, rank=r, world=world, gather_cells=gather, device=0,
                                          comm_id=b"\0" * 128, **cfg), loopback=lb)
            lv = ctx.levels[0]
            assert lv["distributed"] and lv["nz_local"] * world == box[2] and lv["z0"] == r * lv["nz_local"]
            psi0, f0 = dense_start(ctx, seed)
            z = slice(lv["z0"], lv["z0"] + lv["nz_local"])
            assert np.array_equal(ctx.get_psi(), psi0[z]) and np.array_equal(ctx.get_f(), f0[z])
            ctx.timing(True)
            errs = ctx.cycles(cycles)
            t = ctx.timing_read()
            ctx.timing(False)
            if expect_fused:
                assert t["fused_pre"][1] == cycles and t["fused_post"][1] == cycles and t["half_sweep"][1] == 0, t
            else:
                assert t["fused_pre"][1] == 0 and t["fused_post"][1] == 0 and t["half_sweep"][1] > 0, t
            assert t["exchange"][1] > 0, t
            out[r] = (ctx.get_psi(), errs)
            ctx.close()
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    lb.close()
    assert not errors, errors
    return np.concatenate([out[r][0] for r in range(world)], axis=0), [out[r][1] for r in range(world)]


@pytest.mark.parametrize("cid,env,fused", [
    ("slab-zs-64", dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536), True),
    ("slab-piece-64-f64", dict(MGP_FUSED=0), False),
], ids=["k_zs-f32", "per-piece-f64"])
def test_dense_loopback_slabs(cid, env, fused, monkeypatch):
    """World 2: every rank sets its own planes of the dense global fields (set_planes), so the ghost planes of
    u and of f that the first exchange delivers hold generic data.  Gathered psi == the single domain == the
    oracle, bit for bit."""
    kw, seed = case(cid)
    _env(monkeypatch, env)
    psi, errs = _loopback_dense(kw["n"], 2, 4096, {k: v for k, v in kw.items() if k != "n"}, seed, cycles=2,
                                expect_fused=fused)
    s = _Run(monkeypatch, dict(kw, gather_cells=4096), env)
    assert (s.engines()[0] == "zs") == fused
    o = Oracle(threads=8, **oracle_kw(kw))
    dense_start(o, seed)
    dense_start(s.ctx, seed)
    es = []
    for _ in range(2):
        old = o.get(0)
        eo = o.step()
        es.append(s.cycle())
        _check_err(es[-1], eo, o.get(0), old)
    assert np.array_equal(s.ctx.get_psi(), o.get(0)), "single-domain psi differs from the oracle"
    assert np.array_equal(psi, o.get(0)), "gathered slab psi differs from the oracle"
    for e in errs:
        np.testing.assert_allclose(e, es, rtol=1e-12, atol=0)
