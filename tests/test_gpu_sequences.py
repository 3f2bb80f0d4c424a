"""GPU: random call sequences through the C ABI against the per-level host model (abi_model.py).

Every other GPU file sets level 0, runs a few cycles and compares with the oracle.  Here a context is driven the way
the Lua side can drive it: cycles, the four pieces, field and plane I/O on every level, twoGrid on caller arrays,
metrics, norms, fingerprints, timing, the debugging check, the coarse-engine switch, a hybrid hand-off, mixed-precision
refinement brackets and the refused calls, in the order abi_model.sequence() draws them.  Each op runs on the model and
on the context; after EVERY op the op's own outputs, u and f of every level and psiOld (or its promised refusal) are
compared.  This is the coverage of the host layer's state across calls: per-level u / t pointers that swap or rotate,
where psiOld lives, pending lazy zeros, the hipGraph cache keyed on the pointer state, mgp_two_grid's save / restore.

Bars: fields bit for bit; err as test_gpu_parity._check_err (test_gpu_dense_fw._check_err_raw for cpu-raw.lua's float
arithmetic); residual norms 1e-12 relative to a NumPy sum of the model's fp64 residual; metrics as
test_metrics_under_temporally_blocked_finest_level; field stats as test_field_stats_match_host_restatement; the
refinement's norms and err 1e-12 (test_gpu_refine.py); everything else exact.

On a mismatch the message names the config, the seed and the op, and prints the ops so far as Python: paste them into
a test that calls _replay(monkeypatch, cid, OPS).
"""
import collections
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abi_model as A  # noqa: E402
from test_gpu_dense import _env, _mg  # noqa: E402
from test_gpu_dense_fw import _check_err_raw  # noqa: E402
from test_gpu_parity import _check_err  # noqa: E402

# level-0 temporally blocked configs: prefixes of the PRE / POST kernel a timed cycle must have run
KERNELS = {
    "zs-64x32x16": ("k_zs_split<float", "k_zs<float, false"),
    "zs-128x64x32-splitpost": ("k_zs_split<float", "k_zs_split_post<float"),
    "zs-128x64x32-two-fused": ("k_zs_split<float", "k_zs_split_post<float"),
    "zs-128x64x32-zpost": ("k_zs_split<float", None),
    "zs-64x32x64-F-warm": ("k_zs_split<float", "k_zs<float, false"),
    "zs-f64-64x32x16-pc-zero": ("k_zs<double, true", "k_zs<double, false"),
    "ys-1024-f32": ("k_ys<float, true", "k_ys<float, false"),
    "ys-1024-f64-F": ("k_ys<double, true", "k_ys<double, false"),
    "fw-zs-64x32x16": ("k_zs<float, true, 2", "k_zs<float, false"),
    "noerr-64x32x16": ("k_zs_split<float", "k_zs<float, false"),
}
# kernels of the fused levels >= 1 (fused_pre_sub / fused_post_sub)
SUB_KERNELS = {
    "zs-128x64x32-two-fused": ("k_zs", "k_zs<float, false"),
    "zs-128x64x32-zpost": ("k_zs_split_cl<float>", "k_zs<float, false"),
}


class Pair:
    """A context and its model, under the config's environment (some switches are read at launch or capture time, so
    every call runs under it again)."""

    def __init__(self, monkeypatch, cid, seed=None, every=1):
        self.mp, self.cid, self.seed, self.every = monkeypatch, cid, seed, every
        self.kw, self.env, engines = A.CONFIGS[cid]
        _env(monkeypatch, self.env)
        mg = self.mg = _mg()
        self.ctx = mg.Context(mg.make_opts(**self.kw))
        self.m = A.Model(**self.kw)
        self.done = []
        self.counts = collections.Counter()
        self.queue = []       # the model's hand-offs the context's callback has yet to make
        self.cb_errors = []
        got = [lv["engine"] for lv in self.ctx.levels]
        assert [(lv["nx"], lv["ny"]) for lv in self.ctx.levels] == [(s[-1], s[-2]) for s in self.m.shapes]
        assert all(got[l] == e for l, e in engines.items()), (cid, got, engines)
        self.engines = got

    # -- reporting --
    def fail(self, what):
        ops = "\n".join(f"    {op!r}," for op in self.done)
        pytest.fail(f"{self.cid} seed {self.seed}, op {len(self.done) - 1} {self.done[-1]!r}: {what}\n"
                    f"OPS = [\n{ops}\n]\n_replay(monkeypatch, {self.cid!r}, OPS)", pytrace=False)

    def same(self, got, want, what):
        if not (got.shape == want.shape and np.array_equal(got, want)):
            bad = np.argwhere(got != want) if got.shape == want.shape else []
            first = tuple(bad[0]) if len(bad) else None
            self.fail(f"{what} differs in {len(bad)} of {want.size} cells, first at {first}: "
                      f"{got[first] if first else got.shape!r} vs the model's {want[first] if first else want.shape!r}")

    def close(self, got, want, what, scale=None):
        tol = 1e-12 * abs(want if scale is None else scale)
        if not (abs(got - want) <= tol or (math.isnan(got) and math.isnan(want))):
            self.fail(f"{what}: {got!r} vs the model's {want!r}")

    # -- the hand-off callback: the model's own twoGrid, checked against what the context hands over --
    def _callback(self, h, u, f, n):
        if not self.queue:
            self.cb_errors.append("a hand-off the model did not make")
            raise RuntimeError
        mh, mu, mf, out = self.queue.pop(0)
        if h != mh or n != mu.shape[-1] or not np.array_equal(u, mu) or not np.array_equal(f, mf):
            self.cb_errors.append(f"hand-off (h {h!r}, size {n}) differs from the model's (h {mh!r}): u equal "
                                  f"{np.array_equal(u, mu)}, f equal {np.array_equal(f, mf)}")
        u[...] = out

    # -- one op on the context --
    def _ctx_apply(self, op):
        ctx, m, L = self.ctx, self.m, self.mg._lib
        name, a = op[0], op[1:]
        dt = m.dtype
        vp = lambda arr: arr.ctypes.data  # noqa: E731
        if name == "cycle":
            return ctx.cycle()
        if name == "cycles":
            return list(ctx.cycles(a[0]))
        if name == "set_field":
            l, which, seed = a
            data = A.dense(m.shapes[l] if 0 <= l < m.nlev else (8,), dt, seed)
            return L.check(L.lib.mgp_set_field(ctx._h, l, which, vp(data), data.size, L.MEM_HOST), ctx._h)
        if name == "set_planes":
            l, which, z, nz, seed = a
            data = A.dense((nz,) + m.shapes[l][1:], dt, seed)
            return L.check(L.lib.mgp_set_planes(ctx._h, l, which, z, nz, vp(data), L.MEM_HOST), ctx._h)
        if name == "get_planes":
            l, which, z, nz = a
            out = np.full((nz,) + m.shapes[l][-2:], 7, dt)
            L.check(L.lib.mgp_get_planes(ctx._h, l, which, z, nz, vp(out), L.MEM_HOST), ctx._h)
            return out
        if name == "get_field":
            l, which = a
            out = np.full(m.shapes[l] if 0 <= l < m.nlev else (8,), 7, dt)
            L.check(L.lib.mgp_get_field(ctx._h, l, which, vp(out), out.size, L.MEM_HOST), ctx._h)
            return out
        if name == "two_grid":
            size, hmode, seed = a
            shp = m.shapes[m.sizes.index(size)] if size in m.sizes else (8,)
            u, f = A.dense(shp, dt, seed), A.dense(shp, dt, seed + 1)
            h = m.two_grid_h(size, hmode) if size in m.sizes else 1.0
            L.check(L.lib.mgp_two_grid(ctx._h, h, vp(u), vp(f), size, L.MEM_HOST), ctx._h)
            return u
        if name == "smooth":
            return L.check(L.lib.mgp_smooth(ctx._h, a[0], a[1]), ctx._h)
        if name in ("residual_restrict", "prolong_correct"):
            return L.check(getattr(L.lib, "mgp_" + name)(ctx._h, a[0]), ctx._h)
        if name == "residual_norm":
            return ctx.residual_norm(a[0])
        if name == "field_stats":
            return ctx.field_stats(a[1], a[0])
        if name == "timing":
            return ctx.timing(bool(a[0]))
        if name == "set_debug":
            return ctx.set_debug(a[0])
        if name == "set_coarse_level":
            return ctx.set_coarse_level(a[0])
        if name == "set_coarse_handoff":
            return ctx.set_coarse_handoff(a[0], self._callback if a[1] else None)
        if name == "cg_solve":
            ctx.cg_solve(maxiter=a[0])
            return None
        if name == "refine_set":
            return ctx.refine_set(a[0], np.random.default_rng(a[1]).uniform(-1.0, 1.0, m.shapes[0]))
        if name == "refine_step":
            return ctx.refine_step(a[0])
        return getattr(ctx, name)(*a)  # coarse_solve, metrics, sync, refine_begin / _end / _get / _residual

    def _outputs(self, op, got, want):
        name, m = op[0], self.m
        if name in ("cycle", "cycles"):
            got, want = (got, want) if name == "cycles" else ([got], [want])
            if len(got) != len(want):
                self.fail(f"{len(got)} errs")
            for i, (g, w) in enumerate(zip(got, want)):
                if not self.kw.get("err_mode", 1):
                    if not math.isnan(g):
                        self.fail(f"err {g!r} with err_mode 0")
                    continue
                old, new = m.cycle_log[i]
                try:
                    (_check_err_raw if m.arith == "double" else _check_err)(g, w, new, old)
                except AssertionError as e:
                    self.fail(f"err of cycle {i + 1} of the call: {g!r} vs the model's {w!r} ({e})")
        elif name in ("get_field", "get_planes", "two_grid", "refine_get"):
            self.same(got, want.reshape(got.shape), "the output")
        elif name == "metrics":
            if got[1] != want[1]:
                self.fail(f"metrics count {got[1]} vs the model's {want[1]}")
            self.close(got[0], want[0], "rel_err")
            self.close(got[2], want[2], "frob")
        elif name in ("residual_norm", "refine_residual", "refine_step"):
            for g, w, what in zip(got, want, ("rnorm", "fnorm", "err")):
                self.close(g, w, what)
        elif name == "field_stats":
            l, which = op[1], op[2]
            d = (m.u if which == A.U else m.f)[l].astype(np.float64)
            if got[0] != want[0]:
                self.fail(f"hash {got[0]:#x} vs the model's {want[0]:#x}")
            self.close(got[1], want[1], "sum", np.abs(d).sum())
            self.close(got[2], want[2], "sum of squares")
            if got[3] != want[3]:
                self.fail(f"max |x| {got[3]!r} vs {want[3]!r}")

    def state(self):
        ctx, m, mg = self.ctx, self.m, self.mg
        for l in range(m.nlev):
            self.same(ctx.get_field(mg.FIELD_U, l), m.u[l], f"u of level {l}")
            self.same(ctx.get_field(mg.FIELD_F, l), m.f[l], f"f of level {l}")
        if m.psi_old is not None:
            try:
                self.same(ctx.get_field(mg.FIELD_PSI_OLD), m.psi_old, "psiOld")
            except mg.MGPError as e:
                self.fail(f"psiOld refused ({e}) where the model has one")
        else:
            try:
                ctx.get_field(mg.FIELD_PSI_OLD)
                self.fail("psiOld returned where no outer iteration left one")
            except mg.MGPError as e:
                if e.code != A.ERR_STATE:
                    self.fail(f"psiOld refusal with status {e.code}")
        if m.refining():
            self.same(ctx.refine_get(A.REFINE_PSI), m.psi64, "the refinement's psi")
            self.same(ctx.refine_get(A.REFINE_F), m.f64, "the refinement's f")

    def run(self, op):
        _env(self.mp, self.env)
        self.done.append(op)
        try:
            want, refused = self.m.apply(op), None
        except A.Refusal as r:
            want, refused = None, r.status
        self.queue = list(self.m.handoff_log)
        try:
            got, status = self._ctx_apply(op), None
        except self.mg.MGPError as e:
            got, status = None, e.code
        if self.cb_errors:
            self.fail("; ".join(self.cb_errors))
        if status != refused:
            self.fail(f"status {status} vs the model's {refused}")
        if self.queue:
            self.fail(f"{len(self.queue)} hand-offs of the model the context did not make")
        if refused is None:
            self.counts[op[0]] += 1
            self._outputs(op, got, want)
        else:
            self.counts["refused"] += 1
        if len(self.done) % self.every == 0:
            self.state()

    def timed_cycle(self):
        """As test_gpu_dense._timed_check: one eager cycle under mgp_timing ran level 0's phases as one launch each
        on the kernels of KERNELS, and the levels of SUB_KERNELS theirs."""
        self.run(("timing", 1))
        self.run(("cycle",))
        t, k = self.ctx.timing_read(), self.ctx.timing_kernels()
        self.run(("timing", 0))
        pre, post = KERNELS[self.cid]
        assert t["fused_pre"][1] == 1 and t["fused_post"][1] == 1 and t["half_sweep"][1] == 0, t
        assert k["fused_pre"][0].startswith(pre), k
        assert post is None or k["fused_post"][0].startswith(post), k
        if self.cid in SUB_KERNELS:
            spre, spost = SUB_KERNELS[self.cid]
            assert t["fused_pre_sub"][1] >= 1 and t["fused_post_sub"][1] >= 1, t
            assert k["fused_pre_sub"][0].startswith(spre) and k["fused_post_sub"][0].startswith(spost), k


def _replay(monkeypatch, cid, ops, seed=None, every=1):
    """every: u / f / psiOld of every level are read back after every that-many-th op (and after the last)."""
    p = Pair(monkeypatch, cid, seed, every)
    for op in ops:
        p.run(op)
    if len(ops) % every:
        p.state()
    return p


RUNS = [(cid, s) for cid in A.CONFIGS for s in A.SEEDS]


@pytest.mark.parametrize("cid,seed", RUNS, ids=[f"{c}-{s}" for c, s in RUNS])
def test_random_sequence_matches_the_model(cid, seed, monkeypatch):
    p = _replay(monkeypatch, cid, A.sequence(cid, seed), seed)
    if cid in KERNELS and seed == A.SEEDS[0]:
        p.timed_cycle()
    print(f"{cid} seed {seed}: engines {p.engines}; ops {dict(sorted(p.counts.items()))}")


@pytest.mark.parametrize("cid", sorted(A.CONFIGS))
def test_random_sequence_with_sparse_reads(cid, monkeypatch):
    """Reading u of a level materialises its pending lazy zero, so the read-back after every op above never lets one
    survive into the next call.  The first seed's sequence again with the state read back after every 7th op only
    (each op's own outputs are still compared): pending zeros and rotated buffers carry over from call to call."""
    _replay(monkeypatch, cid, A.sequence(cid, A.SEEDS[0]), A.SEEDS[0], every=7)


# ---- deterministic sequences ----

@pytest.mark.parametrize("cid", sorted(A.GRAPH_CAP))
def test_graph_cache_cap(cid, monkeypatch):
    """More than 8 distinct buffer-pointer states: an odd number of Jacobi sweeps flips u / t of one level, so a walk
    of single sweeps down the levels gives a new state before every mgp_cycles call, past the 8 entries the hipGraph
    cache holds (one is captured at creation); from there the cycles run eagerly.  With 2 + 1 sweeps every cycle
    flips the per-piece levels itself, so one mgp_cycles(3) call alternates between two states, and replayed, freshly
    captured and eager cycles meet in one call.  u and f of every level and every err equal the model's."""
    monkeypatch.setitem(A.CONFIGS, cid, A.EXTRA[cid])
    ops = A.graph_cap_ops(cid)
    assert sum(op[0] == "smooth" for op in ops) > 8
    _replay(monkeypatch, cid, ops)


def test_psi_old_is_refused_while_refining(monkeypatch):
    """Found by the sequences: after mgp_refine_step MGP_FIELD_PSI_OLD returned the inner fp32 cycles' psiOld, after
    mgp_refine_begin / _residual it was refused.  Decided (include/mgpoisson.h): while refinement is active the outer
    iteration is the fp64 one, whose psiOld is not stored, so PSI_OLD / ERROR are refused like mgp_metrics, and after
    mgp_refine_end until the next outer iteration.  (Pair.state() reads psiOld after every op.)"""
    p = _replay(monkeypatch, "zs-64x32x16", [
        ("set_field", 0, A.U, 31), ("set_field", 0, A.F, 32), ("cycle",), ("get_field", 0, A.PSI_OLD),
        ("refine_begin",), ("get_field", 0, A.PSI_OLD), ("refine_step", 2), ("get_field", 0, A.PSI_OLD),
        ("get_field", 0, A.ERROR), ("metrics",), ("refine_end",), ("get_field", 0, A.PSI_OLD), ("cycle",),
        ("get_field", 0, A.PSI_OLD), ("metrics",)])
    assert p.counts["refused"] == 5


@pytest.mark.parametrize("cid", A.TWO_GRID_CIDS)
def test_two_grid_keeps_psi_old(cid, monkeypatch):
    """twoGrid never touches psiOld (cpu-raw.lua sets it in the outer loop only): after mgp_two_grid at the finest
    size, with the level's h (the engines run) and with 2 / n (one launch per piece), mgp_metrics, MGP_FIELD_PSI_OLD
    and MGP_FIELD_ERROR still describe the last outer iteration, and the next cycle's err and psi are the model's.
    (Pair.state() reads psiOld after every op as well.)"""
    _replay(monkeypatch, cid, A.two_grid_ops(cid))


# ---- world 2 through the loopback transport ----

def _slab_rank(mg, ctx, m, ops, rec):
    """One rank: execute every op on its part and record (status, output, its planes of u and f of every level, its
    planes of psiOld or the refusal's status).  Nothing is compared here: a failed comparison must not strand the
    peer in a barrier."""
    L = mg._lib
    dt = m.dtype

    def part(l, z, nz):
        """The rank's share of the global planes [z, z + nz) of level l: (local begin, global begin, count)."""
        lv = ctx.levels[l]
        z0, own = (lv["z0"], lv["nz_local"]) if lv["distributed"] else (0, lv["nz_global"])
        lo, hi = max(z, z0), min(z + nz, z0 + own)
        return (lo - z0, lo, hi - lo) if hi > lo else (0, z0, 0)  # (every rank calls, with no plane if it has none)

    def apply(op):
        name, a = op[0], op[1:]
        if name == "set_planes":
            l, which, z, nz, seed = a
            data = A.dense((nz,) + m.shapes[l][1:], dt, seed)
            loc, glo, cnt = part(l, z, nz)
            mine = np.ascontiguousarray(data[glo - z:glo - z + cnt]) if cnt else np.zeros(1, dt)
            return L.check(L.lib.mgp_set_planes(ctx._h, l, which, loc, cnt, mine.ctypes.data, L.MEM_HOST), ctx._h)
        if name == "get_planes":
            l, which, z, nz = a
            loc, glo, cnt = part(l, z, nz)
            out = np.full((max(cnt, 1),) + m.shapes[l][1:], 7, dt)
            L.check(L.lib.mgp_get_planes(ctx._h, l, which, loc, cnt, out.ctypes.data, L.MEM_HOST), ctx._h)
            return glo, out[:cnt]
        if name == "cycle":
            return ctx.cycle()
        if name == "cycles":
            return list(ctx.cycles(a[0]))
        if name == "two_grid":
            u = A.dense(m.shapes[m.sizes.index(a[0])], dt, a[2])
            return L.check(L.lib.mgp_two_grid(ctx._h, 1.0, u.ctypes.data, u.ctypes.data, a[0], L.MEM_HOST), ctx._h)
        if name == "cg_solve":
            return ctx.cg_solve(maxiter=a[0])
        if name == "field_stats":
            return ctx.field_stats(a[1], a[0])
        return getattr(ctx, name)(*a)  # the pieces, residual_norm, metrics, refine_begin

    for op in ops:
        try:
            out, status = apply(op), None
        except mg.MGPError as e:
            out, status = None, e.code
        planes = [(ctx.get_field(mg.FIELD_U, l), ctx.get_field(mg.FIELD_F, l)) for l in range(m.nlev)]
        try:
            old = ctx.get_field(mg.FIELD_PSI_OLD)
        except mg.MGPError as e:
            old = e.code
        rec.append((status, out, planes, old))


@pytest.mark.parametrize("cid,seed", [(c, s) for c in A.SLAB_CONFIGS for s in A.SEEDS[:2]],
                         ids=[f"{c}-{s}" for c in A.SLAB_CONFIGS for s in A.SEEDS[:2]])
def test_slab_sequence_matches_the_model(cid, seed, monkeypatch):
    """World 2, every rank executing abi_model.slab_sequence(): the ranks' planes of u and f of every level (levels
    0 and 1 distributed, the rest replicated) equal the one-domain model's after every op, the outputs agree, the
    ranks' hashes add up to the model's, and mgp_two_grid / mgp_cg_solve / mgp_refine_begin are refused.  The ranks
    only execute and record; the comparison runs here after the join."""
    import threading

    from test_gpu_dense import SWITCHES

    kw, env = A.SLAB_CONFIGS[cid]
    for k in SWITCHES + ("MGP_DEEP_HALO",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    mg = _mg()
    world = A.SLAB_WORLD
    ops = A.slab_sequence(cid, seed)
    m = A.Model(world=world, **kw)
    lb = mg.Loopback(world)
    recs, errors, levels = [[] for _ in range(world)], [], [None] * world

    def rank_main(r):
        try:
            ctx = mg.Context(mg.make_opts(rank=r, world=world, gather_cells=A.SLAB_GATHER, device=0,
                                          comm_id=b"\0" * 128, **kw), loopback=lb)
            levels[r] = ctx.levels
            _slab_rank(mg, ctx, m, ops, recs[r])
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
    dist = [lv["distributed"] for lv in levels[0]]
    assert dist[:3] == [True, True, False] and [lv["engine"] for lv in levels[0]][0] == ("zs" if "zs" in cid else "piece")

    done, counts = [], collections.Counter()

    def fail(what):
        text = "\n".join(f"    {op!r}," for op in done)
        pytest.fail(f"{cid} seed {seed}, op {len(done) - 1} {done[-1]!r}: {what}\nOPS = [\n{text}\n]", pytrace=False)

    def slab(r, l, a):
        lv = levels[r][l]
        return a[lv["z0"]:lv["z0"] + lv["nz_local"]] if lv["distributed"] else a

    for i, op in enumerate(ops):
        done.append(op)
        try:
            want, refused = m.apply(op), None
        except A.Refusal as x:
            want, refused = None, x.status
        counts["refused" if refused is not None else op[0]] += 1
        for r in range(world):
            status, got, planes, old = recs[r][i]
            if status != refused:
                fail(f"rank {r}: status {status} vs the model's {refused}")
            for l in range(m.nlev):
                for a, b, what in ((planes[l][0], m.u[l], "u"), (planes[l][1], m.f[l], "f")):
                    if not np.array_equal(a, slab(r, l, b)):
                        fail(f"rank {r}: {what} of level {l} differs in {int((a != slab(r, l, b)).sum())} cells")
            if m.psi_old is None:
                if not (isinstance(old, int) and old == A.ERR_STATE):
                    fail(f"rank {r}: psiOld returned where the model has none")
            elif isinstance(old, int) or not np.array_equal(old, slab(r, 0, m.psi_old)):
                fail(f"rank {r}: psiOld " + (f"refused ({old})" if isinstance(old, int) else "differs"))
            if refused is not None:
                continue
            if op[0] in ("cycle", "cycles"):
                for j, (g, w) in enumerate(zip([got] if op[0] == "cycle" else got, [want] if op[0] == "cycle" else want)):
                    try:
                        _check_err(g, w, m.cycle_log[j][1], m.cycle_log[j][0])
                    except AssertionError as e:
                        fail(f"rank {r}: err of cycle {j + 1} of the call ({e})")
            elif op[0] == "get_planes":
                glo, arr = got
                if not np.array_equal(arr, want[glo - op[3]:glo - op[3] + arr.shape[0]]):
                    fail(f"rank {r}: planes from global {glo} differ")
            elif op[0] == "residual_norm":
                if not all(abs(g - w) <= 1e-12 * w for g, w in zip(got, want)):
                    fail(f"rank {r}: norms {got} vs {want}")
            elif op[0] == "metrics":
                if got[1] != want[1] or not all(abs(got[k] - want[k]) <= 1e-12 * abs(want[k]) for k in (0, 2)):
                    fail(f"rank {r}: metrics {got} vs {want}")
        if refused is None and op[0] == "field_stats":
            l, which = op[1], op[2]
            parts = [recs[r][i][1] for r in range(world)]
            if dist[l]:  # the ranks' hashes and sums add up to the global ones
                h = sum(p[0] for p in parts) & A.M64
                s1, s2, mx = sum(p[1] for p in parts), sum(p[2] for p in parts), max(p[3] for p in parts)
            else:
                assert all(p == parts[0] for p in parts), parts
                h, s1, s2, mx = parts[0]
            d = (m.u if which == A.U else m.f)[l].astype(np.float64)
            if h != want[0] or mx != want[3] or abs(s1 - want[1]) > 1e-12 * np.abs(d).sum() or abs(s2 - want[2]) > 1e-12 * want[2]:
                fail(f"field stats {(h, s1, s2, mx)} vs the model's {want}")
    print(f"{cid} seed {seed}: distributed {dist}; ops {dict(sorted(counts.items()))}")
