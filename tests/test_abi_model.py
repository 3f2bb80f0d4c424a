"""CPU guard of the ABI model and the sequence generator (abi_model.py) that test_gpu_sequences.py drives contexts with.

1. The model is the reference: its cycles equal the C oracle's step() bit for bit (psi identical, err the same
   double) over 4 cycles from dense fields on every configuration of the GPU file and on the option corners; its
   two_grid equals the oracle's; its stored coarse levels equal the warm buffers of the NumPy oracle
   (mgp_oracle_np.Multigrid.V), the only oracle that exposes them.
2. The sequences are fit to compare bit for bit.  For every (config, seed) the GPU file runs, the model alone must
   keep every stored value finite and inside [1e-25, 1e25] (float; 1e-150 .. 1e150 double) or exactly zero after
   every op, at most 15 % of the ops may be refusals, and over a config's seeds every op kind must occur and every
   level must be the target of a piece and of a field write.  These are conditions on the generator, not
   measurements: seeds and lengths are chosen so that they hold.
"""
import functools

import mgp_oracle_np as N
import numpy as np
import pytest

import abi_model as A
from dense_start import FW, LC, RAW, RB, dense_fields, oracle_kw
from oracle_lib import Oracle

# the option corners of the composition (beside every CONFIGS entry)
CORNERS = {
    "3d-64x32x16-f32-rbgs": dict(dim=3, n=(64, 32, 16), real="float", **RB, **LC),
    "3d-32-f64-F-warm": dict(dim=3, n=(32, 32, 32), real="double", cycle="F", coarse_init="warm", **RB, **LC),
    "2d-64-f64-jacobi-warm": dict(dim=2, n=(64, 64, 1), real="double", coarse_init="warm"),
    "2d-64x32-raw-warm": dict(dim=2, n=(64, 32, 1), coarse_init="warm", **RAW),
    "3d-32x16x16-f32-fw-F": dict(dim=3, n=(32, 16, 16), real="float", cycle="F", **RB, **LC, **FW),
    "2d-32-gslex-1-3-linear": dict(dim=2, n=(32, 32, 1), real="double", smoother="gs_lex", nu1=1, nu2=3, prolong="linear"),
    "3d-16-f32-nu1-0": dict(dim=3, n=(16, 16, 16), real="float", smoother="rbgs", nu1=0, nu2=2, **LC),
}
ALL = dict({cid: v[0] for cid, v in A.CONFIGS.items()}, **CORNERS)


def _seed(cid):
    return 2001 + 20 * sorted(ALL).index(cid)


@pytest.mark.parametrize("cid", sorted(ALL))
def test_model_cycles_equal_the_oracle(cid):
    kw = ALL[cid]
    m, o = A.Model(**kw), Oracle(threads=8, **oracle_kw(kw))
    psi0, f0 = dense_fields(m.shapes[0], m.dtype, _seed(cid))
    o.set(0, psi0)
    o.set(1, f0)
    m.set_field(0, A.U, psi0)
    m.set_field(0, A.F, f0)
    for it in range(4):
        old = m.u[0].copy()
        e_m, e_o = m.cycle(), o.step()
        assert np.array_equal(m.u[0], o.get(0)), f"psi differs after cycle {it + 1}"
        if kw.get("err_mode", 1):
            assert e_m == e_o, (it + 1, e_m, e_o)
            assert np.array_equal(m.psi_old, old)
        else:
            assert np.isnan(e_m) and m.psi_old is None
    assert np.array_equal(m.f[0], f0)


@pytest.mark.parametrize("cid", sorted(CORNERS) + ["zs-64x32x16", "blk-32-f64-F", "jacobi-256-f64-warm"])
def test_model_two_grid_equals_the_oracle(cid):
    """From every level size, with the level's own h and with twice it; the level's own u / f and psiOld stay."""
    kw = ALL[cid]
    m, o = A.Model(**kw), Oracle(**oracle_kw(kw))
    m.apply(("set_field", 0, A.U, 3))
    m.apply(("set_field", 0, A.F, 4))
    o.set(0, m.u[0])
    o.set(1, m.f[0])
    m.cycle()  # (an outer iteration, so that there is a psiOld to keep; the oracle's too: the warm guesses below)
    o.step()
    old = m.psi_old.copy()
    for l, size in enumerate(m.sizes):
        for hmode in ("level", "2/n"):
            u, f = dense_fields(m.shapes[l], m.dtype, _seed(cid) + 2 * l)
            before = (m.u[l].copy(), m.f[l].copy())
            h = m.two_grid_h(size, hmode)
            got = m.two_grid(h, u, f, size)
            want = u.copy()
            o.two_grid(h, want, f, size)
            assert np.array_equal(got, want), (l, hmode)
            assert np.array_equal(m.u[l], before[0]) and np.array_equal(m.f[l], before[1])
            assert np.array_equal(m.psi_old, old)


NP = dict(smoother={"jacobi": N.JACOBI, "rbgs": N.RBGS}, cycle={"V": N.CYCLE_V, "F": N.CYCLE_F},
          prolong={"pc": N.PROLONG_PC, "linear": N.PROLONG_LINEAR}, init={"fresh": N.COARSE_FRESH, "warm": N.COARSE_WARM},
          bc={"zero": N.BC_ZERO, "consistent": N.BC_CONSISTENT},
          restriction={"average": N.RESTRICT_AVERAGE, "full_weighting": N.RESTRICT_FULL_WEIGHTING})


@pytest.mark.parametrize("cid", ["3d-32-f64-F-warm", "2d-64-f64-jacobi-warm", "2d-64x32-raw-warm", "3d-64x32x16-f32-rbgs",
                                 "3d-32x16x16-f32-fw-F"])
def test_model_coarse_levels_equal_the_numpy_oracles_warm_buffers(cid):
    """u[l] below the finest level is Vs[l] of the last visit (cpu-raw.lua:221): the NumPy oracle keeps exactly that
    in Multigrid.V, warm or fresh."""
    kw = A.Model(**ALL[cid]).kw
    m = A.Model(**ALL[cid])
    g = N.Multigrid(dim=kw["dim"], n=kw["n"], dtype=m.dtype, nu1=kw["nu1"], nu2=kw["nu2"], smoother=NP["smoother"][kw["smoother"]],
                    cycle=NP["cycle"][kw["cycle"]], prolong_kind=NP["prolong"][kw["prolong"]],
                    coarse_init=NP["init"][kw["coarse_init"]], coarse_sweeps=kw["coarse_sweeps"],
                    coarse_bc=NP["bc"][kw["coarse_bc"]], restriction=NP["restriction"][kw["restriction"]], arith=m.arith)
    psi0, f0 = dense_fields(m.shapes[0], m.dtype, _seed(cid))
    g.psi, g.f = psi0.reshape(g.shapes[0]).copy(), f0.reshape(g.shapes[0]).copy()  # (its 2D arrays are (1, ny, nx))
    m.set_field(0, A.U, psi0)
    m.set_field(0, A.F, f0)
    for it in range(3):
        e_g, e_m = g.step(), m.cycle()
        assert np.array_equal(m.u[0], g.psi.reshape(m.shapes[0])), it + 1
        assert abs(e_g - e_m) <= 1e-12 * e_m
        for l in range(1, m.nlev):
            assert np.array_equal(m.u[l], g.V[l].reshape(m.shapes[l])), (it + 1, l)


def test_fingerprint_is_test_gpu_larges():
    """The vectorised hash equals the cell-by-cell restatement of test_gpu_large.fingerprint."""
    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & A.M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & A.M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & A.M64
        return z ^ (z >> 31)

    for dt, ut in ((np.float32, np.uint32), (np.float64, np.uint64)):
        a = A.dense((3, 4, 8), dt, 5)
        h = 0
        for i, b in enumerate(a.view(ut).ravel()):
            h = (h + mix(int(b) ^ mix(2 * 32 + i))) & A.M64
        assert A.fingerprint(a, z0=2) == h


def test_refusals_leave_the_model_unchanged():
    m = A.Model(dim=3, n=(16, 16, 16), real="float", **RB, **LC)
    m.apply(("set_field", 0, A.U, 1))
    m.apply(("set_field", 0, A.F, 2))
    before = [a.copy() for _, a in m.stored()]
    for op, status in [(("metrics",), A.ERR_STATE), (("get_field", 0, A.PSI_OLD), A.ERR_STATE),
                       (("get_planes", 0, A.U, 10, 7), A.ERR_ARG), (("two_grid", 3, "level", 5), A.ERR_ARG),
                       (("set_field", 1, A.RESIDUAL, 5), A.ERR_ARG), (("set_coarse_level", 3), A.ERR_ARG),
                       (("set_coarse_level", 16), A.ERR_ARG), (("refine_end",), A.ERR_STATE),
                       (("get_field", m.nlev - 1, A.CORRECTION), A.ERR_ARG), (("smooth", m.nlev, 1), A.ERR_ARG)]:
        with pytest.raises(A.Refusal) as e:
            m.apply(op)
        assert e.value.status == status, op
    m.apply(("refine_begin",))
    for op in [("cycle",), ("cycles", 2), ("two_grid", 16, "level", 5), ("metrics",), ("cg_solve", 2),
               ("set_field", 0, A.U, 5), ("set_planes", 0, A.F, 0, 2, 5), ("refine_begin",)]:
        with pytest.raises(A.Refusal) as e:
            m.apply(op)
        assert e.value.status == A.ERR_STATE, op
    m.apply(("refine_end",))
    assert all(np.array_equal(a, b) for (_, a), b in zip(m.stored(), before))
    with pytest.raises(A.Refusal) as e:
        A.Model(dim=2, n=(16, 16, 1)).apply(("refine_begin",))
    assert e.value.status == A.ERR_ARG


# ---- the generator guards ----

@functools.lru_cache(maxsize=None)
def _run(cid, seed):
    """The model alone over the sequence (seed "graph-cap" / "two-grid": the deterministic ones): (ops, refused ops,
    (lo, hi) of the stored nonzero magnitudes, the first op after which a stored value left the admitted range or
    None)."""
    m = A.Model(**(A.EXTRA[cid] if seed == "graph-cap" else A.CONFIGS[cid])[0])
    ops = (A.graph_cap_ops(cid) if seed == "graph-cap" else A.two_grid_ops(cid) if seed == "two-grid" else
           A.sequence(cid, seed))
    big, small = (1e25, 1e-25) if m.dtype == np.float32 else (1e150, 1e-150)
    refused, lo, hi, bad = [], np.inf, 0.0, None
    for i, op in enumerate(ops):
        try:
            m.apply(op)
        except A.Refusal:
            refused.append(i)
        for name, a in m.stored():
            mag = np.abs(a[a != 0]).astype(np.float64)
            ok = bool(np.all(np.isfinite(a))) and (mag.size == 0 or (mag.max() <= big and mag.min() >= small))
            if mag.size and ok:
                lo, hi = min(lo, float(mag.min())), max(hi, float(mag.max()))
            if not ok and bad is None:
                bad = (i, op, name)
    return ops, refused, (lo, hi), bad


PAIRS = [(cid, s) for cid in A.CONFIGS for s in A.SEEDS]


@pytest.mark.parametrize("cid,seed", PAIRS, ids=[f"{c}-{s}" for c, s in PAIRS])
def test_sequence_stays_in_range_and_mostly_executes(cid, seed):
    ops, refused, (lo, hi), bad = _run(cid, seed)
    print(f"{cid} seed {seed}: {len(ops)} ops, {len(refused)} refused, stored |x| in [{lo:.3g}, {hi:.3g}]")
    assert ops == A.sequence(cid, seed)  # a function of (config, seed, length) alone
    assert A.LENGTH <= len(ops) <= A.LENGTH + 12
    assert bad is None, bad
    assert len(refused) <= 0.15 * len(ops), (len(refused), len(ops))


FIXED = [(cid, "graph-cap") for cid in sorted(A.GRAPH_CAP)] + [(cid, "two-grid") for cid in A.TWO_GRID_CIDS]


@pytest.mark.parametrize("cid,which", FIXED, ids=[f"{c}-{w}" for c, w in FIXED])
def test_deterministic_sequences_stay_in_range(cid, which):
    ops, refused, (lo, hi), bad = _run(cid, which)
    print(f"{cid} {which}: {len(ops)} ops, stored |x| in [{lo:.3g}, {hi:.3g}]")
    assert bad is None, bad
    assert not refused


@pytest.mark.parametrize("cid", sorted(A.CONFIGS))
def test_seeds_cover_every_kind_and_level(cid):
    m = A.Model(**A.CONFIGS[cid][0])
    kinds, pieces, writes = set(), set(), set()
    refused_kinds = set()
    for seed in A.SEEDS:
        ops, refused, _, _ = _run(cid, seed)
        for i, op in enumerate(ops):
            if i in refused:
                refused_kinds.add(op[0])
                continue
            kinds.add(op[0])
            if op[0] in ("smooth", "residual_restrict", "prolong_correct"):
                pieces.add(op[1])
            if op[0] == "coarse_solve":
                pieces.add(m.nlev - 1)
            if op[0] in ("set_field", "set_planes"):
                writes.add(op[1])
    want = set(A.KINDS)
    if m.dim == 2:
        want -= {"set_planes", "get_planes"}
    if m.dtype == np.float32 and m.arith == "real":
        want |= set(A.REFINE_KINDS)
    if not m.kw["err_mode"]:  # no psiOld, ever: the call is there, and refused
        want -= {"metrics"}
        assert "metrics" in refused_kinds
    assert want <= kinds, sorted(want - kinds)
    assert refused_kinds, "no refusal in any seed"
    assert pieces == set(range(m.nlev)), sorted(set(range(m.nlev)) - pieces)
    assert writes == set(range(m.nlev)), sorted(set(range(m.nlev)) - writes)


SLABS = [(cid, s) for cid in A.SLAB_CONFIGS for s in A.SEEDS[:2]]


@pytest.mark.parametrize("cid,seed", SLABS, ids=[f"{c}-{s}" for c, s in SLABS])
def test_slab_sequence_guards(cid, seed):
    """The world-2 sequences on the one-domain model: value range, refusal share, and within each sequence every op
    kind, with writes and pieces on distributed (0, 1) and replicated levels."""
    m = A.Model(world=A.SLAB_WORLD, **A.SLAB_CONFIGS[cid][0])
    ops = A.slab_sequence(cid, seed)
    assert ops == A.slab_sequence(cid, seed)
    big, small = (1e25, 1e-25) if m.dtype == np.float32 else (1e150, 1e-150)
    refused, kinds, writes, pieces = 0, set(), set(), set()
    for i, op in enumerate(ops):
        try:
            m.apply(op)
            kinds.add(op[0])
        except A.Refusal as r:
            refused += 1
            assert op[0] in ("two_grid", "cg_solve", "refine_begin", "metrics") and r.status in (A.ERR_STATE, A.ERR_ARG), op
        for name, a in m.stored():
            mag = np.abs(a[a != 0]).astype(np.float64)
            assert np.all(np.isfinite(a)) and (mag.size == 0 or (mag.max() <= big and mag.min() >= small)), (i, op, name)
        if op[0] == "set_planes":
            writes.add(op[1])
        if op[0] in ("smooth", "residual_restrict", "prolong_correct"):
            pieces.add(op[1])
    assert refused <= 0.15 * len(ops), (refused, len(ops))
    assert {"set_planes", "cycle", "smooth"} <= kinds
    for levels in (writes, pieces):
        assert levels & {0, 1} and levels & set(range(2, m.nlev)), levels


def test_slab_seeds_cover_every_kind():
    for cid in A.SLAB_CONFIGS:
        seen = {op[0] for s in A.SEEDS[:2] for op in A.slab_sequence(cid, s)}
        assert set(A.SLAB_KINDS) <= seen, sorted(set(A.SLAB_KINDS) - seen)
