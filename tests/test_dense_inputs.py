"""CPU guard of the dense start states (dense_start.py) that test_gpu_dense.py and test_gpu_dense_fw.py compare the
GPU with the oracle on.

The GPU comparison is bit for bit, so it needs inputs on which a mismatch can only be an indexing or ordering
error: for every (box, real, options) of dense_start.CASES, three oracle steps from the dense start must leave psi
finite with no zero and no subnormal cell (a flush-to-zero difference or an overflow would otherwise look like a
wrong load), and err must fall from cycle to cycle (the start is one the solver converges from, not noise it
amplifies).  This is a condition on the reference alone, not a measurement of the GPU.

err of the reference with seeds 101 / 102: 64 x 32 x 16 fp32 0.577, 0.0132, 8.8e-4; 128^3 fp32 0.576, 0.0131,
9.1e-4; 1024^2 fp32 0.575, 0.0099, 5.3e-4; 256^2 fp64 Jacobi 0.569, 0.034, 0.017.  Two non-square 2D red/black
cases with coarse_bc = zero do not fall monotonically in the reference and are held to errs[2] < errs[0] only:
1024 x 512 fp64 linear goes 0.576, 0.078, 0.107; 512 x 256 fp32 pc goes 0.579, 0.088, 0.126.  (A case whose err
grows past its first value is not admitted at all: dense_start.py names the one configuration left out for that.)
"""
import numpy as np
import pytest

from dense_start import CASES, RESET_SEED_OFFSET, SECOND_FIELDS, case, dense_fields, dense_start, oracle_kw
from oracle_lib import Oracle

NOT_MONOTONE = {"ys-1024x512-f64-zero", "blk2-512x256-f32"}

assert all(cid in SECOND_FIELDS for cid in CASES if cid.startswith("reset-"))
STARTS = [(cid, 0) for cid in CASES] + [(cid, RESET_SEED_OFFSET) for cid in CASES if cid in SECOND_FIELDS]


@pytest.mark.parametrize("cid,offset", STARTS, ids=[c if not s else f"{c}-second-fields" for c, s in STARTS])
def test_reference_is_well_conditioned_from_the_dense_start(cid, offset):
    kw, seed = case(cid)
    o = Oracle(threads=8, **oracle_kw(kw))
    psi0, f0 = dense_start(o, seed + offset)
    assert np.array_equal(o.get(0), psi0) and np.array_equal(o.get(1), f0)
    tiny = np.finfo(o.dtype).tiny
    errs = []
    for it in range(3):
        errs.append(o.step())
        psi = o.get(0)
        assert np.all(np.isfinite(psi)), f"cycle {it + 1}"
        # no zero and no subnormal cell: min |psi| is a normal number
        assert np.abs(psi).min() >= tiny, (it + 1, float(np.abs(psi).min()))
    assert all(np.isfinite(errs)), errs
    if cid in NOT_MONOTONE:
        assert errs[2] < errs[0], errs
    else:
        assert errs[0] > errs[1] > errs[2], errs


def test_dense_fields_are_deterministic_and_distinct():
    a = dense_fields((16, 8, 4), np.float32, 101)
    b = dense_fields((16, 8, 4), np.float32, 101)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[0].dtype == np.float32 and dense_fields((4, 4), np.float64, 7)[0].dtype == np.float64
    assert not np.array_equal(a[0], a[1])  # psi0 and f0 come from different generators
    assert not np.array_equal(a[0], dense_fields((16, 8, 4), np.float32, 103)[0])
    seeds = [s for _, s in CASES.values()]
    # no case's psi or f seed (seed, seed + 1, and the reset cases' second pair) is another's
    used = [s + d for s in seeds for d in (0, 1, RESET_SEED_OFFSET, RESET_SEED_OFFSET + 1)]
    assert len(set(used)) == len(used)


@pytest.mark.parametrize("cid", ["zs-64x32x16", "ys-1024-f32", "jacobi-256-f64"])
def test_dense_f_has_no_zero_cell_where_the_point_charge_has_one_nonzero(cid):
    """Why the dense start exists: from init_point_charge() all but one level-0 load of f (and of psi in the first
    cycle) reads a zero, so a load of the wrong cell goes unseen; the dense fields have no zero at all and no
    mirror symmetry a swapped index could hide behind."""
    kw, seed = case(cid)
    o = Oracle(**oracle_kw(kw))
    o.init_point_charge()
    assert np.count_nonzero(o.get(1)) == 1 and np.count_nonzero(o.get(0)) == 1  # (psi = -f)
    psi0, f0 = dense_start(o, seed)
    assert np.count_nonzero(f0) == f0.size and np.count_nonzero(psi0) == psi0.size
    for a in (psi0, f0):
        for ax in range(a.ndim):
            assert not np.array_equal(a, np.flip(a, axis=ax))
        if a.shape[-1] == a.shape[-2]:
            assert not np.array_equal(a, np.swapaxes(a, -1, -2))
