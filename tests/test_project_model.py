"""CPU: the NumPy restatement of the MAC-grid divergence D and gradient G (project_model.py) against the oracle's
level-0 operator: D(v - G psi) == f - A psi with f = D v.

On fields of small integers times powers of two every operation is exact, so the identity holds bit for bit in fp32
and fp64 for c0 in {0, +1, -1}.  On uniform random fields the two sides differ by rounding only; the bound is
64 eps (n0^2 max|psi| + n0 max|v|), four times the largest ratio observed (15.1) when the definitions were prototyped.
"""
import numpy as np
import pytest

import mgp_oracle_np as onp
import project_model as pm

SHAPES_2D = [(2, 2), (4, 4), (64, 16), (2, 1)]  # (nx, ny)
SHAPES_3D = [(2, 2, 2), (16, 8, 4), (2, 4, 8), (8, 8, 32), (1, 1, 4)]  # (nx, ny, nz)
EXACT = [(2, s) for s in SHAPES_2D] + [(3, s) for s in SHAPES_3D]
RANDOM = [(2, (32, 32)), (2, (64, 4)), (3, (16, 16, 16)), (3, (8, 8, 32))]
DTYPES = [np.float32, np.float64]
C0S = [0.0, 1.0, -1.0]


def _shape(box):
    return (box[2] if len(box) == 3 else 1, box[1], box[0])


def _ids(box):
    return "x".join(map(str, box))


def _both_sides(psi, v, dim, c0):
    h = 1.0 / psi.shape[2]
    f = pm.divergence(*v, dim)
    lhs = pm.divergence(*pm.subtract(v, pm.gradient(psi, dim, c0)), dim)
    rhs = onp.residual(psi, f, h, dim, cl=c0)
    return lhs, rhs


@pytest.mark.parametrize("c0", C0S)
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("dim,box", EXACT, ids=[_ids(b) for _, b in EXACT])
def test_identity_is_exact_on_dyadic_fields(dim, box, dt, c0):
    dt = np.dtype(dt)
    rng = np.random.default_rng(7 + sum(box))
    shape = _shape(box)
    psi = pm.dyadic(rng, shape, dt)
    v = pm.dyadic_faces(rng, shape, dim, dt)
    lhs, rhs = _both_sides(psi, v, dim, c0)
    assert lhs.dtype == rhs.dtype == dt
    assert np.any(rhs != 0)
    assert lhs.tobytes() == rhs.tobytes()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("dim,box", EXACT, ids=[_ids(b) for _, b in EXACT])
def test_neumann_wall_faces_keep_their_bits(dim, box, dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(11 + sum(box))
    shape = _shape(box)
    psi = rng.uniform(-1, 1, shape).astype(dt)
    v = list(pm.random_faces(rng, shape, dim, dt))
    # signed zeros and a subnormal on the walls
    v[0][:, :, 0].flat[0] = dt.type(-0.0)
    v[0][:, :, -1].flat[0] = dt.type(0.0)
    v[1][:, 0, :].flat[0] = dt.type(-0.0)
    v[1][:, -1, :].flat[0] = np.finfo(dt).smallest_subnormal
    if dim == 3:
        v[2][0].flat[0] = dt.type(-0.0)
    g = pm.gradient(psi, dim, -1.0)
    w = pm.subtract(v, g)
    walls = [(0, np.s_[:, :, 0]), (0, np.s_[:, :, -1]), (1, np.s_[:, 0, :]), (1, np.s_[:, -1, :])]
    if dim == 3:
        walls += [(2, np.s_[0]), (2, np.s_[-1])]
    for a, sl in walls:
        assert g[a][sl].tobytes() == np.zeros_like(g[a][sl]).tobytes()  # +0, not -0
        assert w[a][sl].tobytes() == v[a][sl].tobytes()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("dim,box", EXACT, ids=[_ids(b) for _, b in EXACT])
def test_neumann_adjointness_on_integer_fields(dim, box, dt):
    """<D v, psi> = -<v, G psi> with zero wall faces: summation by parts, exact on integers."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(13 + sum(box))
    shape = _shape(box)
    psi = pm.dyadic(rng, shape, dt, exp=0)
    v = pm.dyadic_faces(rng, shape, dim, dt, exp=0)
    v[0][:, :, 0] = v[0][:, :, -1] = 0
    v[1][:, 0, :] = v[1][:, -1, :] = 0
    if dim == 3:
        v[2][0] = v[2][-1] = 0
    g = pm.gradient(psi, dim, -1.0)
    lhs = np.sum(pm.divergence(*v, dim).astype(np.float64) * psi)
    rhs = -sum(np.sum(a.astype(np.float64) * b) for a, b in zip(v, g) if a is not None)
    assert lhs == rhs and np.isfinite(lhs)


@pytest.mark.parametrize("c0", C0S)
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("dim,box", RANDOM, ids=[_ids(b) for _, b in RANDOM])
def test_identity_within_rounding_on_random_fields(dim, box, dt, c0):
    dt = np.dtype(dt)
    rng = np.random.default_rng(17 + sum(box))
    shape = _shape(box)
    psi = rng.uniform(-1, 1, shape).astype(dt)
    v = pm.random_faces(rng, shape, dim, dt)
    lhs, rhs = _both_sides(psi, v, dim, c0)
    n0 = float(box[0])
    vmax = max(np.abs(a).max() for a in v if a is not None)
    bound = 64 * np.finfo(dt).eps * (n0 * n0 * np.abs(psi).max() + n0 * vmax)
    diff = np.abs(lhs.astype(np.float64) - rhs.astype(np.float64)).max()
    print(f"{_ids(box)} {dt} c0={c0}: max diff {diff:.3e} = {diff / (bound / 64):.2f} eps-units, bound {bound:.3e}")
    assert diff <= bound


def test_one_cell_axis_takes_both_ghosts_from_its_cell():
    psi = np.array([[[3.0]]], dtype=np.float32)
    gx, gy, _ = pm.gradient(psi, 2, 1.0)  # face Dirichlet: ghost = -psi, ih = 1
    assert gx.tolist() == [[[6.0, -6.0]]] and gy.tolist() == [[[6.0], [-6.0]]]
    gx, _, _ = pm.gradient(psi, 2, 0.0)
    assert gx.tolist() == [[[3.0, -3.0]]]
