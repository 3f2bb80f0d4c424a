"""CPU: the cubic prolongation P3 of the full multigrid start and the FMG criterion, on the host model (fmg_model.py).

The criterion: after mgp_fmg(cycles=1, final=1) the algebraic error max|u_FMG - u_converged| is at most the
discretisation error max|u_converged - u_exact| ("alg/disc" <= 1).  Settings: fp64, RB-GS 2 + 2, trilinear correction,
2^d average, 48 coarse sweeps, V-cycle.  Problems on the unit box, cell centres x = (i + 1/2) h:
  face        u = prod sin(pi x), f = -d pi^2 u (u = 0 on the faces);
  neumann     f = prod cos(pi x) minus its mean, u = -f / (d pi^2) (means removed before comparing);
  consistent  the face problem's f and u (level 0 holds the ghost cell CENTRE at 0, half a cell outside the face, so
              the discretisation error is that boundary's O(h) against this u).
"""
import math

import numpy as np
import pytest

from fmg_model import FmgModel, fmg_prolong_arr

SETTINGS = dict(real="double", smoother="rbgs", nu1=2, nu2=2, prolong="linear", restriction="average", coarse_sweeps=48,
                cycle="V")


def _poly(c, x):
    return ((c[3] * x + c[2]) * x + c[1]) * x + c[0]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_p3_reproduces_cubics_in_the_interior(dim, dtype):
    m = 12
    rng = np.random.default_rng(5 + dim)
    coef = rng.uniform(-1.0, 1.0, (dim, 4))
    X = (np.arange(m) + 0.5) / m          # coarse centres
    x = (np.arange(2 * m) + 0.5) / (2 * m)  # fine centres
    V = np.ones((m,) * dim)
    want = np.ones((2 * m,) * dim)
    for a in range(dim):  # axis a of the array (the last is x); any assignment of the polynomials will do
        shp = [1] * dim
        shp[a] = -1
        V = V * _poly(coef[a], X).reshape(shp)
        want = want * _poly(coef[a], x).reshape(shp)
    got = fmg_prolong_arr(dim, V.astype(dtype), 0.37)
    assert got.dtype == dtype and got.shape == want.shape
    inner = (slice(4, 2 * m - 4),) * dim  # fine cells whose stencil holds no ghost
    err = np.abs(got[inner].astype(np.float64) - want[inner]).max()
    print(f"dim {dim} {np.dtype(dtype).name}: max interior error {err:.3e}")
    # |p| <= 4 per axis; a few dozen roundings of values of that size
    assert err <= 64 * 4.0 ** dim * np.finfo(dtype).eps


def _extend(A, s):
    """Two ghost layers per side on every axis: s times the mirrored in-box layers, axis by axis."""
    for a in range(A.ndim):
        A = np.moveaxis(A, a, 0)
        m = A.shape[0]
        A = np.concatenate([s * A[[1, 0]], A, s * A[[m - 1, m - 2]]])
        A = np.moveaxis(A, 0, a)
    return A


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("cl", [1.0, -1.0], ids=["odd(c=+1)", "even(c=-1)"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_p3_is_exact_on_odd_and_even_extensions(dim, cl, dtype):
    V = np.random.default_rng(9).uniform(-1.0, 1.0, (6, 4, 8)[:dim] if dim == 3 else (4, 8)).astype(dtype)
    big = fmg_prolong_arr(dim, _extend(V, dtype(-cl)), 0.0)  # (its own ghosts touch only the cells cut away)
    inner = (slice(4, -4),) * dim
    assert fmg_prolong_arr(dim, V, cl).tobytes() == np.ascontiguousarray(big[inner]).tobytes()


def test_p3_one_cell_axes():
    """m = 1: E[-1] = E[1] = mc A[0], E[-2] = E[2] = mc (mc A[0])."""
    a, cl = 0.8125, 0.5
    mc = -cl
    g1 = mc * a
    g2 = mc * g1
    wp, wn, wq, wr = 105 / 128, 35 / 128, -7 / 128, -5 / 128
    child = ((wp * a + wn * g1) + wq * g1) + wr * g2
    got = fmg_prolong_arr(2, np.array([[a]]), cl)
    yc = ((wp * child + wn * (mc * child)) + wq * (mc * child)) + wr * (mc * (mc * child))
    assert got.shape == (2, 2) and (got == yc).all()


def _problem(bc, dim, n):
    h = 1.0 / n
    x = (np.arange(n) + 0.5) * h
    if bc == "neumann":
        g, k = np.cos(np.pi * x), np.pi
    else:
        g, k = np.sin(np.pi * x), np.pi
    u = np.ones((n,) * dim)
    for a in range(dim):
        shp = [1] * dim
        shp[a] = -1
        u = u * g.reshape(shp)
    if bc == "neumann":
        f = u - u.sum() / u.size
        return f, -f / (dim * k * k)
    return -dim * k * k * u, u


def _center(a, bc):
    return a - a.sum() / a.size if bc == "neumann" else a


def _ratio(bc, dim, n, operator="cubic"):
    kw = dict(dim=dim, n=(n, n, n if dim == 3 else 1), coarse_bc=bc, **SETTINGS)
    f, exact = _problem(bc, dim, n)
    m = FmgModel(**kw)
    m.fmg_operator = operator
    m.f[0] = f.copy()
    m.fmg(1, 1)
    c = FmgModel(**kw)
    c.f[0] = f.copy()
    for _ in range(80):
        if c.cycles(1)[0] <= 1e-14 * np.abs(c.u[0]).max():
            break
    conv = _center(c.u[0], bc)
    alg = np.abs(_center(m.u[0], bc) - conv).max()
    disc = np.abs(conv - _center(exact, bc)).max()
    return alg / disc, alg, disc


@pytest.mark.parametrize("bc", ["face", "neumann", "consistent"])
@pytest.mark.parametrize("dim,n", [(2, 32), (2, 64), (3, 16), (3, 32)], ids=["32^2", "64^2", "16^3", "32^3"])
def test_fmg_criterion(bc, dim, n):
    r, alg, disc = _ratio(bc, dim, n)
    print(f"{bc} {n}^{dim}: alg/disc = {r:.4f} (algebraic {alg:.3e}, discretisation {disc:.3e})")
    assert math.isfinite(r) and r <= 1.0


def test_trilinear_in_its_place_misses_the_criterion():
    """Why the cubic operator exists: the cycle's trilinear operator as the FMG prolongation leaves an algebraic
    error above the discretisation error at 3D face 16^3 with one cycle per level."""
    r, alg, disc = _ratio("face", 3, 16, operator="trilinear")
    print(f"face 16^3, trilinear FMG prolongation: alg/disc = {r:.4f}")
    assert r > 1.0
