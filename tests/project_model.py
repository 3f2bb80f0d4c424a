"""NumPy restatement of the MAC-grid projection operators of include/mgpoisson.h (TEST INFRASTRUCTURE ONLY): the
divergence D of a staggered field and the gradient G of psi with the level-0 ghost rule, every operation rounded in the
arrays' type.  Arrays are (nz, ny, nx)-shaped, x fastest, nz = 1 in 2D: vx (nz, ny, nx+1), vy (nz, ny+1, nx),
vz (nz+1, ny, nx) (None in 2D).
"""
from __future__ import annotations

import numpy as np

C0 = {"zero": 0.0, "consistent": 0.0, "face": 1.0, "neumann": -1.0}  # level 0's boundary coefficient


def face_shapes(shape, dim):
    nz, ny, nx = shape
    out = [(nz, ny, nx + 1), (nz, ny + 1, nx)]
    if dim == 3:
        out.append((nz + 1, ny, nx))
    return out


def divergence(vx, vy, vz, dim):
    """f = (((vx[i+1] - vx[i]) + (vy[j+1] - vy[j])) + (vz[k+1] - vz[k])) ih, ih = nx."""
    dt = vx.dtype
    ih = dt.type(vx.shape[2] - 1)
    s = (vx[:, :, 1:] - vx[:, :, :-1]) + (vy[:, 1:, :] - vy[:, :-1, :])
    if dim == 3:
        s = s + (vz[1:, :, :] - vz[:-1, :, :])
    return (s * ih).astype(dt)


def _axis_gradient(psi, axis, mc, ih):
    lo = np.take(psi, [0], axis=axis)
    hi = np.take(psi, [psi.shape[axis] - 1], axis=axis)
    E = np.concatenate([mc * lo, psi, mc * hi], axis=axis)  # each ghost one multiplication
    n = E.shape[axis]
    return (np.take(E, np.arange(1, n), axis=axis) - np.take(E, np.arange(0, n - 1), axis=axis)) * ih


def gradient(psi, dim, c0):
    """(gx, gy, gz): g(face i) = (E[i] - E[i-1]) ih on the line extended by the ghosts mc psi[0], mc psi[n-1],
    mc = -(T)c0.  gz is None in 2D."""
    dt = psi.dtype
    ih = dt.type(psi.shape[2])
    mc = -dt.type(c0)
    gx = _axis_gradient(psi, 2, mc, ih).astype(dt)
    gy = _axis_gradient(psi, 1, mc, ih).astype(dt)
    gz = _axis_gradient(psi, 0, mc, ih).astype(dt) if dim == 3 else None
    return gx, gy, gz


def subtract(v, g):
    """v - g per axis (None stays None)."""
    return tuple(None if a is None or b is None else (a - b).astype(a.dtype) for a, b in zip(v, g))


def random_faces(rng, shape, dim, dt, scale=1.0):
    out = [(scale * rng.uniform(-1, 1, s)).astype(dt) for s in face_shapes(shape, dim)]
    return tuple(out) + (None,) * (3 - len(out))


def dyadic(rng, shape, dt, lo=-8, hi=9, exp=-2):
    """Small integers times a power of two: sums, differences and products by powers of two are exact."""
    return (rng.integers(lo, hi, shape).astype(np.float64) * 2.0 ** exp).astype(dt)


def dyadic_faces(rng, shape, dim, dt, exp=-2):
    out = [dyadic(rng, s, dt, exp=exp) for s in face_shapes(shape, dim)]
    return tuple(out) + (None,) * (3 - len(out))
