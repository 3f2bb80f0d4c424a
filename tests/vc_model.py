"""NumPy restatement of the variable-coefficient operator of include/mgpoisson.h (mgp_set_coefficients) — TEST
INFRASTRUCTURE ONLY.

A_beta u = div(beta grad u) with face coefficients: the coarse coefficients, the operator's s / S_all / S_wall / dg,
relax and residual, the red/black sweep, the gradient with coefficients, and the host model of a context that has
coefficients set (abi_model.Model / bc_model.BcModel with the smoother and the residual replaced; restriction and
prolongation are the constant cycle's, oracle_lib's pieces).  Every operation is rounded in the arrays' type.
Fields are (nz, ny, nx) arrays ((ny, nx) in 2D); face arrays are always 3D: bx (nz, ny, nx+1), by (nz, ny+1, nx),
bz (nz+1, ny, nx), nz = 1 and bz = None in 2D.
"""
from __future__ import annotations

import numpy as np

import project_model as pm
from abi_model import RESIDUAL, Model, Refusal, ERR_STATE
from bc_model import BC_CL, BcModel
from oracle_lib import restrict_arr


def face_shapes(shape, dim):
    s3 = tuple(shape) if dim == 3 else (1,) + tuple(shape)
    return pm.face_shapes(s3, dim)


def coarsen(B, dim):
    """The next level's faces: the mean of the 2^(d-1) fine faces that tile a coarse face, lower tangential axis first."""
    bx, by, bz = B
    dt = bx.dtype.type
    if dim == 2:
        a = bx[:, :, ::2]
        cx = (a[:, 0::2, :] + a[:, 1::2, :]) * dt(0.5)
        a = by[:, ::2, :]
        cy = (a[:, :, 0::2] + a[:, :, 1::2]) * dt(0.5)
        return cx, cy, None
    a = bx[:, :, ::2]  # tangential (y, z)
    cx = (((a[0::2, 0::2] + a[0::2, 1::2]) + a[1::2, 0::2]) + a[1::2, 1::2]) * dt(0.25)
    a = by[:, ::2, :]  # tangential (x, z)
    cy = (((a[0::2, :, 0::2] + a[0::2, :, 1::2]) + a[1::2, :, 0::2]) + a[1::2, :, 1::2]) * dt(0.25)
    a = bz[::2]  # tangential (x, y)
    cz = (((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + a[:, 1::2, 0::2]) + a[:, 1::2, 1::2]) * dt(0.25)
    return cx, cy, cz


def hierarchy(B, dim, nlev):
    out = [tuple(None if b is None else np.ascontiguousarray(b) for b in B)]
    for _ in range(nlev - 1):
        out.append(coarsen(out[-1], dim))
    return out


def _shift(u, axis, d):
    """The neighbour at offset d along axis; out of the box: +0."""
    z = np.zeros_like(np.take(u, [0], axis=axis))
    n = u.shape[axis]
    if d < 0:
        return np.concatenate([z, np.take(u, np.arange(0, n - 1), axis=axis)], axis=axis)
    return np.concatenate([np.take(u, np.arange(1, n), axis=axis), z], axis=axis)


def _lo_hi(b, axis):
    n = b.shape[axis]
    return np.take(b, np.arange(0, n - 1), axis=axis), np.take(b, np.arange(1, n), axis=axis)


def diag(B, dim, shape3, cl, h):
    """dg = ((-S_all) - c S_wall) / hSq per cell."""
    dt = B[0].dtype.type
    faces = [_lo_hi(B[0], 2), _lo_hi(B[1], 1)] + ([_lo_hi(B[2], 0)] if dim == 3 else [])
    axes = [2, 1, 0][:dim]
    S = W = None
    for (lo, hi), ax in zip(faces, axes):
        idx = np.arange(shape3[ax]).reshape([-1 if a == ax else 1 for a in range(3)])
        wl = np.where(idx == 0, lo, dt(0))
        wh = np.where(idx == shape3[ax] - 1, hi, dt(0))
        if S is None:
            S, W = lo + hi, wl + wh
        else:
            S = S + lo
            S = S + hi
            W = W + wl
            W = W + wh
    hsq = dt(h) * dt(h)
    return ((-S) - dt(cl) * W) / hsq


def stencil(u3, B, dim):
    """s = ((((bxl xl + bxr xr) + byl yl) + byr yr) + bzl zl) + bzr zr."""
    (bxl, bxr), (byl, byr) = _lo_hi(B[0], 2), _lo_hi(B[1], 1)
    s = bxl * _shift(u3, 2, -1) + bxr * _shift(u3, 2, 1)
    s = s + byl * _shift(u3, 1, -1)
    s = s + byr * _shift(u3, 1, 1)
    if dim == 3:
        bzl, bzr = _lo_hi(B[2], 0)
        s = s + bzl * _shift(u3, 0, -1)
        s = s + bzr * _shift(u3, 0, 1)
    return s


def _as3(a, dim):
    return a if dim == 3 else a[None]


def residual(u, f, B, dim, h, cl):
    """r = f - (s inv_hSq + dg u)."""
    dt = u.dtype.type
    u3, f3 = _as3(u, dim), _as3(f, dim)
    inv = dt(1) / (dt(h) * dt(h))
    dg = diag(B, dim, u3.shape, cl, h)
    r = f3 - (stencil(u3, B, dim) * inv + dg * u3)
    return r.reshape(u.shape)


def smooth(u, f, B, dim, sweeps, h, cl):
    """`sweeps` red/black Gauss-Seidel sweeps (red = (i + j + k) even first): a = f - s inv_hSq, u = dg == 0 ? +0 : a / dg."""
    dt = u.dtype.type
    u3, f3 = _as3(u, dim).copy(), _as3(f, dim)
    inv = dt(1) / (dt(h) * dt(h))
    dg = diag(B, dim, u3.shape, cl, h)
    k, j, i = np.indices(u3.shape)
    parity = (i + j + k) & 1
    zero = dg == 0
    safe = np.where(zero, dt(1), dg)
    for _ in range(sweeps):
        for colour in (0, 1):
            a = f3 - stencil(u3, B, dim) * inv
            new = np.where(zero, dt(0), a / safe)
            u3 = np.where(parity == colour, new, u3)
    return np.ascontiguousarray(u3.reshape(u.shape))


def gradient(psi, B, dim, c0, v=None):
    """beta_face g (v None: MGP_GRAD_STORE) or v - (beta_face g) per axis; g as project_model.gradient."""
    g = pm.gradient(_as3(psi, dim), dim, c0)
    out = []
    for a in range(3):
        if g[a] is None:
            out.append(None)
            continue
        bg = B[a] * g[a]
        out.append(bg if v is None else v[a] - bg)
    return tuple(out)


def smooth_beta(shape, dim, dt, phase=0.3):
    """A smooth field with max / min = 10 sampled at the face centres: 1 + 4.5 (1 + prod sin(2 pi x + phase))."""
    s3 = tuple(shape) if dim == 3 else (1,) + tuple(shape)
    out = []
    for a, fs in enumerate(pm.face_shapes(s3, dim)):
        ax = 2 - a
        p = np.ones(fs)
        for d in range(3):
            if dim == 2 and d == 0:
                continue
            n = s3[d]
            x = (np.arange(fs[d]) + (0.0 if d == ax else 0.5)) / n
            p = p * np.sin(2 * np.pi * x + phase).reshape([-1 if q == d else 1 for q in range(3)])
        out.append((1.0 + 4.5 * (1.0 + p)).astype(dt))
    return tuple(out) + (None,) * (3 - len(out))


def random_beta(rng, shape, dim, dt, lo=1.0, hi=10.0):
    """Log-uniform in [lo, hi] per face, each axis drawn on its own."""
    s3 = tuple(shape) if dim == 3 else (1,) + tuple(shape)
    out = [np.exp(rng.uniform(np.log(lo), np.log(hi), fs)).astype(dt) for fs in pm.face_shapes(s3, dim)]
    return tuple(out) + (None,) * (3 - len(out))


def ones_beta(shape, dim, dt):
    s3 = tuple(shape) if dim == 3 else (1,) + tuple(shape)
    out = [np.ones(fs, dt) for fs in pm.face_shapes(s3, dim)]
    return tuple(out) + (None,) * (3 - len(out))


class _Vc:
    """The coefficient state and the two pieces that see beta, over a base model."""
    coef = None  # per level (bx, by, bz)

    def set_coefficients(self, bx, by, bz=None):
        if self.refining() or self.handoff is not None:
            raise Refusal(ERR_STATE, "refining / hand-off")
        B = tuple(None if b is None else np.asarray(b, self.dtype).reshape(s)
                  for b, s in zip((bx, by, bz if self.dim == 3 else None), face_shapes(self.shapes[0], self.dim) + [None]))
        self.coef = hierarchy(B, self.dim, self.nlev)

    def clear_coefficients(self):
        self.coef = None

    def _smooth(self, l, sweeps, h):
        if self.coef is None:
            return super()._smooth(l, sweeps, h)
        self.u[l] = smooth(self.u[l], self.f[l], self.coef[l], self.dim, sweeps, h, self.cl(l))

    def _coarse(self, l, h):
        if self.coef is None:
            return super()._coarse(l, h)
        self._smooth(l, 1 if self.u[l].size == 1 else self.kw["coarse_sweeps"], h)

    def _restrict(self, l, h):
        if self.coef is None:
            return super()._restrict(l, h)
        r = residual(self.u[l], self.f[l], self.coef[l], self.dim, h, self.cl(l))
        self.f[l + 1] = restrict_arr(self.dim, r)

    def view(self, l, which):
        if self.coef is None or which != RESIDUAL:
            return super().view(l, which)
        self._level(l)
        return residual(self.u[l], self.f[l], self.coef[l], self.dim, self.level_h(l), self.cl(l))


class VcModel(_Vc, Model):
    pass


class VcBcModel(_Vc, BcModel):
    pass


def make_model(**kw):
    """The model of a context created with these make_opts keywords (coarse_bc any of the four)."""
    return (VcBcModel if kw.get("coarse_bc", "zero") in BC_CL else VcModel)(**kw)
