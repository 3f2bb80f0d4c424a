"""The host model of the full multigrid start (mgp_fmg, mgp_fmg_restrict_rhs, mgp_fmg_prolong) — TEST INFRASTRUCTURE
ONLY (test_fmg_model.py, test_gpu_fmg.py).

fmg_prolong_arr restates the header's definition of the cubic prolongation P3 in NumPy (every operation an array
operation in the real type, so each is rounded once and nothing contracts).  FmgModel adds the three calls to the host
model of a context: abi_model.Model under coarse_bc = "zero" | "consistent", bc_model.BcModel under "face" | "neumann".
The right-hand-side restriction is oracle_lib's restriction of the residual, applied to f itself.
"""
from __future__ import annotations

import numpy as np

from abi_model import ERR_ARG, ERR_STATE, Model, Refusal
from bc_model import BC_CL, BcModel
from oracle_lib import prolong_correct_arr, restrict_arr, restrict_fw_arr


def _axis_p3(A, axis, mc):
    """One pass of P3 along `axis`: the line A[0 .. m) extended by two ghosts per side, each mc times the sample it
    mirrors (one multiplication each; m = 1: the second ghost is mc times the first), then the two children
        2I     = ((wp E[I] + wn E[I-1]) + wq E[I+1]) + wr E[I-2]
        2I + 1 = ((wp E[I] + wn E[I+1]) + wq E[I-1]) + wr E[I+2]."""
    A = np.moveaxis(A, axis, 0)
    m = A.shape[0]
    dt = A.dtype.type
    wp, wn, wq, wr = dt(105.0 / 128.0), dt(35.0 / 128.0), dt(-7.0 / 128.0), dt(-5.0 / 128.0)
    if m == 1:
        g1 = mc * A[0]
        g2 = mc * g1
        E = np.stack([g2, g1, A[0], g1, g2])
    else:
        E = np.concatenate([(mc * A[1])[None], (mc * A[0])[None], A, (mc * A[m - 1])[None], (mc * A[m - 2])[None]])
    assert E.dtype == A.dtype
    c, l1, r1, l2, r2 = E[2:2 + m], E[1:1 + m], E[3:3 + m], E[0:m], E[4:4 + m]
    even = ((wp * c + wn * l1) + wq * r1) + wr * l2
    odd = ((wp * c + wn * r1) + wq * l1) + wr * r2
    out = np.empty((2 * m,) + A.shape[1:], A.dtype)
    out[0::2], out[1::2] = even, odd
    return np.moveaxis(out, 0, axis)


def fmg_prolong_arr(dim, V, cl):
    """P3 V: the fine array of twice V's shape on every active axis; passes in the order x, y, z, each on the result
    of the pass before.  V: (ny, nx) or (nz, ny, nx), x fastest; cl: the coarse level's boundary coefficient."""
    V = np.ascontiguousarray(V)
    assert V.ndim == dim
    mc = -V.dtype.type(cl)
    for axis in range(dim - 1, -1, -1):  # x is the last axis
        V = _axis_p3(V, axis, mc)
    return np.ascontiguousarray(V)


class _Fmg:
    """The three calls on a Model.  fmg_operator = "trilinear" puts the cycle's trilinear operator (onto zeros) in
    P3's place: the composition the CPU test holds the cubic operator against."""

    fmg_operator = "cubic"

    def _fmg_refuses(self, handoff=False):
        if self.arith == "double":
            raise Refusal(ERR_ARG, "MGP_ARITH_DOUBLE")
        if self.world > 1:
            raise Refusal(ERR_STATE, "single-GPU contexts only")
        if self.refining():
            raise Refusal(ERR_STATE, "refining")
        if handoff and self.handoff is not None:
            raise Refusal(ERR_STATE, "a coarse hand-off is set")

    def _fmg_restrict(self, l):
        if self.kw["restriction"] == "full_weighting":
            self.f[l + 1] = restrict_fw_arr(self.dim, self.f[l], self.cl(l + 1))
        else:
            self.f[l + 1] = restrict_arr(self.dim, self.f[l])

    def _fmg_prolong(self, l):
        if self.fmg_operator == "cubic":
            self.u[l] = fmg_prolong_arr(self.dim, self.u[l + 1], self.cl(l + 1))
        else:
            self.u[l] = prolong_correct_arr(self.dim, np.zeros_like(self.u[l]), self.u[l + 1], "linear", self.cl(l + 1))
        if l == 0:
            self.psi_old = None

    def fmg_restrict_rhs(self, l):
        self._level(l, 1)
        self._fmg_refuses()
        self._fmg_restrict(l)

    def fmg_prolong(self, l):
        self._level(l, 1)
        self._fmg_refuses()
        self._fmg_prolong(l)

    def fmg(self, cycles=1, final=1):
        """Returns the errs of the `final` outer iterations."""
        if not (isinstance(cycles, int) and cycles >= 1 and isinstance(final, int) and final >= 0):
            raise Refusal(ERR_ARG, "cycles >= 1, final >= 0")
        self._fmg_refuses(handoff=True)
        last = self.nlev - 1
        for l in range(last):
            self._fmg_restrict(l)
        self.u[last] = np.zeros_like(self.u[last])
        self._coarse(last, self.level_h(last))
        self.psi_old = None
        for l in range(last - 1, -1, -1):
            self._fmg_prolong(l)
            self.u[l + 1] = np.zeros_like(self.u[l + 1])
            if l > 0:
                for _ in range(cycles):
                    self._rec(l, self.level_h(l), self.kw["cycle"] == "F")
        return self.cycles(final)


class _FmgGhost(_Fmg, Model):
    pass


class _FmgBox(_Fmg, BcModel):
    pass


def FmgModel(world=1, **kw):
    """The model of a context with these make_opts keywords (coarse_bc: any of the four boundaries)."""
    return (_FmgBox if kw.get("coarse_bc") in BC_CL else _FmgGhost)(world, **kw)
