"""The host model of a context under the box boundaries MGP_BC_FACE / MGP_BC_NEUMANN (test_bc_model.py,
test_gpu_bc.py) — TEST INFRASTRUCTURE ONLY.

abi_model.Model with three things replaced: the level coefficient (cl = +1 / -1 on EVERY level, level 0 included,
where `zero` / `consistent` have 0 there), the coarsest solve (the one-cell level's diagonal (-2 dim - 2 dim cl) / h^2
is 0 under Neumann: the header defines that a cell whose diagonal is 0 is relaxed to +0) and the fp64 defect of an
active refinement (level 0's cl instead of 0).  The arithmetic is oracle_lib's stateless *_arr pieces, which take any
cl.  make_opts takes the boundary as coarse_bc = "face" | "neumann".
"""
from __future__ import annotations

import numpy as np

from abi_model import Model
from oracle_lib import residual_arr

BC_CL = {"face": 1.0, "neumann": -1.0}


def mean_free(a):
    """a minus its mean (fp64 sum), rounded to a's type: what a caller does to f before a Neumann solve."""
    d = a.astype(np.float64)
    return (d - d.sum() / d.size).astype(a.dtype)


class BcModel(Model):
    def __init__(self, world=1, **kw):
        self.bc = kw.pop("coarse_bc")
        assert self.bc in BC_CL, self.bc
        super().__init__(world, **kw)
        self.kw["coarse_bc"] = self.bc

    def cl(self, l):
        return BC_CL[self.bc]

    def _coarse(self, l, h):
        if self.u[l].size == 1 and self.bc == "neumann":  # the singular cell: +0 whatever f holds
            self.u[l] = np.zeros_like(self.u[l])
            return
        super()._coarse(l, h)

    def _smooth(self, l, sweeps, h):
        # (mgp_smooth on the one-cell level relaxes the same singular cell)
        if self.u[l].size == 1 and self.bc == "neumann":
            if sweeps > 0:
                self.u[l] = np.zeros_like(self.u[l])
            return
        super()._smooth(l, sweeps, h)

    def remove_mean(self, l, which, mean):
        """mgp_remove_mean with the mean the device returned: every cell RN((double)x - mean); on level 0 psiOld and
        the metrics are gone."""
        self._writable(l, which)
        a = self.u if which == 0 else self.f
        a[l] = (a[l].astype(np.float64) - mean).astype(self.dtype)
        if l == 0:
            self.psi_old = None

    def refine_remove_mean(self, which, mean):
        self._active()
        if which == 0:
            self.psi64 = self.psi64 - mean
        else:
            self.f64 = self.f64 - mean

    def _defect(self):
        r = residual_arr(self.dim, self.psi64, self.f64, 1.0 / self.n[0], self.cl(0))
        self.f[0] = r.astype(np.float32)
        self.psi_old = None
        return float(np.sqrt((r * r).sum())), float(np.sqrt((self.f64 * self.f64).sum()))
