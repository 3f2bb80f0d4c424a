"""A host model of one mgp_ctx and a generator of random call sequences through the C ABI (test_abi_model.py,
test_gpu_sequences.py) — TEST INFRASTRUCTURE ONLY.

The GPU tests elsewhere set level 0, run a few cycles and compare with the oracle.  What the host layer of the library
does between and across calls (per-level u / t pointers that swap or rotate, where psiOld lives, pending lazy zeros,
ghost-plane flags, the hipGraph cache keyed on the pointer state, the save / restore of mgp_two_grid) is state no
kernel test sees.  Model restates the OBSERVABLE state of a world-1 context, u[l] and f[l] of every level (the header's
"stored, writable state": psi / f on level 0, Vs / Rs below), psiOld and the fp64 fields of an active refinement, with
one method per ABI call, composed from the stateless oracle kernels of oracle_lib.py only (smooth_arr, residual_arr,
restrict_arr, restrict_fw_arr, prolong_correct_arr, err_arr, coarse_coef).  A call the header promises to refuse raises
Refusal(status) and leaves the state as it was.

sequence(cid, seed, length) draws a list of ops (tuples whose repr pastes into a regression test) from
default_rng(seed) alone: nothing a GPU returns feeds back into it.  Model.apply(op) runs one op on the model and
returns its outputs; test_gpu_sequences.py holds the mirror that runs it on a context.
"""
from __future__ import annotations

import numpy as np

from dense_start import FW, LC, RAW, RB
from oracle_lib import (coarse_coef, err_arr, prolong_correct_arr, residual_arr, restrict_arr, restrict_fw_arr,
                        smooth_arr)

ERR_ARG, ERR_STATE = -1, -5  # mgp_status
U, F, RESIDUAL, CORRECTION, PSI_OLD, ERROR = 0, 1, 2, 3, 4, 5  # MGP_FIELD_* (TMP is left out: it is no stored state)
REFINE_PSI, REFINE_F = 0, 1
M64 = (1 << 64) - 1


class Refusal(Exception):
    """The call returns `status` before any launch; the model's state is unchanged."""

    def __init__(self, status, why=""):
        super().__init__(f"status {status}: {why}")
        self.status = status


def dense(shape, dtype, seed):
    """uniform(-1, 1) from default_rng(seed), cast to the real type (dense_start.dense_fields' distribution)."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(dtype)


def _mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def fingerprint(arr, z0=0):
    """test_gpu_large.fingerprint (mgp_field_stats' hash) in uint64 arrays: sum mod 2^64 over cells of
    mix64(bits(x) ^ mix64(global lexicographic index))."""
    a = np.ascontiguousarray(arr)
    bits = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).ravel().astype(np.uint64)
    nplane = a.shape[-1] * a.shape[-2] if a.ndim == 3 else a.size
    with np.errstate(over="ignore"):
        idx = np.arange(a.size, dtype=np.uint64) + np.uint64(z0 * nplane)
        return int(np.sum(_mix64(bits ^ _mix64(idx)), dtype=np.uint64)) & M64


def ref_metrics(psi, old):
    """test_gpu_parity._ref_metrics: gpu.lua:173-200 / test-gpu-obj.lua:216-247 (errorBuf in real, sums fp64)."""
    dt = psi.dtype.type
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where((old != 0) & (old != psi), np.abs(1.0 - (psi / old).astype(np.float64)).astype(psi.dtype), dt(0))
    nz = e != 0
    d = psi.astype(np.float64) - old.astype(np.float64)
    n = int(nz.sum())
    return (float(e[nz].astype(np.float64).sum()) / n if n else float("nan")), n, float(np.sqrt((d * d).sum() / d.size))


def level_shapes(dim, n):
    """plan_levels of one rank's whole box: every axis halves while all active axes have >= 2 cells."""
    nx, ny, nz = n[0], n[1], (n[2] if dim == 3 else 1)
    out = []
    while True:
        out.append((nz, ny, nx) if dim == 3 else (ny, nx))
        if not (nx >= 2 and ny >= 2 and (dim == 2 or nz >= 2)):
            return out
        nx, ny, nz = nx // 2, ny // 2, (nz // 2 if dim == 3 else 1)


class Model:
    """kw: the keywords of mgpoisson.make_opts (world 1).  All levels start at zero, as mgp_create leaves them."""

    def __init__(self, world=1, **kw):
        self.world = world  # > 1: a slab decomposition, whose gathered state is the one domain's (this model)
        d = dict(dim=2, n=(8, 8, 1), real="double", nu1=7, nu2=7, smoother="jacobi", cycle="V", prolong="pc",
                 coarse_init="fresh", coarse_bc="zero", coarse_sweeps=48, err_mode=1, restriction="average", arith="real")
        assert set(kw) <= set(d), set(kw) - set(d)
        d.update(kw)
        self.kw = d
        self.dim, self.n = d["dim"], tuple(d["n"])
        self.dtype = np.dtype(np.float64 if d["real"] == "double" else np.float32)
        self.arith = d["arith"] if d["real"] == "float" else "real"
        self.shapes = level_shapes(self.dim, self.n)
        self.nlev = len(self.shapes)
        self.sizes = [s[-1] for s in self.shapes]  # nx of every level
        self.u = [np.zeros(s, self.dtype) for s in self.shapes]
        self.f = [np.zeros(s, self.dtype) for s in self.shapes]
        self.psi_old = None
        self.psi64 = self.f64 = None  # an active refinement's fields
        self.handoff = None           # (level, the callback's own Vs / Rs below it)
        self.handoff_log = []         # (h, u in, f in, u out) of every hand-off of the last op
        self.cycle_log = []
        self.tail_ok = d["smoother"] != "gs_lex" and self.arith == "real"

    # -- helpers --
    def level_h(self, l):
        return float(2 ** l) / self.n[0]

    def cl(self, l):
        return coarse_coef(self.kw["coarse_bc"], l)

    def refining(self):
        return self.psi64 is not None

    def _level(self, l, below=0):
        if not (isinstance(l, int) and 0 <= l < self.nlev - below):
            raise Refusal(ERR_ARG, f"level {l}")

    def _smooth(self, l, sweeps, h):
        self.u[l] = smooth_arr(self.dim, self.u[l], self.f[l], self.kw["smoother"], sweeps, h, self.cl(l), self.arith)

    def _restrict(self, l, h):
        r = residual_arr(self.dim, self.u[l], self.f[l], h, self.cl(l), self.arith)
        if self.kw["restriction"] == "full_weighting":
            self.f[l + 1] = restrict_fw_arr(self.dim, r, self.cl(l + 1), self.arith)
        else:
            self.f[l + 1] = restrict_arr(self.dim, r, self.arith)

    def _prolong(self, l):
        self.u[l] = prolong_correct_arr(self.dim, self.u[l], self.u[l + 1], self.kw["prolong"], self.cl(l + 1), self.arith)

    def _coarse(self, l, h):
        self._smooth(l, 1 if self.u[l].size == 1 else self.kw["coarse_sweeps"], h)

    def _rec(self, l, h, fcycle):
        """cycle_rec of oracle/mgp_oracle.c (cpu.lua:70-165) on the model's levels."""
        if self.handoff is not None and l == self.handoff[0]:
            return self._handoff(l, h)
        if l == self.nlev - 1:
            return self._coarse(l, h)
        self._smooth(l, self.kw["nu1"], h)
        self._restrict(l, h)
        if self.kw["coarse_init"] == "fresh":
            self.u[l + 1] = np.zeros_like(self.u[l + 1])
        if fcycle:
            self._rec(l + 1, 2 * h, True)
        self._rec(l + 1, 2 * h, False)
        self._prolong(l)
        self._smooth(l, self.kw["nu2"], h)

    def _handoff(self, l, h):
        """The callback of mgp_set_coarse_handoff: twoGrid(h, u, f, size) of a solver of its own (its Vs / Rs below
        the level are the callback's, not the context's: the context's levels below stay as they are)."""
        hand, (_, su, sf) = self.handoff, self.handoff
        u_in, f_in = self.u[l].copy(), self.f[l].copy()
        mine = (self.u[l + 1:], self.f[l + 1:])
        self.u[l + 1:], self.f[l + 1:] = su, sf
        self.handoff = None
        self._rec(l, h, self.kw["cycle"] == "F")
        su[:], sf[:] = self.u[l + 1:], self.f[l + 1:]
        self.u[l + 1:], self.f[l + 1:] = mine
        self.handoff = hand
        self.handoff_log.append((h, u_in, f_in, self.u[l].copy()))

    # -- one method per ABI call --
    def cycles(self, k):
        if not (isinstance(k, int) and k >= 0):
            raise Refusal(ERR_ARG, "k")
        if self.refining():
            raise Refusal(ERR_STATE, "refining")
        errs = []
        self.cycle_log = []  # (psiOld, psi) of every outer iteration of this call
        for _ in range(k):
            old = self.u[0].copy()  # psiOld = psi (cpu.lua:200)
            self._rec(0, 1.0 / self.n[0], self.kw["cycle"] == "F")
            self.cycle_log.append((old, self.u[0]))
            if self.kw["err_mode"]:
                self.psi_old = old
                errs.append(err_arr(self.u[0], old, self.arith))
            else:
                errs.append(float("nan"))
        return errs

    def cycle(self):
        return self.cycles(1)[0]

    def smooth(self, l, sweeps):
        self._level(l)
        if sweeps < 0:
            raise Refusal(ERR_ARG, "sweeps")
        self._smooth(l, sweeps, self.level_h(l))

    def residual_restrict(self, l):
        self._level(l, 1)
        self._restrict(l, self.level_h(l))

    def prolong_correct(self, l):
        self._level(l, 1)
        self._prolong(l)

    def coarse_solve(self):
        self._coarse(self.nlev - 1, self.level_h(self.nlev - 1))

    def two_grid(self, h, u, f, size):
        """cpu-raw.lua:186 on the caller's arrays: that level's own u / f and psiOld are unchanged, the levels below
        are the cycle's scratch.  Returns the new u."""
        if self.refining():
            raise Refusal(ERR_STATE, "refining")
        if self.world > 1:
            raise Refusal(ERR_STATE, "single-GPU contexts only")
        if size not in self.sizes:
            raise Refusal(ERR_ARG, "no level of that size")
        l = self.sizes.index(size)
        su, sf = self.u[l], self.f[l]
        self.u[l], self.f[l] = np.array(u, self.dtype), np.array(f, self.dtype)
        self._rec(l, h, self.kw["cycle"] == "F")
        out = self.u[l]
        self.u[l], self.f[l] = su, sf
        return out

    def _writable(self, l, which):
        self._level(l)
        if which not in (U, F):
            raise Refusal(ERR_ARG, "a read-only view")
        if l == 0 and self.refining():
            raise Refusal(ERR_STATE, "refining")

    def set_field(self, l, which, arr):
        self._level(l)
        if l == 0 and self.refining():
            raise Refusal(ERR_STATE, "refining")
        self._writable(l, which)
        (self.u if which == U else self.f)[l] = np.array(arr, self.dtype).reshape(self.shapes[l])

    def _planes(self, l, z, nz):
        depth = self.shapes[l][0] if self.dim == 3 else 1
        if z < 0 or nz < 0 or z + nz > depth:
            raise Refusal(ERR_ARG, "planes outside the slab")

    def set_planes(self, l, which, z, arr):
        if l == 0 and self.refining():
            raise Refusal(ERR_STATE, "refining")
        self._level(l)
        if which not in (U, F):
            raise Refusal(ERR_ARG, "a read-only view")
        self._planes(l, z, arr.shape[0])
        a = (self.u if which == U else self.f)[l].copy()
        a[z:z + arr.shape[0]] = arr
        (self.u if which == U else self.f)[l] = a

    def view(self, l, which):
        self._level(l)
        if which == U:
            return self.u[l].copy()
        if which == F:
            return self.f[l].copy()
        if which == RESIDUAL:
            return residual_arr(self.dim, self.u[l], self.f[l], self.level_h(l), self.cl(l), self.arith)
        if which == CORRECTION:  # P V onto zeros
            if l + 1 >= self.nlev:
                raise Refusal(ERR_ARG, "the coarsest level has no correction")
            return prolong_correct_arr(self.dim, np.zeros_like(self.u[l]), self.u[l + 1], self.kw["prolong"],
                                       self.cl(l + 1), self.arith)
        if which in (PSI_OLD, ERROR):
            if l != 0 or self.psi_old is None:
                raise Refusal(ERR_STATE, "no psiOld")
            if which == PSI_OLD:
                return self.psi_old.copy()
            if self.arith == "double":  # cpu-raw.lua:96-100: the double difference squared, rounded once
                d = self.u[0].astype(np.float64) - self.psi_old.astype(np.float64)
                return (d * d).astype(self.dtype)
            d = self.u[0] - self.psi_old
            return d * d
        raise Refusal(ERR_ARG, "unknown field")

    def get_field(self, l, which):
        return self.view(l, which)

    def get_planes(self, l, which, z, nz):
        self._level(l)
        if not 0 <= which <= 6:
            raise Refusal(ERR_ARG, "unknown field")
        self._planes(l, z, nz)
        v = self.view(l, which)
        return v[z:z + nz] if self.dim == 3 else v[None][z:z + nz]

    def metrics(self):
        if self.refining():
            raise Refusal(ERR_STATE, "refining")
        if self.psi_old is None:
            raise Refusal(ERR_STATE, "no outer iteration with err_mode 1")
        return ref_metrics(self.u[0], self.psi_old)

    def residual_norm(self, l):
        self._level(l)
        r = self.view(l, RESIDUAL).astype(np.float64)
        f = self.f[l].astype(np.float64)
        return float(np.sqrt((r * r).sum())), float(np.sqrt((f * f).sum()))

    def field_stats(self, l, which):
        self._level(l)
        if which not in (U, F):
            raise Refusal(ERR_ARG, "U or F")
        a = (self.u if which == U else self.f)[l]
        d = a.astype(np.float64)
        return fingerprint(a), float(d.sum()), float((d * d).sum()), float(np.abs(d).max())

    def set_coarse_level(self, size, fits=True):
        """No observable state.  fits: whether the levels from that size fit one workgroup's LDS (the caller's
        knowledge: the generator offers only sizes that certainly do or certainly do not)."""
        if size == 0:
            return
        if size not in self.sizes[1:] or not self.tail_ok or not fits:
            raise Refusal(ERR_ARG, "no such level, or it does not fit the coarse engine")

    def set_coarse_handoff(self, size, on):
        if not on:
            self.handoff = None
            return
        if size not in self.sizes[1:]:
            raise Refusal(ERR_ARG, "no level >= 1 of that size")
        l = self.sizes.index(size)
        self.handoff = (l, [np.zeros_like(a) for a in self.u[l + 1:]], [np.zeros_like(a) for a in self.f[l + 1:]])

    def cg_solve(self, maxiter):
        """Its numerics have tests of their own; here: the solver's own state is unchanged."""
        if self.refining():
            raise Refusal(ERR_STATE, "refining")
        if self.world > 1:
            raise Refusal(ERR_STATE, "single-GPU contexts only")

    # -- mixed-precision refinement (the model of test_gpu_refine.py) --
    def refine_begin(self):
        if self.dtype != np.float32 or self.arith != "real":
            raise Refusal(ERR_ARG, "fp32 MGP_ARITH_REAL contexts only")
        if self.world > 1:
            raise Refusal(ERR_STATE, "one GPU only")
        if self.refining():
            raise Refusal(ERR_STATE, "already active")
        self.psi64, self.f64 = self.u[0].astype(np.float64), self.f[0].astype(np.float64)
        self.psi_old = None

    def _active(self):
        if not self.refining():
            raise Refusal(ERR_STATE, "refinement is not active")

    def refine_end(self):
        self._active()
        self.u[0], self.f[0] = self.psi64.astype(np.float32), self.f64.astype(np.float32)
        self.psi64 = self.f64 = None
        self.psi_old = None

    def refine_set(self, which, arr):
        self._active()
        if which == REFINE_PSI:
            self.psi64 = np.array(arr, np.float64)
        else:
            self.f64 = np.array(arr, np.float64)

    def refine_get(self, which):
        self._active()
        return (self.psi64 if which == REFINE_PSI else self.f64).copy()

    def _defect(self):
        r = residual_arr(self.dim, self.psi64, self.f64, 1.0 / self.n[0])
        self.f[0] = r.astype(np.float32)
        self.psi_old = None
        return float(np.sqrt((r * r).sum())), float(np.sqrt((self.f64 * self.f64).sum()))

    def refine_residual(self):
        self._active()
        return self._defect()

    def refine_step(self, inner):
        self._active()
        if inner < 1:
            raise Refusal(ERR_ARG, "inner >= 1")
        rn, fn = self._defect()
        self.u[0] = np.zeros_like(self.u[0])
        for _ in range(inner):
            self._rec(0, 1.0 / self.n[0], self.kw["cycle"] == "F")
        e = self.u[0].astype(np.float64)
        self.psi64 = self.psi64 + e
        self.psi_old = None
        return rn, fn, float(np.sqrt((e * e).sum() / e.size))

    # -- ops --
    def apply(self, op):
        """Run one op of sequence(); returns its outputs (None where the call has none).  Raises Refusal."""
        name, a = op[0], op[1:]
        self.handoff_log = []
        if name == "cycle":
            return self.cycle()
        if name == "cycles":
            return self.cycles(a[0])
        if name == "set_field":
            l, which, seed = a
            self._level(l)
            return self.set_field(l, which, dense(self.shapes[l], self.dtype, seed))
        if name == "set_planes":
            l, which, z, nz, seed = a
            self._level(l)
            return self.set_planes(l, which, z, dense((nz,) + self.shapes[l][1:], self.dtype, seed))
        if name == "two_grid":
            size, hmode, seed = a
            if size not in self.sizes:
                raise Refusal(ERR_STATE if self.refining() or self.world > 1 else ERR_ARG, "no level of that size")
            shp = self.shapes[self.sizes.index(size)]
            return self.two_grid(self.two_grid_h(size, hmode), dense(shp, self.dtype, seed),
                                 dense(shp, self.dtype, seed + 1), size)
        if name in ("timing", "set_debug", "sync"):
            return None
        if name == "refine_set":
            return self.refine_set(a[0], np.random.default_rng(a[1]).uniform(-1.0, 1.0, self.shapes[0]))
        return getattr(self, name)(*a)

    def two_grid_h(self, size, hmode):
        """"level": the level's own h, on which the engines run; "2/n": twice it, which every engine's h == level_h
        gate turns down, so the cycle runs one launch per piece."""
        return (2.0 if hmode == "2/n" else 1.0) * self.level_h(self.sizes.index(size))

    def stored(self):
        """Every array of the observable state, named."""
        out = [(f"u[{l}]", a) for l, a in enumerate(self.u)] + [(f"f[{l}]", a) for l, a in enumerate(self.f)]
        if self.psi_old is not None:
            out.append(("psi_old", self.psi_old))
        if self.refining():
            out += [("psi64", self.psi64), ("f64", self.f64)]
        return out


# ---- the configurations the GPU file runs: id -> (make_opts keywords, environment, engines asserted) ----
# The environment's thresholds are those of the existing tests of each engine (test_gpu_dense.py,
# test_gpu_zs_split_post.py, test_gpu_switches.py, test_gpu_fw.py).  engines: {level: engine} asserted from ctx.levels.
ZS = dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=32768)
CONFIGS = {
    # 1. k_zs_split PRE + k_zs POST on level 0, k_blk below, the tail
    "zs-64x32x16": (dict(dim=3, n=(64, 32, 16), real="float", **RB, **LC), ZS, {0: "zs", 1: "tail"}),
    # 2. 128 x 64 x 32: k_zs_split_post; two fused levels; zs + zpost with the stage-split PRE
    "zs-128x64x32-splitpost": (dict(dim=3, n=(128, 64, 32), real="float", **RB, **LC),
                               dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536, MGP_ZS_SPLIT_POST_MIN_CELLS=0), {0: "zs"}),
    "zs-128x64x32-two-fused": (dict(dim=3, n=(128, 64, 32), real="float", **RB, **LC),
                               dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=32768, MGP_ZS_SPLIT_POST_MIN_CELLS=0),
                               {0: "zs", 1: "zs"}),
    "zs-128x64x32-zpost": (dict(dim=3, n=(128, 64, 32), real="float", **RB, **LC),
                           dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=1 << 18, MGP_ZPOST_MIN_CELLS=32768),
                           {0: "zs", 1: "zpost"}),
    # 3. F-cycle, warm: warm guesses and revisits take k_zs
    "zs-64x32x64-F-warm": (dict(dim=3, n=(64, 32, 64), real="float", cycle="F", coarse_init="warm", **RB, **LC),
                           dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536), {0: "zs"}),
    # 4. fp64 k_zs, pc / zero
    "zs-f64-64x32x16-pc-zero": (dict(dim=3, n=(64, 32, 16), real="double", prolong="pc", coarse_bc="zero", **RB), ZS,
                                {0: "zs"}),
    # 5. k_ys
    "ys-1024-f32": (dict(dim=2, n=(1024, 1024, 1), real="float", **RB, **LC),
                    dict(MGP_FUSED=1, MGP_YS_MIN_CELLS=65536), {0: "zs"}),
    "ys-1024-f64-F": (dict(dim=2, n=(1024, 1024, 1), real="double", cycle="F", **RB, **LC),
                      dict(MGP_FUSED=1, MGP_YS_MIN_CELLS=65536), {0: "zs"}),
    # 6. the reference configuration: Jacobi 7 + 7, injection, zero; every sweep flips u / t
    "jacobi-256-f64": (dict(dim=2, n=(256, 256, 1), real="double"), {}, {0: "piece"}),
    "jacobi-256-f64-warm": (dict(dim=2, n=(256, 256, 1), real="double", coarse_init="warm"), {}, {0: "piece"}),
    # 7. k_blk2
    # 7. k_blk2: the tail from 16^2, so that 64^2 and 32^2 are tiled and pair up
    "blk2-128-f32": (dict(dim=2, n=(128, 128, 1), real="float", prolong="pc", coarse_bc="zero", **RB),
                     dict(MGP_TAIL_CELLS=512), {0: "piece", 1: "blk", 2: "blk", 3: "tail"}),
    # 8. 1 + 3 pc F on 32^3 fp64.  With 1 + 3 sweeps neither k_blk (at most 2 sweeps per phase) nor k_bres (nu1 >= 2)
    # is selected: the per-piece paths with k_post1; the 2 + 2 box beside it has k_bres on level 0 and k_blk on level 1
    "blk-32-f64-F": (dict(dim=3, n=(32, 32, 32), real="double", smoother="rbgs", nu1=1, nu2=3, prolong="pc",
                          cycle="F"), {}, {0: "piece", 1: "tail"}),
    "blk-bres-64x32x32-f64-F": (dict(dim=3, n=(64, 32, 32), real="double", prolong="pc", cycle="F", **RB), {},
                                {0: "piece", 1: "blk", 2: "tail"}),
    # 9. cpu-raw.lua's float arithmetic: every level per piece, set_coarse_level refused
    "raw-64": (dict(dim=2, n=(64, 64, 1), **RAW), {}, {l: "piece" for l in range(7)}),
    # 10. the full weighting fused into k_zs PRE, k_resfw below
    "fw-zs-64x32x16": (dict(dim=3, n=(64, 32, 16), real="float", **RB, **LC, **FW), ZS, {0: "zs"}),
    # 11. lexicographic Gauss-Seidel
    "gslex-64": (dict(dim=2, n=(64, 64, 1), real="double", smoother="gs_lex", nu1=1, nu2=3, prolong="linear"), {},
                 {l: "piece" for l in range(7)}),
    # 12. err_mode 0: errs are NaN, metrics / PSI_OLD refused
    "noerr-64x32x16": (dict(dim=3, n=(64, 32, 16), real="float", err_mode=0, **RB, **LC), ZS, {0: "zs"}),
    # 13. nu1 = 0: the lazy zero must be a real one
    "nu1-0-32": (dict(dim=3, n=(32, 32, 32), real="float", smoother="rbgs", nu1=0, nu2=2, **LC), {},
                 {0: "piece", 1: "tail"}),
}
SEEDS = (1, 2, 3)
LENGTH = 40
# a dense level-0 reset every RESET_EVERY ops where the reference's own cycles diverge from dense fields (the
# zero-boundary Jacobi configuration: test_abi_model.py holds the stored values to the stated range)
RESET_EVERY = {"jacobi-256-f64": 8, "jacobi-256-f64-warm": 8}

KINDS = ("cycle", "cycles", "set_field", "set_planes", "get_planes", "get_field", "smooth", "residual_restrict",
         "prolong_correct", "coarse_solve", "two_grid", "metrics", "residual_norm", "field_stats", "timing", "set_debug",
         "sync", "set_coarse_level", "set_coarse_handoff", "cg_solve")
REFINE_KINDS = ("refine_begin", "refine_set", "refine_get", "refine_residual", "refine_step", "refine_end")


def sequence(cid, seed, length=LENGTH):
    """`length` ops (a few more when a bracket is open at the end) for CONFIGS[cid] from default_rng(seed)."""
    kw = CONFIGS[cid][0]
    m = Model(**kw)  # for the shapes only
    rng = np.random.default_rng([seed, sorted(CONFIGS).index(cid)])
    nlev, dim = m.nlev, m.dim
    can_refine = m.dtype == np.float32 and m.arith == "real"
    level1_bytes = m.u[1].size * m.dtype.itemsize
    ops = []
    timing_left = debug_left = 0
    ops.append(("set_field", 0, U, int(rng.integers(1, 1 << 30))))
    ops.append(("set_field", 0, F, int(rng.integers(1, 1 << 30))))
    weights = dict(cycle=8, cycles=5, set_field=8, set_planes=4 if dim == 3 else 0, get_planes=3 if dim == 3 else 0,
                   get_field=6, smooth=8, residual_restrict=5, prolong_correct=5, coarse_solve=2, two_grid=7, metrics=4,
                   residual_norm=3, field_stats=3, timing=2, set_debug=2, sync=1, set_coarse_level=3,
                   set_coarse_handoff=2, cg_solve=1, refine=2 if can_refine else 0, refused=2)
    names = list(weights)
    p = np.array([weights[k] for k in names], float)
    p /= p.sum()
    ri = lambda lo, hi: int(rng.integers(lo, hi))  # noqa: E731 - [lo, hi)
    sd = lambda: ri(1, 1 << 30)  # noqa: E731
    reset = RESET_EVERY.get(cid, 0)
    # pieces and field writes walk the levels in turn, each seed starting a third of the way on, so that a config's
    # seeds reach every level with both
    turn = {"piece": (seed - 1) * -(-nlev // len(SEEDS)), "write": (seed - 1) * -(-nlev // len(SEEDS))}

    def nxt(what):
        turn[what] += 1
        return (turn[what] - 1) % nlev

    def one(kind):
        nonlocal timing_left, debug_left
        if kind in ("cycle", "coarse_solve", "metrics", "sync"):
            return [(kind,)]
        if kind == "cycles":
            return [("cycles", int(rng.choice([2, 3, 5])))]
        if kind == "set_field":
            return [("set_field", nxt("write"), ri(0, 2), sd())]
        if kind in ("set_planes", "get_planes"):
            l = nxt("write") if kind == "set_planes" else ri(0, nlev)
            depth = m.shapes[l][0]
            z = ri(0, depth)
            nz = ri(1, depth - z + 1)
            if kind == "set_planes":
                return [("set_planes", l, ri(0, 2), z, nz, sd())]
            return [("get_planes", l, int(rng.choice([U, F, RESIDUAL])), z, nz)]
        if kind == "get_field":
            which = int(rng.choice([U, F, RESIDUAL, CORRECTION, PSI_OLD, ERROR]))
            if not kw.get("err_mode", 1) and ri(0, 4):  # (refused there: once in a while is enough)
                which = int(rng.choice([U, F, RESIDUAL, CORRECTION]))
            l = 0 if which in (PSI_OLD, ERROR) else ri(0, nlev - (which == CORRECTION))
            return [("get_field", l, which)]
        if kind == "smooth":
            return [("smooth", nxt("piece"), ri(1, 4))]
        if kind in ("residual_restrict", "prolong_correct"):
            l = nxt("piece")
            return [(kind, l)] if l < nlev - 1 else [("coarse_solve",)]  # (the coarsest level's piece)
        if kind == "two_grid":
            return [("two_grid", m.sizes[ri(0, nlev)], str(rng.choice(["level", "2/n"])), sd())]
        if kind in ("residual_norm",):
            return [(kind, ri(0, nlev))]
        if kind == "field_stats":
            return [(kind, ri(0, nlev), ri(0, 2))]
        if kind == "timing":
            if timing_left:
                return []
            timing_left = 3  # timing(off) follows at most 3 ops later: the event pool is finite
            return [("timing", 1)]
        if kind == "set_debug":
            if debug_left:
                return []
            debug_left = ri(2, 5)
            return [("set_debug", 1)]
        if kind == "set_coarse_level":
            c = ri(0, 6)
            if not any(op[0] == "set_coarse_level" for op in ops):  # a sequence's first is one that is accepted
                c = 3 if (m.tail_ok and c % 2) else 0
            if c in (0, 4) or (c in (2, 5) and not m.tail_ok):  # (every size is refused without the coarse engine)
                return [("set_coarse_level", 0)]
            if c == 1:  # a size with no level >= 1
                return [("set_coarse_level", int(rng.choice([3, m.sizes[0], 2 * m.sizes[0]])))]
            if c == 2 and level1_bytes > (1 << 18):  # level 1 alone is larger than any LDS: does not fit
                return [("set_coarse_level", m.sizes[1], False)]
            fit = [s for l, s in enumerate(m.sizes) if l >= 1 and m.u[l].size <= 512]  # well inside the default 4096
            return [("set_coarse_level", int(rng.choice(fit)))]
        if kind == "set_coarse_handoff":
            if ri(0, 3) == 0:
                return [("set_coarse_handoff", 0, False)]
            # (levels of at most 32768 cells: the callback's cycle runs on the host)
            ok = [s for l, s in enumerate(m.sizes) if l >= 1 and m.u[l].size <= 32768]
            return [("set_coarse_handoff", int(rng.choice(ok)), True), ("cycle",), ("set_coarse_handoff", 0, False)]
        if kind == "cg_solve":
            return [("cg_solve", ri(1, 6))]
        if kind == "refine":
            body = [("refine_begin",), ("refine_set", ri(0, 2), sd()), ("refine_residual",), ("refine_step", ri(1, 3)),
                    ("refine_get", ri(0, 2))]
            for _ in range(ri(0, 3)):  # two ordinary calls that stay allowed while refining
                body.append([("smooth", ri(1, nlev), 1), ("residual_norm", ri(1, nlev)), ("refine_step", 1)][ri(0, 3)])
            # one of the ordinary calls refused while refining
            body.insert(ri(1, len(body) + 1), [("cycle",), ("cycles", 2), ("set_field", 0, ri(0, 2), sd()), ("metrics",),
                                               ("two_grid", m.sizes[0], "level", sd()), ("cg_solve", 2),
                                               ("set_planes", 0, ri(0, 2), 0, 1, sd()), ("refine_begin",)][ri(0, 8)])
            return body + [("refine_end",)]
        assert kind == "refused", kind
        # refused calls: argument and state checks that return before any launch
        c = ri(0, 8)
        return [[("get_planes", ri(0, nlev), U, 0, (m.shapes[0][0] if dim == 3 else 1) + 1),
                 ("two_grid", 3, "level", sd()),
                 ("set_field", ri(0, nlev), int(rng.choice([RESIDUAL, CORRECTION, PSI_OLD])), sd()),
                 ("set_coarse_level", 3),
                 ("smooth", nlev, 1),
                 ("refine_end",),
                 ("refine_step", 1) if can_refine else ("refine_begin",),
                 ("get_field", nlev - 1, CORRECTION)][c]]

    # the deck: every kind is certain in two of a config's three seeds (so that over the seeds each occurs whatever
    # the weights draw), the rest of the length is drawn by weight; then shuffled
    k0 = seed + sorted(CONFIGS).index(cid)
    deck = [k for i, k in enumerate(names) if weights[k] and (i + k0) % 3 != 0]
    need = -(-nlev // len(SEEDS))  # pieces and writes enough for this seed's share of the levels
    deck += [("smooth", "residual_restrict", "prolong_correct")[(i + k0) % 3] for i in range(need)]
    deck += [("set_field", "set_planes")[(i + k0) % 2 if dim == 3 else 0] for i in range(need)]
    rng.shuffle(deck)
    deck = ["cycle"] + deck  # (an outer iteration first: metrics and psiOld are mostly there to compare)
    last_reset = 0
    while len(ops) < length or deck:
        if reset and len(ops) - last_reset >= reset:
            ops += [("set_field", 0, U, sd()), ("set_field", 0, F, sd())]
            last_reset = len(ops)
        kind = deck.pop(0) if deck else str(rng.choice(names, p=p))
        got = one(kind)
        if kind == "refine" and deck:  # its parts in turn over the brackets of a config
            pass
        for op in got:
            ops.append(op)
            if timing_left and op != ("timing", 1):
                timing_left -= 1
                if timing_left == 0:
                    ops.append(("timing", 0))
            if debug_left and op != ("set_debug", 1):
                debug_left -= 1
                if debug_left == 0:
                    ops.append(("set_debug", 0))
    if timing_left:
        ops.append(("timing", 0))
    if debug_left:
        ops.append(("set_debug", 0))
    return ops


# ---- the deterministic sequences of test_gpu_sequences.py (here so that the CPU guard holds them to the value range) ----

GRAPH_CAP = {"graph-cap-7+7": (7, 7), "graph-cap-2+1": (2, 1)}
for _cid, (_nu1, _nu2) in GRAPH_CAP.items():  # the Jacobi reference configuration, and one whose cycles flip u / t
    EXTRA = globals().setdefault("EXTRA", {})
    EXTRA[_cid] = (dict(CONFIGS["jacobi-256-f64"][0], nu1=_nu1, nu2=_nu2), {}, {0: "piece"})


def graph_cap_ops(cid):
    """Single Jacobi sweeps walking down the levels, each a new buffer-pointer state, with mgp_cycles(3) between
    them: 12 states, past the 8 entries of the hipGraph cache.  Level 0 is set again every fourth step (the
    zero-boundary Jacobi cycles grow from dense fields)."""
    nlev = Model(**EXTRA[cid][0]).nlev
    ops = [("set_field", 0, U, 11), ("set_field", 0, F, 12), ("cycles", 3)]
    for i, l in enumerate(list(range(1, nlev)) + [0, 3, 1]):
        if i % 4 == 3:
            ops += [("set_field", 0, U, 13 + 2 * i), ("set_field", 0, F, 14 + 2 * i)]
        ops += [("smooth", l, 1), ("cycles", 3)]
    return ops


TWO_GRID_CIDS = ("zs-64x32x16", "ys-1024-f32", "ys-1024-f64-F", "jacobi-256-f64", "blk2-128-f32")


def two_grid_ops(cid):
    """cycles(2), then twoGrid at the finest size with both h, each followed by the reads of psiOld's consumers."""
    n0 = CONFIGS[cid][0]["n"][0]
    reads = [("metrics",), ("get_field", 0, PSI_OLD), ("get_field", 0, ERROR)]
    return ([("set_field", 0, U, 21), ("set_field", 0, F, 22), ("cycles", 2), ("two_grid", n0, "level", 23)] + reads +
            [("two_grid", n0, "2/n", 25)] + reads + [("cycle",), ("metrics",)])


# ---- world 2 through the loopback transport ----
# id -> (make_opts keywords, environment): dense_start.CASES' slab boxes; levels 0 and 1 are distributed (32 and 16
# planes per rank), 16^3 and below replicated (gather_cells 4096)
SLAB_WORLD, SLAB_GATHER = 2, 4096
_SLAB = dict(dim=3, n=(64, 64, 64), **RB, **LC)
SLAB_CONFIGS = {
    "slab-zs-64": (dict(real="float", **_SLAB), dict(MGP_FUSED=1, MGP_FUSED_MIN_CELLS=65536)),
    "slab-piece-64-f64": (dict(real="double", **_SLAB), dict(MGP_FUSED=0)),
    "slab-piece-64-f64-no-deep-halo": (dict(real="double", **_SLAB), dict(MGP_FUSED=0, MGP_DEEP_HALO=0)),
}
SLAB_KINDS = ("set_planes", "cycle", "cycles", "smooth", "residual_restrict", "prolong_correct", "coarse_solve",
              "get_planes", "residual_norm", "field_stats", "metrics", "two_grid", "cg_solve", "refine_begin")


def slab_sequence(cid, seed, length=30):
    """Ops every rank of the decomposition executes (plane ranges are GLOBAL: a rank takes its part): writes of U and F
    on distributed and replicated levels, cycles, the four pieces, reads, norms, fingerprints, metrics and the calls
    refused for world > 1.  Writes and pieces between cycles are what the ghost-plane state (ghost_ok, ghost_zero,
    fghost_ok, early_u) has to survive."""
    m = Model(**SLAB_CONFIGS[cid][0])
    rng = np.random.default_rng([seed, 100 + sorted(SLAB_CONFIGS).index(cid)])
    nlev = m.nlev
    ri = lambda lo, hi: int(rng.integers(lo, hi))  # noqa: E731
    sd = lambda: ri(1, 1 << 30)  # noqa: E731
    turn = {"piece": seed - 1, "write": seed}

    def nxt(what):
        turn[what] += 1
        return (turn[what] - 1) % nlev

    def planes(l):
        depth = m.shapes[l][0]
        z = ri(0, depth)
        return z, ri(1, depth - z + 1)

    def one(kind):
        if kind in ("cycle", "coarse_solve", "metrics", "refine_begin"):
            return (kind,)
        if kind == "cycles":
            return ("cycles", int(rng.choice([2, 3])))
        if kind == "set_planes":
            l = nxt("write")
            return ("set_planes", l, ri(0, 2)) + planes(l) + (sd(),)
        if kind == "get_planes":
            l = ri(0, nlev)
            return ("get_planes", l, int(rng.choice([U, F, RESIDUAL]))) + planes(l)
        if kind == "smooth":
            return ("smooth", nxt("piece"), ri(1, 4))
        if kind in ("residual_restrict", "prolong_correct"):
            l = nxt("piece")
            return (kind, l) if l < nlev - 1 else ("coarse_solve",)
        if kind == "residual_norm":
            return (kind, ri(0, nlev))
        if kind == "field_stats":
            return (kind, ri(0, nlev), ri(0, 2))
        if kind == "two_grid":
            return ("two_grid", m.sizes[ri(0, nlev)], "level", sd())
        assert kind == "cg_solve", kind
        return ("cg_solve", 2)

    weights = dict(set_planes=6, cycle=5, cycles=3, smooth=5, residual_restrict=4, prolong_correct=4, coarse_solve=1,
                   get_planes=3, residual_norm=2, field_stats=2, metrics=2, two_grid=0.5, cg_solve=0.5, refine_begin=0.5)
    names = list(weights)
    p = np.array([weights[k] for k in names], float)
    p /= p.sum()
    d0 = m.shapes[0][0]
    ops = [("set_planes", 0, U, 0, d0, sd()), ("set_planes", 0, F, 0, d0, sd()), ("cycle",)]
    deck = [k for i, k in enumerate(names) if (i + seed) % 3 != 0]
    deck += ["smooth", "residual_restrict", "prolong_correct", "set_planes", "set_planes", "set_planes"]
    rng.shuffle(deck)
    while len(ops) < length or deck:
        ops.append(one(deck.pop(0) if deck else str(rng.choice(names, p=p))))
    return ops
