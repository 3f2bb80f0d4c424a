"""Time to a double-precision answer: a real='double' context against mixed-precision defect correction
(mgp_refine_*: fp64 psi / f, fp64 defect and add, fp32 inner cycles), on the point charge with RB-GS 2+2, linear
prolongation and a V-cycle, at 3D 512^3 and 2D 4096^2: bench.py's headline configuration, consistent coarse boundary
included (with the reference's ghost-0 coarse levels this cycle diverges on the point charge at these sizes in every
precision; `--coarse-bc zero` shows it, and "converged" is then false).

Per shape, one context at a time, in this one process:
  double   wall time and cycles until ||f - A psi|| / ||f|| <= RTOL, by mgp_cycles in batches of BATCH cycles
           with mgp_residual_norm after each batch (its host synchronisation included, as the mixed loop's is)
  mixed    the same by mgp_refine_solve(inner, RTOL, epsilon=0) for inner in INNERS
  kernels  launch_defect and launch_refine_add alone from HIP events (mgp_timing's MGP_TIMING_REFINE_* kinds), as
           GB/s of their algorithmic bytes (20 B/cell for the defect without the zero guess, 24 with it, 20 for the
           add) next to mgp_copy_bandwidth's figure
Every measurement runs once untimed first (code objects, graphs, clocks), then REPS times from a fresh point
charge; the minimum and every sample are reported.  Each GPU step runs under a time limit of its own
(faulthandler ends the process when one expires).  Prints one JSON line (last line of the output).

usage: python3 tools/refine_time.py [--shapes 3d,2d] [--n3 512] [--n2 4096] [--reps 3] [--limit 120]
       [--coarse-bc consistent|zero]"""
import argparse
import faulthandler
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lua-multigrid-poisson_amd"))

RTOL = 1e-12
INNERS = (2, 4, 6)
BATCH = 2
MAX_CYCLES = 400
CFG = dict(smoother="rbgs", nu1=2, nu2=2, prolong="linear", cycle="V", coarse_bc="consistent")


class Limit:
    """A time limit for one GPU step: the process is ended (with a traceback) when the step outlives it."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[refine_time] {self.what} (limit {self.seconds} s)", file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def double_to_rtol(ctx):
    """(seconds, cycles, rel) from a fresh point charge."""
    ctx.init_point_charge()
    ctx.sync()
    t0 = time.perf_counter()
    cycles = 0
    rn, fn = ctx.residual_norm(0)
    while rn > RTOL * fn and cycles < MAX_CYCLES:
        ctx.cycles(BATCH)
        cycles += BATCH
        rn, fn = ctx.residual_norm(0)
    return time.perf_counter() - t0, cycles, rn / fn


def mixed_to_rtol(ctx, inner):
    """(seconds, outer steps, rel) from a fresh point charge."""
    ctx.init_point_charge()
    ctx.sync()
    t0 = time.perf_counter()
    steps, rel, _ = ctx.refine_solve(inner=inner, rtol=RTOL, epsilon=0.0, maxouter=MAX_CYCLES // inner)
    return time.perf_counter() - t0, steps, float(rel[-1])


def samples(fn, reps, limit, what):
    with Limit(limit, what + ": warm-up"):
        fn()
    out = []
    for r in range(reps):
        with Limit(limit, f"{what}: sample {r + 1}"):
            out.append(fn())
    return out


def measure(mg, dim, n, reps, limit):
    box = (n, n, n if dim == 3 else 1)
    cells = n ** dim
    res = {"dim": dim, "n": n, "cells": cells}
    with Limit(limit, f"{dim}D {n}: double context"):
        ctx = mg.Context(mg.make_opts(dim=dim, n=box, real="double", **CFG))
    s = samples(lambda: double_to_rtol(ctx), reps, limit, f"{dim}D {n}: double to {RTOL:g}")
    best = min(s)
    res["double"] = {"seconds": best[0], "cycles": best[1], "rel": best[2], "converged": best[2] <= RTOL, "ms_per_cycle": 1e3 * best[0] / max(best[1], 1),
                     "samples_s": [x[0] for x in s], "batch": BATCH}
    ctx.close()
    with Limit(limit, f"{dim}D {n}: mixed context"):
        ctx = mg.Context(mg.make_opts(dim=dim, n=box, real="float", **CFG))
        ctx.refine_begin()
    res["mixed"] = {}
    for inner in INNERS:
        s = samples(lambda: mixed_to_rtol(ctx, inner), reps, limit, f"{dim}D {n}: mixed inner {inner} to {RTOL:g}")
        best = min(s)
        res["mixed"][str(inner)] = {"seconds": best[0], "steps": best[1], "cycles": best[1] * inner, "rel": best[2],
                                    "converged": best[2] <= RTOL,
                                    "samples_s": [x[0] for x in s],
                                    "ratio_mixed_to_double": best[0] / res["double"]["seconds"]}
    # the two fp64 passes alone, from HIP events around each launch
    k = 10
    with Limit(limit, f"{dim}D {n}: kernel timing"):
        ctx.init_point_charge()
        ctx.refine_residual()
        ctx.refine_step(1)
        ctx.timing(True)
        for _ in range(k):
            ctx.refine_residual()
        t = ctx.timing_read()
        ms, launches, nbytes = t["refine_defect"]
        res["defect_no_zero"] = {"us": 1e3 * ms / launches, "bytes_per_cell": nbytes / launches / cells,
                                 "GBps": nbytes / (1e-3 * ms) / 1e9}
        ctx.timing(True)
        for _ in range(k):
            ctx.refine_step(1)
        t = ctx.timing_read()
        for key, name in (("refine_defect", "defect"), ("refine_add", "add")):
            ms, launches, nbytes = t[key]
            res[name] = {"us": 1e3 * ms / launches, "bytes_per_cell": nbytes / launches / cells,
                         "GBps": nbytes / (1e-3 * ms) / 1e9}
        ctx.timing(False)
    ctx.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="3d,2d")
    p.add_argument("--n3", type=int, default=512)
    p.add_argument("--n2", type=int, default=4096)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    p.add_argument("--coarse-bc", default=CFG["coarse_bc"], choices=["consistent", "zero"])
    a = p.parse_args()
    CFG["coarse_bc"] = a.coarse_bc
    import mgpoisson as mg

    out = {"tool": "tools/refine_time.py", "rtol": RTOL, "config": CFG, "rhs": "point charge", "reps": a.reps, "shapes": {}}
    with Limit(a.limit, "copy bandwidth"):
        out["copy_GBps"] = mg.copy_bandwidth(-1, 2 << 30, 10)
    for s in a.shapes.split(","):
        dim, n = (3, a.n3) if s == "3d" else (2, a.n2)
        out["shapes"][f"{dim}d_{n}"] = measure(mg, dim, n, a.reps, a.limit)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
