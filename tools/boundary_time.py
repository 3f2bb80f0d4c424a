"""The box boundaries' cost and convergence: ms per cycle under each coarse_bc value ('zero', 'consistent', 'face',
'neumann') and under 'zero' with MGP_ZS_SPLIT=0 MGP_ZS_SPLIT_POST=0 (level 0 then runs k_zs, the kernel family the
boundary-modified level 0 of 'face' / 'neumann' runs: the stage-split kernels are cl = 0 only), on two shapes:

  3d_512   3D 512^3, fp32, red/black GS 2+2, trilinear P, V-cycle, err on
  2d_4096  2D 4096^2, the same options

All lines of a shape live in one process and are sampled in turn: after WARM untimed cycles each, REPS rounds of one
CYCLES-cycle call per line; the minimum and every sample.  The copy figure (mgp_copy_bandwidth) is from the same run.
Then, per boundary, the number of cycles to ||r|| / ||f|| <= 1e-6 from a dense start (psi and f uniform in [-1, 1),
f's mean removed on the device; at most MAX_CYCLES, with the smallest value reached and its cycle).  Each GPU step runs under a time limit of its own (faulthandler ends the process when
one expires).  Prints one JSON line (last line of the output) and writes it to --out.

usage: python3 tools/boundary_time.py [--shapes 3d_512,2d_4096] [--reps 3] [--limit 120] [--out profiles/boundary_time.json]"""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "lua-multigrid-poisson_amd"))

CYCLES, WARM, RTOL, MAX_CYCLES = 20, 5, 1e-6, 100
CFG = dict(real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", cycle="V", err_mode=1)
SHAPES = {"3d_512": dict(dim=3, n=(512, 512, 512)), "2d_4096": dict(dim=2, n=(4096, 4096, 1))}
NOSPLIT = {"MGP_ZS_SPLIT": "0", "MGP_ZS_SPLIT_POST": "0"}
# line -> (coarse_bc, the environment its context is created under)
LINES = {"zero": ("zero", {}), "consistent": ("consistent", {}), "face": ("face", {}), "neumann": ("neumann", {}),
         "zero_nosplit": ("zero", NOSPLIT)}


class Limit:
    """A time limit for one GPU step: the process is ended (with a traceback) when the step outlives it."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[boundary_time] {self.what} (limit {self.seconds} s)", file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def dense(shape, seed):
    return (2.0 * np.random.default_rng(seed).random(shape, dtype=np.float32) - 1.0).astype(np.float32)


def start(mg, ctx, psi0, f0):
    ctx.set_psi(psi0)
    ctx.set_f(f0)
    return ctx.remove_mean(0, mg.FIELD_F)


def measure(mg, name, reps, limit):
    kw = dict(SHAPES[name], **CFG)
    res = {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, "cycles_per_sample": CYCLES,
           "warm_cycles": WARM, "lines": {}, "cycles_to_rtol": {}, "rtol": RTOL}
    ctxs = {}
    for line, (bc, env) in LINES.items():
        with Limit(limit, f"{name}: context {line}"):
            os.environ.update(env)  # (the tile settings are read when the context is created, and kept in it)
            ctxs[line] = mg.Context(mg.make_opts(coarse_bc=bc, **kw))
            for k in env:
                del os.environ[k]
        res["lines"][line] = {"coarse_bc": bc, "env": env, "engines": [lv["engine"] for lv in ctxs[line].levels],
                              "samples_s": []}
    shape = ctxs["zero"].shape(0)
    psi0, f0 = dense(shape, 1), dense(shape, 2)
    for line, ctx in ctxs.items():
        with Limit(limit, f"{name}: {line}: dense start and warm-up"):
            start(mg, ctx, psi0, f0)
            ctx.cycles(WARM)
    for r in range(reps):
        for line, ctx in ctxs.items():
            with Limit(limit, f"{name}: {line}: sample {r + 1}"):
                ctx.sync()
                t0 = time.perf_counter()
                ctx.cycles(CYCLES)
                res["lines"][line]["samples_s"].append(time.perf_counter() - t0)
    for line, d in res["lines"].items():
        d["ms_per_cycle"] = 1e3 * min(d["samples_s"]) / CYCLES
        with Limit(limit, f"{name}: {line}: the level-0 kernels of one timed cycle"):
            ctx = ctxs[line]
            ctx.timing(True)
            ctx.cycle()
            k = ctx.timing_kernels()
            ctx.timing(False)
        d["level0_kernels"] = {kind: k[kind][0] for kind in ("fused_pre", "fused_post") if kind in k}
    for line in ("zero", "consistent", "face", "neumann"):
        ctx = ctxs[line]
        with Limit(limit, f"{name}: {line}: cycles to {RTOL:g}"):
            start(mg, ctx, psi0, f0)
            hist = []
            for k in range(MAX_CYCLES + 1):
                rn, fn = ctx.residual_norm()
                hist.append(rn / fn)
                if not rn / fn > RTOL:
                    break
                ctx.cycle()
        # (cycles None: not reached within MAX_CYCLES; the smallest value then shows where the run stalled or left)
        res["cycles_to_rtol"][line] = {"cycles": len(hist) - 1 if hist[-1] <= RTOL else None, "min_rel_residual": min(hist),
                                       "cycles_at_min": hist.index(min(hist)), "rel_residual": hist}
    for ctx in ctxs.values():
        ctx.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="3d_512,2d_4096")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_time.json"))
    a = p.parse_args()
    import mgpoisson as mg

    out = {"tool": "tools/boundary_time.py", "rhs": "dense uniform(-1, 1), mean removed", "reps": a.reps, "shapes": {}}
    with Limit(a.limit, "copy bandwidth"):
        out["copy_GBps"] = mg.copy_bandwidth(-1, 2 << 30, 10)
    for name in a.shapes.split(","):
        out["shapes"][name] = measure(mg, name, a.reps, a.limit)
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
