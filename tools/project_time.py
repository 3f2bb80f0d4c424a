"""The cost of the MAC-grid projection passes (mgp_divergence, mgp_gradient, mgp_project) from device memory:

  fp32, red/black GS 2+2, trilinear correction, V-cycle, err on; boundaries 'face' and 'neumann';
  3d_512 (512^3) and 2d_4096 (4096^2).

Per shape and boundary, in one process and one context, the face arrays PyTorch tensors on the device (uniform in
[-1, 1), zero wall faces under Neumann):

  divergence, gradient_subtract   time per call (PIECE_CALLS calls per sample, each with its host synchronisation), the
                                  algorithmic bytes (3D: 4 / 7 reals per cell, 2D: 3 / 5), GB/s and the share of the
                                  copy figure;
  set_field_dev, get_field_dev    mgp_set_field / mgp_get_field of f / psi from device memory, the same way (2 reals per
                                  cell): the pack and unpack passes a caller had to use before;
  project_1_1, project_0_2        wall time of one mgp_project(1, 1) / mgp_project(0, 2) call with norms, and the
                                  divergence norms it returns.

Expectations fixed before the first measurement, reported as met or missed:
  (a) mgp_divergence moves its algorithmic bytes at least as fast as mgp_set_field moves its own in the same run;
  (b) mgp_gradient(SUBTRACT) does the same against mgp_get_field.

The timed lines are sampled in turn, REPS rounds, best of; the copy figure (mgp_copy_bandwidth) is from the same run.
Each GPU step runs under a time limit of its own.  Prints one JSON line and writes it to --out.

usage: python3 tools/project_time.py [--shapes 3d_512,2d_4096] [--bcs face,neumann] [--reps 3] [--limit 120]
                                     [--out profiles/project_time.json]"""
import argparse
import faulthandler
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "lua-multigrid-poisson_amd"))

PIECE_CALLS = 10
CFG = dict(real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", cycle="V", err_mode=1)
SHAPES = {"3d_512": dict(dim=3, n=(512, 512, 512)), "2d_4096": dict(dim=2, n=(4096, 4096, 1))}
REALS = {3: dict(divergence=4, gradient_subtract=7), 2: dict(divergence=3, gradient_subtract=5)}


class Limit:
    """A time limit for one GPU step: the process is ended (with a traceback) when the step outlives it."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[project_time] {self.what} (limit {self.seconds} s)", file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def faces(torch, ctx, bc, seed):
    """The face arrays on the device: uniform in [-1, 1), the wall faces zero under Neumann."""
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    v = [2.0 * torch.rand(s, generator=gen, device="cuda:0", dtype=torch.float32) - 1.0 for s in ctx.face_shapes()]
    if bc == "neumann":
        v[0][:, :, 0] = 0
        v[0][:, :, -1] = 0
        v[1][:, 0, :] = 0
        v[1][:, -1, :] = 0
        if len(v) == 3:
            v[2][0] = 0
            v[2][-1] = 0
    torch.cuda.synchronize()
    return v


def measure(mg, torch, name, bc, reps, limit, copy_gbps):
    L = mg._lib
    kw = dict(SHAPES[name], coarse_bc=bc, **CFG)
    with Limit(limit, f"{name} {bc}: context and fields"):
        ctx = mg.Context(mg.make_opts(**kw))
        v = faces(torch, ctx, bc, 3)
        v0 = [t.clone() for t in v]
        lex = torch.empty(ctx.shape(0), device="cuda:0", dtype=torch.float32)
        torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in v] + [None] * (3 - len(v))
    cells = ctx.count(0)
    dim = kw["dim"]

    def restore():
        for t, t0 in zip(v, v0):
            t.copy_(t0)
        torch.cuda.synchronize()

    def set_dev():
        ctx._chk(L.lib.mgp_set_field(ctx._h, 0, L.FIELD_F, lex.data_ptr(), cells, L.MEM_DEVICE))

    def get_dev():
        ctx._chk(L.lib.mgp_get_field(ctx._h, 0, L.FIELD_U, lex.data_ptr(), cells, L.MEM_DEVICE))

    pieces = {"divergence": lambda: ctx.divergence_ptr(*ptrs),
              "gradient_subtract": lambda: ctx.gradient_ptr(*ptrs, subtract=True),
              "set_field_dev": set_dev, "get_field_dev": get_dev}
    reals = dict(REALS[dim], set_field_dev=2, get_field_dev=2)
    res = {"config": {k: (list(x) if isinstance(x, tuple) else x) for k, x in kw.items()},
           "engines": [lv["engine"] for lv in ctx.levels], "lines": {}}
    lines = res["lines"]
    with Limit(limit, f"{name} {bc}: warm-up"):
        for key, (f, c) in (("project_1_1", (1, 1)), ("project_0_2", (0, 2))):
            restore()
            before, after = ctx.project_ptr(*ptrs, fmg=f, cycles=c)
            lines[key] = {"div_before": before, "div_after": after, "samples_s": []}
        get_dev()  # (lex = psi: a finite field for mgp_set_field)
        for p in pieces:
            lines[p] = {"algorithmic_bytes": reals[p] * cells * 4, "calls_per_sample": PIECE_CALLS, "samples_s": []}
            pieces[p]()
    for r in range(reps):
        for key, (f, c) in (("project_1_1", (1, 1)), ("project_0_2", (0, 2))):
            with Limit(limit, f"{name} {bc}: {key}: sample {r + 1}"):
                restore()
                ctx.sync()
                lines[key]["samples_s"].append(timed(lambda: ctx.project_ptr(*ptrs, fmg=f, cycles=c)))
        for p, fn in pieces.items():
            with Limit(limit, f"{name} {bc}: {p}: sample {r + 1}"):
                ctx.sync()
                lines[p]["samples_s"].append(timed(lambda: [fn() for _ in range(PIECE_CALLS)]))
    for key in ("project_1_1", "project_0_2"):
        lines[key]["ms"] = 1e3 * min(lines[key]["samples_s"])
    for p in pieces:
        d = lines[p]
        d["ms"] = 1e3 * min(d["samples_s"]) / PIECE_CALLS
        d["GBps"] = d["algorithmic_bytes"] / (d["ms"] * 1e6)
        d["fraction_of_copy"] = d["GBps"] / copy_gbps
    res["expectation_a_divergence_at_least_set_field"] = lines["divergence"]["GBps"] >= lines["set_field_dev"]["GBps"]
    res["expectation_b_gradient_at_least_get_field"] = lines["gradient_subtract"]["GBps"] >= lines["get_field_dev"]["GBps"]
    ctx.close()
    del v, v0, lex
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="3d_512,2d_4096")
    p.add_argument("--bcs", default="face,neumann")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_time.json"))
    a = p.parse_args()
    import mgpoisson as mg
    import torch

    out = {"tool": "tools/project_time.py", "faces": "dense uniform(-1, 1) on the device, zero wall faces under neumann",
           "reps": a.reps, "shapes": {}}
    with Limit(a.limit, "copy bandwidth"):
        out["copy_GBps"] = mg.copy_bandwidth(-1, 2 << 30, 10)
    for name in a.shapes.split(","):
        out["shapes"][name] = {bc: measure(mg, torch, name, bc, a.reps, a.limit, out["copy_GBps"])
                               for bc in a.bcs.split(",")}
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
