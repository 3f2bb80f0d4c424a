"""The batched MAC-grid projection (mgp_batch_divergence, mgp_batch_gradient, mgp_batch_project) on many small boxes,
faces in device memory, for B in BATCHES on two shapes:

  3d_64    3D 64^3, fp32, boundary 'face', red/black GS 2+2, trilinear correction, V-cycle, err on
  2d_256   2D 256^2, the same options

The face arrays are PyTorch tensors on the device, uniform in [-1, 1), different per member.  Per shape, in one process:

  ordinary              wall time of one Context.project_ptr(1, 1) call with norms on one such box (its host
                        synchronisation included), and the projections per second from it
  per B:
    project_1_1         wall time of one BatchContext.project_ptr(1, 1) call with norms, the member-projections per
                        second from it and their ratio to the ordinary context's projections per second
    divergence, gradient_subtract
                        time per call (PIECE_CALLS calls per sample, each with its host synchronisation), the algorithmic
                        bytes (3D: 4 / 7 reals per cell, 2D: 3 / 5), GB/s and the share of the copy figure
    set_field_dev, get_field_dev
                        mgp_batch_set_field of f / mgp_batch_get_field of psi from device memory, the same way (2 reals
                        per cell): the pack and unpack passes a caller of a batch had to use before

Expectations fixed before the first measurement, reported as met or missed, at B = 64 on each shape:
  (a) more member-projections per second than the ordinary context gives projections per second;
  (b) mgp_batch_divergence moves its algorithmic bytes at a higher rate than mgp_batch_set_field moves its own;
  (c) mgp_batch_gradient(SUBTRACT) does the same against mgp_batch_get_field.

The timed lines are sampled in turn, REPS rounds, best of; the copy figure (mgp_copy_bandwidth) is from the same run.
Each GPU step runs under a time limit of its own.  Prints one JSON line and writes it to --out.

usage: python3 tools/batch_project_time.py [--batches 1,8,64,256] [--shapes 3d_64,2d_256] [--reps 3] [--limit 120]
                                           [--out profiles/batch_project_time.json]"""
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
CFG = dict(real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", cycle="V", err_mode=1, coarse_bc="face")
SHAPES = {"3d_64": dict(dim=3, n=(64, 64, 64)), "2d_256": dict(dim=2, n=(256, 256, 1))}
REALS = {3: dict(divergence=4, gradient_subtract=7), 2: dict(divergence=3, gradient_subtract=5)}


class Limit:
    """A time limit for one GPU step: the process is ended (with a traceback) when the step outlives it."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[batch_project_time] {self.what} (limit {self.seconds} s)", file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def faces(torch, shapes, seed):
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    v = [2.0 * torch.rand(s, generator=gen, device="cuda:0", dtype=torch.float32) - 1.0 for s in shapes]
    torch.cuda.synchronize()
    return v


class Faces:
    """Device face arrays with a copy to restore them from (the projection and the gradient work in place)."""

    def __init__(self, torch, shapes, seed):
        self.torch = torch
        self.v = faces(torch, shapes, seed)
        self.v0 = [t.clone() for t in self.v]
        self.ptrs = [t.data_ptr() for t in self.v] + [None] * (3 - len(self.v))
        torch.cuda.synchronize()

    def restore(self):
        for t, t0 in zip(self.v, self.v0):
            t.copy_(t0)
        self.torch.cuda.synchronize()


def measure(mg, torch, name, batches, reps, limit, copy_gbps):
    L = mg._lib
    kw = dict(SHAPES[name], **CFG)
    opts = mg.make_opts(**kw)
    dim = kw["dim"]
    res = {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, "batched": {}}
    with Limit(limit, f"{name}: ordinary context, warm-up"):
        ctx = mg.Context(opts)
        cv = Faces(torch, ctx.face_shapes(), 5)
        before, after = ctx.project_ptr(*cv.ptrs, fmg=1, cycles=1)
    res["ordinary"] = {"engines": [lv["engine"] for lv in ctx.levels], "div_before": before, "div_after": after,
                       "samples_s": []}
    state = {}
    for B in batches:
        with Limit(limit, f"{name}: batch of {B}, warm-up"):
            b = mg.BatchContext(opts, B)
            bv = Faces(torch, b.face_shapes(), 7 + B)
            lex = torch.empty(b.shape(), device="cuda:0", dtype=torch.float32)
            cells = lex.numel()
            torch.cuda.synchronize()
            before, after = b.project_ptr(*bv.ptrs, fmg=1, cycles=1)
            pieces = {
                "divergence": lambda b=b, bv=bv: b.divergence_ptr(*bv.ptrs),
                "gradient_subtract": lambda b=b, bv=bv: b.gradient_ptr(*bv.ptrs, subtract=True),
                "set_field_dev": lambda b=b, lex=lex: b.set_field_ptr(L.FIELD_F, lex.data_ptr()),
                "get_field_dev": lambda b=b, lex=lex: b.get_field_ptr(L.FIELD_U, lex.data_ptr()),
            }
            reals = dict(REALS[dim], set_field_dev=2, get_field_dev=2)
            line = {"engines": [lv["engine"] for lv in b.levels],
                    "project_1_1": {"div_before_max": float(before.max()), "div_after_max": float(after.max()),
                                    "samples_s": []}}
            pieces["get_field_dev"]()  # (lex = psi: a finite field for mgp_batch_set_field)
            for p, fn in pieces.items():
                line[p] = {"algorithmic_bytes": reals[p] * cells * 4, "calls_per_sample": PIECE_CALLS, "samples_s": []}
                fn()
        state[B] = (b, bv, lex, pieces)
        res["batched"][str(B)] = line
    for r in range(reps):
        with Limit(limit, f"{name}: Context.project(1, 1): sample {r + 1}"):
            cv.restore()
            ctx.sync()
            res["ordinary"]["samples_s"].append(timed(lambda: ctx.project_ptr(*cv.ptrs, fmg=1, cycles=1)))
        for B in batches:
            b, bv, lex, pieces = state[B]
            line = res["batched"][str(B)]
            with Limit(limit, f"{name}: B = {B}, project(1, 1): sample {r + 1}"):
                bv.restore()
                line["project_1_1"]["samples_s"].append(timed(lambda: b.project_ptr(*bv.ptrs, fmg=1, cycles=1)))
            for p, fn in pieces.items():
                with Limit(limit, f"{name}: B = {B}, {p}: sample {r + 1}"):
                    torch.cuda.synchronize()
                    line[p]["samples_s"].append(timed(lambda: [fn() for _ in range(PIECE_CALLS)]))
    ctx.close()
    o = res["ordinary"]
    o["ms"] = 1e3 * min(o["samples_s"])
    o["projections_per_s"] = 1e3 / o["ms"]
    for B in batches:
        b, bv, lex, pieces = state[B]
        b.close()
        line = res["batched"][str(B)]
        a = line["project_1_1"]
        a["ms"] = 1e3 * min(a["samples_s"])
        a["member_projections_per_s"] = B * 1e3 / a["ms"]
        a["ratio_to_ordinary"] = a["member_projections_per_s"] / o["projections_per_s"]
        for p in pieces:
            d = line[p]
            d["ms"] = 1e3 * min(d["samples_s"]) / PIECE_CALLS
            d["GBps"] = d["algorithmic_bytes"] / (d["ms"] * 1e6)
            d["fraction_of_copy"] = d["GBps"] / copy_gbps
    state.clear()
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="1,8,64,256")
    p.add_argument("--shapes", default="3d_64,2d_256")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_project_time.json"))
    a = p.parse_args()
    import mgpoisson as mg
    import torch

    batches = [int(x) for x in a.batches.split(",")]
    out = {"tool": "tools/batch_project_time.py", "faces": "dense uniform(-1, 1) on the device, different per member",
           "reps": a.reps, "shapes": {}}
    with Limit(a.limit, "copy bandwidth"):
        out["copy_GBps"] = mg.copy_bandwidth(-1, 2 << 30, 10)
    for name in a.shapes.split(","):
        out["shapes"][name] = measure(mg, torch, name, batches, a.reps, a.limit, out["copy_GBps"])
    exp = {}
    for name, s in out["shapes"].items():
        l64 = s["batched"].get("64")
        exp[name] = None if l64 is None else {
            "a_more_member_projections_than_ordinary": l64["project_1_1"]["ratio_to_ordinary"] > 1.0,
            "b_divergence_faster_than_set_field": l64["divergence"]["GBps"] > l64["set_field_dev"]["GBps"],
            "c_gradient_faster_than_get_field": l64["gradient_subtract"]["GBps"] > l64["get_field_dev"]["GBps"]}
    out["expectations_at_B64"] = exp
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
