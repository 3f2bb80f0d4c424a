"""The full multigrid start's cost (mgp_fmg) against plain cycles from a zero guess, on two shapes:

  3d_512   3D 512^3, fp32, boundary 'face', red/black GS 2+2, trilinear correction, V-cycle, err on
  2d_4096  2D 4096^2, the same options

f is dense (uniform in [-1, 1)) with its mean removed on the device, as in tools/boundary_time.py.  Per shape, in one
process and one context:

  (a) fmg_1_1, fmg_2_2        wall time of mgp_fmg(1, 1) and mgp_fmg(2, 2) (one call, its host synchronisation included)
                              and ||r|| / ||f|| after each;
  (b) cycles_for_1_1, _2_2    the number of plain mgp_cycles from psi = 0 that reach the same ||r|| / ||f||, and the wall
                              time of one mgp_cycles(k) call (psi zeroed before the clock starts);
  (c) fmg_prolong_0, fmg_restrict_rhs_0, prolong_correct_0
                              the pieces on level 0 alone (PIECE_CALLS calls per sample, each with its synchronisation;
                              time per call), their algorithmic bytes (write 1 + read 1/2^d reals per cell; read 1 +
                              write 1/2^d; mgp_prolong_correct: read 1 + write 1 + read 1/2^d) and the fraction of the
                              copy figure they reach;
  (d) launches                kernel dispatches of one mgp_fmg(1, 1): the difference of two rocprofv3 --kernel-trace
                              runs of a child process (--launch-probe) with and without the call (null when rocprofv3 is
                              not there).

The timed lines are sampled in turn, REPS rounds, best of; the copy figure (mgp_copy_bandwidth) is from the same run.
Each GPU step runs under a time limit of its own.  Prints one JSON line and writes it to --out.

usage: python3 tools/fmg_time.py [--shapes 3d_512,2d_4096] [--reps 3] [--limit 120] [--out profiles/fmg_time.json]"""
import argparse
import csv
import faulthandler
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "lua-multigrid-poisson_amd"))

MAX_CYCLES, PIECE_CALLS = 40, 10
CFG = dict(real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", cycle="V", err_mode=1, coarse_bc="face")
SHAPES = {"3d_512": dict(dim=3, n=(512, 512, 512)), "2d_4096": dict(dim=2, n=(4096, 4096, 1))}


class Limit:
    """A time limit for one GPU step: the process is ended (with a traceback) when the step outlives it."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[fmg_time] {self.what} (limit {self.seconds} s)", file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def dense(shape, seed):
    return (2.0 * np.random.default_rng(seed).random(shape, dtype=np.float32) - 1.0).astype(np.float32)


def setup(mg, name):
    kw = dict(SHAPES[name], **CFG)
    ctx = mg.Context(mg.make_opts(**kw))
    ctx.set_f(dense(ctx.shape(0), 2))
    ctx.remove_mean(0, mg.FIELD_F)
    return kw, ctx


def rel_residual(ctx):
    rn, fn = ctx.residual_norm()
    return rn / fn


def cycles_to(ctx, zeros, target):
    """(k, ||r||/||f|| after each cycle): plain cycles from psi = 0 until the target is reached (k None: not within
    MAX_CYCLES)."""
    ctx.set_psi(zeros)
    hist = []
    for _ in range(MAX_CYCLES):
        ctx.cycle()
        hist.append(rel_residual(ctx))
        if hist[-1] <= target:
            return len(hist), hist
    return None, hist


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def measure(mg, name, reps, limit, copy_gbps):
    with Limit(limit, f"{name}: context and f"):
        kw, ctx = setup(mg, name)
    cells = int(np.prod(ctx.shape(0)))
    zeros = np.zeros(ctx.shape(0), np.float32)
    res = {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()},
           "engines": [lv["engine"] for lv in ctx.levels], "lines": {}}
    lines = res["lines"]
    with Limit(limit, f"{name}: warm-up and the residuals the starts reach"):
        for c, f in ((1, 1), (2, 2)):
            ctx.fmg(c, f)
            lines[f"fmg_{c}_{f}"] = {"rel_residual": rel_residual(ctx), "samples_s": []}
    for c in (1, 2):
        with Limit(limit, f"{name}: plain cycles to the residual of fmg({c}, {c})"):
            k, hist = cycles_to(ctx, zeros, lines[f"fmg_{c}_{c}"]["rel_residual"])
        lines[f"cycles_for_{c}_{c}"] = {"cycles": k, "rel_residual_per_cycle": hist, "samples_s": []}
    pieces = {"fmg_prolong_0": lambda: ctx.fmg_prolong(0), "fmg_restrict_rhs_0": lambda: ctx.fmg_restrict_rhs(0),
              "prolong_correct_0": lambda: ctx.prolong_correct(0)}
    frac = 1.0 / 2 ** kw["dim"]
    reals = {"fmg_prolong_0": 1 + frac, "fmg_restrict_rhs_0": 1 + frac, "prolong_correct_0": 2 + frac}
    for p in pieces:
        lines[p] = {"algorithmic_bytes": reals[p] * cells * 4, "calls_per_sample": PIECE_CALLS, "samples_s": []}
        with Limit(limit, f"{name}: {p}: warm-up"):
            pieces[p]()
    for r in range(reps):
        for c in (1, 2):
            with Limit(limit, f"{name}: fmg({c}, {c}): sample {r + 1}"):
                ctx.sync()
                lines[f"fmg_{c}_{c}"]["samples_s"].append(timed(lambda: ctx.fmg(c, c)))
            k = lines[f"cycles_for_{c}_{c}"]["cycles"]
            if k is not None:
                with Limit(limit, f"{name}: {k} plain cycles: sample {r + 1}"):
                    ctx.set_psi(zeros)
                    ctx.sync()
                    lines[f"cycles_for_{c}_{c}"]["samples_s"].append(timed(lambda: ctx.cycles(k)))
        for p, fn in pieces.items():
            with Limit(limit, f"{name}: {p}: sample {r + 1}"):
                ctx.sync()
                lines[p]["samples_s"].append(timed(lambda: [fn() for _ in range(PIECE_CALLS)]))
    for c in (1, 2):
        a, b = lines[f"fmg_{c}_{c}"], lines[f"cycles_for_{c}_{c}"]
        a["ms"] = 1e3 * min(a["samples_s"])
        b["ms"] = 1e3 * min(b["samples_s"]) if b["samples_s"] else None
        a["faster_than_plain_cycles"] = None if b["ms"] is None else a["ms"] < b["ms"]
    for p in pieces:
        d = lines[p]
        d["ms"] = 1e3 * min(d["samples_s"]) / PIECE_CALLS
        d["GBps"] = d["algorithmic_bytes"] / (d["ms"] * 1e6)
        d["fraction_of_copy"] = d["GBps"] / copy_gbps
    lines["fmg_prolong_0"]["no_longer_than_prolong_correct_0"] = (lines["fmg_prolong_0"]["ms"] <=
                                                                  lines["prolong_correct_0"]["ms"])
    ctx.close()
    return res


def launch_probe(mg, name, with_fmg):
    """The child of count_launches: the set-up, and with_fmg one mgp_fmg(1, 1)."""
    _, ctx = setup(mg, name)
    if with_fmg:
        ctx.fmg(1, 1)
    ctx.sync()
    ctx.close()


def count_launches(name, limit):
    """Kernel dispatches of one mgp_fmg(1, 1), or (None, why)."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return None, "rocprofv3 not found"
    counts = []
    for with_fmg in (0, 1):
        tmp = tempfile.mkdtemp(prefix="fmg_launches_")
        try:
            cmd = [tool, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                   os.path.abspath(__file__), "--launch-probe", str(with_fmg), "--shapes", name]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            if r.returncode != 0:
                return None, f"rocprofv3 run failed ({r.returncode}): {r.stderr[-300:]}"
            files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
            if not files:
                return None, "no kernel trace written"
            n = 0
            for path in files:
                with open(path, newline="") as fh:
                    n += sum(1 for _ in csv.DictReader(fh))
            counts.append(n)
        except subprocess.TimeoutExpired:
            return None, "rocprofv3 run outlived its limit"
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return counts[1] - counts[0], None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="3d_512,2d_4096")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmg_time.json"))
    p.add_argument("--no-launches", action="store_true", help="skip (d), the rocprofv3 runs")
    p.add_argument("--launch-probe", type=int, default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    import mgpoisson as mg

    if a.launch_probe is not None:
        with Limit(a.limit, "launch probe"):
            launch_probe(mg, a.shapes.split(",")[0], bool(a.launch_probe))
        return
    out = {"tool": "tools/fmg_time.py", "rhs": "dense uniform(-1, 1), mean removed", "reps": a.reps, "shapes": {}}
    with Limit(a.limit, "copy bandwidth"):
        out["copy_GBps"] = mg.copy_bandwidth(-1, 2 << 30, 10)
    for name in a.shapes.split(","):
        out["shapes"][name] = measure(mg, name, a.reps, a.limit, out["copy_GBps"])
    for name in a.shapes.split(","):  # (after every context of this process is closed)
        n, why = (None, "skipped") if a.no_launches else count_launches(name, 2 * a.limit)
        out["shapes"][name]["launches_per_fmg_1_1"] = n
        if why:
            out["shapes"][name]["launches_note"] = why
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
