"""The batched full multigrid start (mgp_batch_fmg) on many small boxes, against the ordinary context's mgp_fmg on one
such box and against plain batched cycles from a zero guess, for B in BATCHES on two shapes:

  3d_64    3D 64^3, fp32, boundary 'face', red/black GS 2+2, trilinear correction, V-cycle, err on
  2d_256   2D 256^2, the same options

f is smooth: member m holds -d pi^2 prod sin(pi x) at the cell centres, times (1 + m / B) (a dense random f shows the
full multigrid start no benefit: README "Full multigrid start").  Per shape, in one process:

  ordinary            wall time of Context.fmg(1, 1) on member 0's f (one call, its host synchronisation included)
  per B:
    fmg_1_1           wall time of BatchContext.fmg(1, 1), member-starts per second, their ratio to the ordinary context's
                      starts per second, the ascent's launches (mgp_batch_fmg_launches), the members' ||r|| / ||f||
                      (min, median, max)
    plain_cycles      the number k of plain mgp_batch_cycles from psi = 0 after which every member is at or below its
                      residual after fmg(1, 1), and the wall time of one cycles(k) call (psi zeroed before the clock).
                      Where they never get there within MAX_CYCLES (reached = false: the residual stalls at the real
                      type's rounding floor above it), k is the first cycle that lowers the largest residual by less
                      than a fifth: the cycles spent until the stall, a lower bound
  p3_level0           (B = PIECE_B) the kernel time of the batched P3 onto level 0 and of k_batch_prolong on level 0, from
                      one rocprofv3 --kernel-trace run of a child process (--trace-probe: fmg(1, 1) TRACE_CALLS times
                      with eager launches, so not the timed process and not its graph replays: `source` says so); the
                      level-0 launches are those of the largest grid; best of the calls (null when rocprofv3 is not
                      there).  From the same trace lds_ascent_us, the one launch of the levels from T down
                      (k_batch_tail<.., true>, at most 256 threads per member), beside tail_cycle_us, one sub-cycle from
                      level T in the cycle's launch (k_batch_tail<.., false>).  A child that does not end cleanly
                      (any non-zero status, a signal, its time limit) ends the traced runs: the shapes after it are
                      not measured, nothing more is started on the GPU

The timed lines are sampled in turn, REPS rounds, best of; the copy figure (mgp_copy_bandwidth) is from the same run.
Each GPU step runs under a time limit of its own.  Prints one JSON line and writes it to --out.

usage: python3 tools/batch_fmg_time.py [--batches 1,8,64,256] [--shapes 3d_64,2d_256] [--reps 3] [--limit 120]
                                       [--out profiles/batch_fmg_time.json]"""
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

MAX_CYCLES, PIECE_B, TRACE_CALLS = 40, 64, 5
CFG = dict(real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", cycle="V", err_mode=1, coarse_bc="face")
SHAPES = {"3d_64": dict(dim=3, n=(64, 64, 64)), "2d_256": dict(dim=2, n=(256, 256, 1))}


class Limit:
    """A time limit for one GPU step: the process is ended (with a traceback) when the step outlives it."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[batch_fmg_time] {self.what} (limit {self.seconds} s)", file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def smooth_f(kw, B):
    """(B, [nz,] ny, nx) float32: -d pi^2 prod sin(pi x) at the cell centres, member m scaled by 1 + m / B."""
    d = kw["dim"]
    axes = [np.sin(np.pi * (np.arange(n) + 0.5) / n) for n in kw["n"][:d]]  # x, y[, z]
    f = axes[0]
    for a in axes[1:]:
        f = np.multiply.outer(a, f)  # x stays the last axis
    f = -d * np.pi ** 2 * f
    scale = 1.0 + np.arange(B) / B
    return (scale.reshape((B,) + (1,) * d) * f).astype(np.float32)


def stats(x):
    return [float(np.min(x)), float(np.median(x)), float(np.max(x))]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def rel_residual(b):
    rn, fn = b.residual_norm()
    return rn / fn


def cycles_to(b, zeros, target):
    """(k, reached, max over members of ||r|| / ||f|| after each cycle): plain cycles from psi = 0 until every member
    is at or below its target; not reached within MAX_CYCLES: k = the first cycle that lowers the largest residual by
    less than a fifth."""
    b.set_psi(zeros)
    hist = []
    for _ in range(MAX_CYCLES):
        b.cycles(1)
        rel = rel_residual(b)
        hist.append(float(rel.max()))
        if np.all(rel <= target):
            return len(hist), True, hist
    for i in range(1, len(hist)):
        if hist[i] > 0.8 * hist[i - 1]:
            return i + 1, False, hist
    return len(hist), False, hist


def measure(mg, name, batches, reps, limit):
    kw = dict(SHAPES[name], **CFG)
    opts = mg.make_opts(**kw)
    res = {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, "batched": {}}
    with Limit(limit, f"{name}: ordinary context"):
        ctx = mg.Context(opts)
        ctx.set_f(smooth_f(kw, 1)[0])
        ctx.fmg(1, 1)
        rn, fn = ctx.residual_norm()
    res["ordinary"] = {"engines": [lv["engine"] for lv in ctx.levels], "rel_residual": rn / fn, "samples_s": []}
    state = {}
    for B in batches:
        with Limit(limit, f"{name}: batch of {B}, warm-up, residuals and the plain cycles that reach them"):
            b = mg.BatchContext(opts, B)
            b.set_f(smooth_f(kw, B))
            zeros = np.zeros(b.shape(), np.float32)
            b.fmg(1, 1)
            target = rel_residual(b)
            launches = b.fmg_launches()
            k, reached, hist = cycles_to(b, zeros, target)
            b.fmg(1, 1)
        state[B] = (b, zeros, k)
        res["batched"][str(B)] = {
            "engines": [lv["engine"] for lv in b.levels],
            "fmg_1_1": {"ascent_launches": launches, "rel_residual_min_median_max": stats(target), "samples_s": []},
            # (the history up to two cycles past k; what follows a stall is its floor)
            "plain_cycles": {"cycles": k, "reached": reached, "max_rel_residual_per_cycle": hist[:k + 2],
                             "later_cycles_min_median_max": stats(hist[k + 2:]) if hist[k + 2:] else None,
                             "launches_per_cycle": b.launches(), "samples_s": []}}
    for r in range(reps):
        with Limit(limit, f"{name}: Context.fmg(1, 1): sample {r + 1}"):
            ctx.sync()
            res["ordinary"]["samples_s"].append(timed(lambda: ctx.fmg(1, 1)))
        for B in batches:
            b, zeros, k = state[B]
            line = res["batched"][str(B)]
            with Limit(limit, f"{name}: B = {B}, fmg(1, 1): sample {r + 1}"):
                line["fmg_1_1"]["samples_s"].append(timed(lambda: b.fmg(1, 1)))
            if k:
                with Limit(limit, f"{name}: B = {B}, {k} plain cycles: sample {r + 1}"):
                    b.set_psi(zeros)
                    line["plain_cycles"]["samples_s"].append(timed(lambda: b.cycles(k)))
    ctx.close()
    o = res["ordinary"]
    o["ms"] = 1e3 * min(o["samples_s"])
    o["starts_per_s"] = 1e3 / o["ms"]
    for B in batches:
        state[B][0].close()
        line = res["batched"][str(B)]
        a, c = line["fmg_1_1"], line["plain_cycles"]
        a["ms"] = 1e3 * min(a["samples_s"])
        a["member_starts_per_s"] = B * 1e3 / a["ms"]
        a["ratio_to_ordinary"] = a["member_starts_per_s"] / o["starts_per_s"]
        c["ms"] = 1e3 * min(c["samples_s"]) if c["samples_s"] else None
        a["faster_than_plain_cycles"] = None if c["ms"] is None else a["ms"] < c["ms"]
    return res


def trace_probe(mg, name, B):
    """The child of p3_level0: TRACE_CALLS fmg(1, 1) calls of a batch of B (eager launches: MGP_GRAPH=0 is set by the
    parent, so every kernel is a dispatch of its own in the trace)."""
    kw = dict(SHAPES[name], **CFG)
    b = mg.BatchContext(mg.make_opts(**kw), B)
    b.set_f(smooth_f(kw, B))
    for _ in range(TRACE_CALLS):
        b.fmg(1, 1)
    b.close()


def p3_level0(name, B, limit):
    """Kernel microseconds of the batched P3 onto level 0 and of k_batch_prolong on level 0 (best of the traced
    calls), or (None, why); the third value is True when the child did not end cleanly."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return None, "rocprofv3 not found", False
    tmp = tempfile.mkdtemp(prefix="batch_fmg_trace_")
    try:
        cmd = [tool, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--trace-probe", str(B), "--shapes", name]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=dict(os.environ, MGP_GRAPH="0"))
        if r.returncode != 0:
            return None, f"rocprofv3 run ended with status {r.returncode}: {r.stderr[-300:]}", True
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as fh:
                rows += list(csv.DictReader(fh))
    except subprocess.TimeoutExpired:
        return None, "rocprofv3 run outlived its limit", True
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {"source": "rocprofv3 --kernel-trace of a child process, eager launches (MGP_GRAPH=0): kernel times, not the "
                     "timed process and not its graph replays"}
    for key, pat in (("fmg_p3_us", "k_fmg_prolong"), ("batch_prolong_us", "k_batch_prolong")):
        mine = [w for w in rows if pat in w.get("Kernel_Name", "")]
        if not mine:
            return None, f"no {pat} dispatch in the trace", False
        grid = lambda w: int(w.get("Grid_Size") or w.get("Grid_Size_X") or 0)  # noqa: E731
        top = max(grid(w) for w in mine)
        lv0 = [w for w in mine if grid(w) == top]
        out[key] = min(int(w["End_Timestamp"]) - int(w["Start_Timestamp"]) for w in lv0) / 1e3
        out[key.replace("_us", "_kernel")] = lv0[0]["Kernel_Name"][lv0[0]["Kernel_Name"].index(pat):].split("(")[0]
        out[key.replace("_us", "_dispatches")] = len(lv0)
    out["fmg_p3_no_longer_than_batch_prolong"] = out["fmg_p3_us"] <= out["batch_prolong_us"]
    for key, flag in (("lds_ascent_us", "true>"), ("tail_cycle_us", "false>")):
        mine = [w for w in rows if "k_batch_tail<" in w.get("Kernel_Name", "") and flag in w["Kernel_Name"]]
        out[key] = min(int(w["End_Timestamp"]) - int(w["Start_Timestamp"]) for w in mine) / 1e3 if mine else None
        out[key.replace("_us", "_dispatches")] = len(mine)
    return out, None, False


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="1,8,64,256")
    p.add_argument("--shapes", default="3d_64,2d_256")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_fmg_time.json"))
    p.add_argument("--no-trace", action="store_true", help="skip p3_level0, the rocprofv3 run")
    p.add_argument("--trace-probe", type=int, default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    import mgpoisson as mg

    if a.trace_probe is not None:
        with Limit(a.limit, "trace probe"):
            trace_probe(mg, a.shapes.split(",")[0], a.trace_probe)
        return
    batches = [int(x) for x in a.batches.split(",")]
    out = {"tool": "tools/batch_fmg_time.py", "rhs": "-d pi^2 prod sin(pi x) at the cell centres, times 1 + m / B",
           "reps": a.reps, "shapes": {}}
    with Limit(a.limit, "copy bandwidth"):
        out["copy_GBps"] = mg.copy_bandwidth(-1, 2 << 30, 10)
    for name in a.shapes.split(","):
        out["shapes"][name] = measure(mg, name, batches, a.reps, a.limit)
    stopped = None  # a traced child that did not end cleanly: nothing more is started on the GPU
    for name in a.shapes.split(","):  # (after every context of this process is closed)
        if a.no_trace:
            got, why = None, "skipped"
        elif stopped:
            got, why = None, f"not measured: the traced run of {stopped} did not end cleanly"
        else:
            got, why, bad = p3_level0(name, PIECE_B, 2 * a.limit)
            stopped = name if bad else None
        out["shapes"][name]["p3_level0"] = dict(got or {}, batch=PIECE_B, **({"note": why} if why else {}))
    exp = {}
    for name, s in out["shapes"].items():
        bt = s["batched"]
        exp[name] = {
            "a_B64_more_member_starts_than_ordinary": bt["64"]["fmg_1_1"]["ratio_to_ordinary"] > 1.0 if "64" in bt else None,
            "b_launches_do_not_depend_on_B": len({v["fmg_1_1"]["ascent_launches"] for v in bt.values()}) == 1,
            "c_p3_level0_no_longer_than_batch_prolong": s["p3_level0"].get("fmg_p3_no_longer_than_batch_prolong"),
            "d_fmg_faster_than_plain_cycles": {B: v["fmg_1_1"]["faster_than_plain_cycles"] for B, v in bt.items()}}
    out["expectations"] = exp
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
