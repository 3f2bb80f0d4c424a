"""The cost of the variable-coefficient cycle (mgp_set_coefficients) on two shapes:

  3d_512   3D 512^3, fp32, boundary 'face', red/black GS 2+2, (tri)linear correction, V-cycle, err on
  2d_4096  2D 4096^2, the same options

with the smooth coefficient field of the tests (1 + 4.5 (1 + prod sin(2 pi x + 0.3)), max / min = 10) and a dense
mean-free f.  Per shape, in one process:

  vc_cycle           ms per cycle with the coefficients set (mgp_cycles(CYCLES) per sample);
  cleared_cycle      the same context after mgp_clear_coefficients (its fused engines again);
  piece_cycle        a constant context forced to one launch per piece on every level through the existing switches
                     (MGP_FUSED=0, MGP_BLK=0, mgp_set_coarse_level(0));
  half_vc, half      level 0's half-sweep, k_half_vc and k_half: the library's HIP events around the two launches of a
                     single mgp_smooth(0, 1) call (mgp_timing), time per half-sweep, with the algorithmic bytes (u and
                     f: 1.5 reals per cell; beta: one real per face, 3 (2D: 2) per cell; together 4.5 (3.5)) and the
                     fraction of the copy figure.

The lines are sampled in turn, REPS rounds, best of; the copy figure (mgp_copy_bandwidth) is from the same run.  Two
expectations, set before measuring, are reported as met or missed:
  (a) k_half_vc moves its algorithmic bytes at >= 90 % of the rate k_half reaches on the same level in the same run;
  (b) the cycle with coefficients costs at most 4.5 / 1.5 = 3 (2D: 3.5 / 1.5) times the per-piece constant cycle.
Each GPU step runs under a time limit of its own.  Prints one JSON line and writes it to --out.

usage: python3 tools/vc_time.py [--shapes 3d_512,2d_4096] [--reps 3] [--limit 120] [--out profiles/vc_time.json]"""
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

CYCLES = 5
CFG = dict(real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear", cycle="V", err_mode=1, coarse_bc="face")
SHAPES = {"3d_512": dict(dim=3, n=(512, 512, 512)), "2d_4096": dict(dim=2, n=(4096, 4096, 1))}
PIECE_ENV = {"MGP_FUSED": "0", "MGP_BLK": "0"}


class Limit:
    """A time limit for one GPU step: the process is ended (with a traceback) when the step outlives it."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[vc_time] {self.what} (limit {self.seconds} s)", file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def dense(shape, seed):
    return (2.0 * np.random.default_rng(seed).random(shape, dtype=np.float32) - 1.0).astype(np.float32)


def smooth_beta(shape3, dim, phase=0.3):
    """The tests' smooth field (tests/vc_model.py smooth_beta) at the face centres, one axis at a time in float32."""
    out = []
    for a in range(dim):
        ax = 2 - a
        fs = list(shape3)
        fs[ax] += 1
        p = np.ones(fs, np.float32)
        for d in range(3):
            if dim == 2 and d == 0:
                continue
            x = (np.arange(fs[d]) + (0.0 if d == ax else 0.5)) / shape3[d]
            p *= np.sin(2 * np.pi * x + phase).astype(np.float32).reshape([-1 if q == d else 1 for q in range(3)])
        p += 1.0
        p *= 4.5
        p += 1.0
        out.append(p)
    return out


def context(mg, name, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        ctx = mg.Context(mg.make_opts(**dict(SHAPES[name], **CFG)))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx.set_f(dense(ctx.shape(0), 2))
    ctx.remove_mean(0, mg.FIELD_F)
    return ctx


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def half_ms(ctx):
    """ms per half-sweep of one mgp_smooth(0, 1): the library's event pairs around its two level-0 launches."""
    ctx.timing(True)  # (counters reset; cycles run without it: timing turns graph replay off)
    ctx.smooth(0, 1)
    ms, n, _ = ctx.timing_read()["half_sweep"]
    ctx.timing(False)
    assert n == 2, n
    return ms / 2


def measure(mg, name, reps, limit, copy_gbps):
    dim = SHAPES[name]["dim"]
    with Limit(limit, f"{name}: contexts, f and the coefficients"):
        vc = context(mg, name)
        piece = context(mg, name, PIECE_ENV)
        piece.set_coarse_level(0)
        shape = vc.shape(0)
        shape3 = shape if dim == 3 else (1,) + tuple(shape)
        beta = smooth_beta(shape3, dim)
        fused_engines = [lv["engine"] for lv in vc.levels]
        vc.set_coefficients(*beta)
        vc_engines = [lv["engine"] for lv in vc.levels]
        piece_engines = [lv["engine"] for lv in piece.levels]
        assert set(vc_engines) == {"piece"} and set(piece_engines) == {"piece"}, (vc_engines, piece_engines)
    cells = int(np.prod(shape))
    zeros = np.zeros(shape, np.float32)
    lines = {k: {"samples_s": []} for k in ("vc_cycle", "cleared_cycle", "piece_cycle")}
    halves = {"half_vc": [], "half": []}
    for r in range(-1, reps):  # round -1: warm-up (graph capture, first launches), not kept
        keep = r >= 0
        with Limit(limit, f"{name}: round {r + 1}: cycle with coefficients"):
            vc.cycles(1)  # (mgp_set_coefficients dropped the graphs: capture outside the clock)
            vc.set_psi(zeros)
            vc.sync()
            t = timed(lambda: vc.cycles(CYCLES))
            if keep:
                lines["vc_cycle"]["samples_s"].append(t)
        with Limit(limit, f"{name}: round {r + 1}: k_half_vc"):
            t = half_ms(vc)
            if keep:
                halves["half_vc"].append(t)
        with Limit(limit, f"{name}: round {r + 1}: per-piece constant cycle and k_half"):
            piece.set_psi(zeros)
            piece.sync()
            t = timed(lambda: piece.cycles(CYCLES))
            if keep:
                lines["piece_cycle"]["samples_s"].append(t)
            t = half_ms(piece)
            if keep:
                halves["half"].append(t)
        with Limit(limit, f"{name}: round {r + 1}: cleared context"):
            vc.clear_coefficients()
            assert [lv["engine"] for lv in vc.levels] == fused_engines
            vc.set_psi(zeros)
            vc.cycles(1)  # (its graphs were dropped: capture outside the clock)
            vc.set_psi(zeros)
            vc.sync()
            t = timed(lambda: vc.cycles(CYCLES))
            if keep:
                lines["cleared_cycle"]["samples_s"].append(t)
            vc.set_coefficients(*beta)
    for d in lines.values():
        d["ms_per_cycle"] = 1e3 * min(d["samples_s"]) / CYCLES
    reals = {"half_vc": 4.5 if dim == 3 else 3.5, "half": 1.5}
    for k, s in halves.items():
        ms = min(s)
        by = reals[k] * cells * 4
        lines[k] = {"samples_ms": s, "ms": ms, "algorithmic_bytes": by, "GBps": by / (ms * 1e6),
                    "fraction_of_copy": by / (ms * 1e6) / copy_gbps}
    ratio_a = lines["half_vc"]["GBps"] / lines["half"]["GBps"]
    ratio_b = lines["vc_cycle"]["ms_per_cycle"] / lines["piece_cycle"]["ms_per_cycle"]
    bound_b = (4.5 if dim == 3 else 3.5) / 1.5
    res = {"config": dict(CFG, **{k: list(v) if isinstance(v, tuple) else v for k, v in SHAPES[name].items()}),
           "engines_cleared": fused_engines, "cycles_per_sample": CYCLES, "lines": lines,
           "expectation_a": {"half_vc_rate_over_half_rate": ratio_a, "at_least": 0.9, "met": bool(ratio_a >= 0.9)},
           "expectation_b": {"vc_cycle_over_piece_cycle": ratio_b, "at_most": bound_b, "met": bool(ratio_b <= bound_b)}}
    vc.close()
    piece.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="3d_512,2d_4096")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "vc_time.json"))
    a = p.parse_args()
    import mgpoisson as mg

    out = {"tool": "tools/vc_time.py", "rhs": "dense uniform(-1, 1), mean removed", "beta": "smooth, max / min = 10",
           "reps": a.reps, "shapes": {}}
    with Limit(a.limit, "copy bandwidth"):
        out["copy_GBps"] = mg.copy_bandwidth(-1, 2 << 30, 10)
    for name in a.shapes.split(","):
        out["shapes"][name] = measure(mg, name, a.reps, a.limit, out["copy_GBps"])
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
