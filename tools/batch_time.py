"""Many small boxes at once: member-cycles per second of a batch (mgp_batch_*: B members in one hierarchy, every
kernel of a cycle one launch over all members) against the cycles per second of the ordinary context on one such box
(Context.cycles, the path a caller had to loop over before), for B in BATCHES on two shapes:

  2d_256   configs[0], the reference's own configuration: 2D 256^2, fp64, Jacobi 7+7, injection, zero, fresh, V
  3d_64    3D 64^3, fp32, red/black GS 2+2, linear, consistent, V

Per line: CYCLES cycles in one call after WARM untimed ones from the point charge, REPS times; the minimum and
every sample.  A batched line also gives its algorithmic bytes per second (what the launches of one member-cycle
must read and write, see alg_bytes) as a fraction of mgp_copy_bandwidth's figure.  Each GPU step runs under a time
limit of its own (faulthandler ends the process when one expires).  Prints one JSON line (last line of the output).

usage: python3 tools/batch_time.py [--batches 1,8,64,256] [--shapes 2d_256,3d_64] [--reps 3] [--limit 120]"""
import argparse
import faulthandler
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lua-multigrid-poisson_amd"))

CYCLES, WARM = 20, 5
SHAPES = {
    "2d_256": dict(dim=2, n=(256, 256, 1), real="double"),
    "3d_64": dict(dim=3, n=(64, 64, 64), real="float", smoother="rbgs", nu1=2, nu2=2, prolong="linear",
                  coarse_bc="consistent", cycle="V"),
}


class Limit:
    """A time limit for one GPU step: the process is ended (with a traceback) when the step outlives it."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[batch_time] {self.what} (limit {self.seconds} s)", file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def alg_bytes(opts, levels):
    """Algorithmic bytes of one member-cycle (V-cycle): per cell of a per-piece level, a Jacobi sweep reads u and f
    and writes the target (3 reals), a red/black half-sweep moves 1.5 reals (mgp_timing's count), the residual +
    restriction 2 + 2^-d, the prolongation + correction 2 + 2^-d; level 0 adds the psiOld snapshot and the err pass
    (2 reals each); the LDS engine loads its first level's u and f and stores every level's u (and Rs below)."""
    d = opts.dim
    rb = opts.real_bytes
    per_sweep = 3.0  # Jacobi: 3; red/black: two half-sweeps of 1.5
    reals = 0.0
    first_tail = True
    for l, lv in enumerate(levels):
        cells = lv["nx"] * lv["ny"] * lv["nz"]
        if lv["engine"] == "tail":
            reals += cells * (3.0 if first_tail else 2.0)
            first_tail = False
            continue
        reals += cells * ((opts.nu1 + opts.nu2) * per_sweep + 2 * (2.0 + 0.5 ** d))
        if opts.coarse_init == 0 and l > 0:
            reals += cells  # the fresh zero guess
    if opts.err_mode:
        c0 = levels[0]["nx"] * levels[0]["ny"] * levels[0]["nz"]
        reals += 4.0 * c0
    return reals * rb


def time_cycles(ctx, sync, reps, limit, what):
    with Limit(limit, what + ": warm-up"):
        ctx.init_point_charge()
        ctx.cycles(WARM)
    out = []
    for r in range(reps):
        with Limit(limit, f"{what}: sample {r + 1}"):
            sync()
            t0 = time.perf_counter()
            ctx.cycles(CYCLES)
            out.append(time.perf_counter() - t0)
    return out


def measure(mg, name, batches, reps, limit, copy_gbps):
    kw = SHAPES[name]
    opts = mg.make_opts(**kw)
    res = {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, "cycles_per_sample": CYCLES,
           "warm_cycles": WARM}
    with Limit(limit, f"{name}: ordinary context"):
        ctx = mg.Context(opts)
    s = time_cycles(ctx, ctx.sync, reps, limit, f"{name}: Context.cycles({CYCLES})")
    ctx.close()
    base = CYCLES / min(s)
    res["ordinary"] = {"cycles_per_s": base, "ms_per_cycle": 1e3 * min(s) / CYCLES, "samples_s": s}
    res["batched"] = {}
    for B in batches:
        with Limit(limit, f"{name}: batch of {B}"):
            b = mg.BatchContext(opts, B)
        nbytes = alg_bytes(opts, b.levels)
        s = time_cycles(b, lambda: None, reps, limit, f"{name}: B = {B}, cycles({CYCLES})")
        launches = b.launches()
        b.close()
        mcps = B * CYCLES / min(s)
        gbps = mcps * nbytes / 1e9
        res["batched"][str(B)] = {"member_cycles_per_s": mcps, "ms_per_cycle": 1e3 * min(s) / CYCLES, "samples_s": s,
                                  "ratio_to_ordinary": mcps / base, "launches_per_cycle": launches,
                                  "alg_bytes_per_member_cycle": nbytes, "alg_GBps": gbps,
                                  "fraction_of_copy": gbps / copy_gbps}
    if "64" in res["batched"]:
        res["accept_B64_faster_than_ordinary"] = res["batched"]["64"]["ratio_to_ordinary"] > 1.0
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="1,8,64,256")
    p.add_argument("--shapes", default="2d_256,3d_64")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    a = p.parse_args()
    import mgpoisson as mg

    out = {"tool": "tools/batch_time.py", "rhs": "point charge", "reps": a.reps, "shapes": {}}
    with Limit(a.limit, "copy bandwidth"):
        out["copy_GBps"] = mg.copy_bandwidth(-1, 2 << 30, 10)
    for name in a.shapes.split(","):
        out["shapes"][name] = measure(mg, name, [int(x) for x in a.batches.split(",")], a.reps, a.limit, out["copy_GBps"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
