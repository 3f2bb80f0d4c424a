"""bench.py's plain run, --full and --dump-outputs, on a 64^3 box (the workload functions called in this process).

* a plain run times exactly --steps cycles after --warmup and carries none of the --full measurements;
* --dump-outputs writes what those cycles returned: err (float64, one per timed cycle) and psi, bit-identical to an
  independent context advanced warmup + steps cycles, and identical from run to run;
* a field above DUMP_SAMPLE values is written as its values at the seeded sample's indices;
* --full adds its fields and writes the same outputs (they are taken before the event-timed pass).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, WARMUP = 64, 3, 2
FULL_ONLY = ("relative_residual", "cpu_baseline", "cpu_baseline_1thread", "roofline", "level0_kernels",
             "finest_smoother_GBps", "fp64_line", "north_star_lines")


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def _run(out, *extra):
    bench = _bench()
    a = bench.parse(["--n", str(N), "--steps", str(STEPS), "--warmup", str(WARMUP), "--copy-probe-mb", "16",
                     "--dump-outputs", str(out), *extra])
    box, strong = bench.workload_box(a, 1)
    cfg = bench.make_cfg(a, box, 0, 1, 0, None)
    line = bench.run_workload(a, cfg, box, strong, 0, 1, 0, None, a.steps, a.warmup, primary=True)
    return line, np.load(os.path.join(out, "err.npy")), np.load(os.path.join(out, "psi.npy"))


def test_sample_indices_are_fixed_and_in_range():
    bench = _bench()
    i = bench.sample_indices(512 ** 3, 1000, bench.DUMP_SEED)
    assert i.dtype == np.int64 and i.shape == (1000,) and i[0] >= 0 and i[-1] < 512 ** 3
    assert np.all(np.diff(i) >= 0) and len(np.unique(i)) > 990
    assert np.array_equal(i, bench.sample_indices(512 ** 3, 1000, bench.DUMP_SEED))
    assert not np.array_equal(i, bench.sample_indices(512 ** 3, 1000, bench.DUMP_SEED + 1))
    big = bench.sample_indices(4096 * 4096 * 512, 1000, bench.DUMP_SEED)  # flat indices past 2^31
    assert big[-1] > 2 ** 31 and big[-1] < 4096 * 4096 * 512
    assert bench.DUMP_SAMPLE * 8 <= 64 << 20 and not bench.parse([]).full and bench.parse(["--full"]).full


@pytest.fixture(scope="module")
def reference():
    """err of the timed cycles and psi after them, from a context of its own (read-only)."""
    import mgpoisson

    bench = _bench()
    a = bench.parse(["--n", str(N)])
    with mgpoisson.Context(mgpoisson.make_opts(**bench.make_cfg(a, (N, N, N), 0, 1, 0, None))) as ctx:
        ctx.init_point_charge()
        ctx.cycles(WARMUP)
        errs = ctx.cycles(STEPS)
        psi = ctx.get_psi()
    errs.setflags(write=False)
    psi.setflags(write=False)
    return errs, psi


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_cycles_returned(tmp_path, reference):
    errs, psi = reference
    line, e, p = _run(tmp_path / "a")
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"])
    assert line["metric"] == "V-cycles/sec + finest-smoother achieved HBM GB/s, 3D Poisson" and line["higher_is_better"]
    assert not [k for k in FULL_ONLY if k in line]
    assert e.dtype == np.float64 and e.shape == (STEPS,) and np.array_equal(e, errs) and line["final_err"] == e[-1]
    assert p.dtype == np.float32 and p.shape == (N ** 3,) and np.array_equal(p, psi.reshape(-1))
    _, e2, p2 = _run(tmp_path / "b")
    assert np.array_equal(e2, e) and np.array_equal(p2, p)


@pytest.mark.gpu
def test_large_field_is_dumped_as_the_seeded_sample(tmp_path, reference, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 5000)
    _, _, p = _run(tmp_path)
    idx = bench.sample_indices(N ** 3, 5000, bench.DUMP_SEED)
    assert p.dtype == np.float32 and np.array_equal(p, reference[1].reshape(-1)[idx])


@pytest.mark.gpu
def test_full_run_adds_its_fields_and_dumps_the_same(tmp_path, reference):
    errs, psi = reference
    line, e, p = _run(tmp_path, "--full", "--cpu-cycles", "1", "--cpu-reps", "1", "--cpu-threads", "2")
    assert line["steps"] == STEPS and line["relative_residual"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline_1thread"]["cores"] == 1
    assert np.array_equal(e, errs) and np.array_equal(p, psi.reshape(-1))
