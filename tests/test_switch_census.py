"""CPU: every environment switch the library reads has a test that sets it, or a stated reason why not.

README's switch list promises identical bits for its settings.  A switch that no test sets is a promise nobody checks,
so a new getenv("MGP_...") in lua-multigrid-poisson_amd/csrc cannot land without a line in TESTED (the test that sets
it) or in EXEMPT (why it has none), and every switch that is not exempt is documented in README.md.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lua-multigrid-poisson_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")

_SW = "test_gpu_switches"
# switch -> (test module, test function of that module that runs with it set)
TESTED = {
    "MGP_BLK": ("test_gpu_block", "test_block_phases_match_oracle"),
    "MGP_BLK2": ("test_gpu_blk2", "test_blk2_cycles_match_oracle_and_single_level_launches"),
    "MGP_BLK_CELLS": (_SW, "test_blk_cells_moves_levels_between_k_blk_and_the_pieces"),
    "MGP_BRES": ("test_gpu_bres", "test_bres_cycles_match_oracle_and_pieces"),
    "MGP_BRES_VN": (_SW, "test_bres_cells_per_thread"),
    "MGP_COMM_TIMEOUT_S": ("test_gpu_rccl", "test_comm_deadline_reports_the_stalled_exchange_and_aborts"),
    "MGP_DEEP_HALO": ("test_gpu_parity", "test_deep_halo_smoothing_loopback"),
    "MGP_EARLY_X": ("test_gpu_parity", "test_early_post_exchange_loopback"),
    "MGP_ERRS_HOST": (_SW, "test_errs_in_device_memory"),
    "MGP_FRESH": ("test_gpu_block", "test_fresh_first_sweep_matches_oracle"),
    "MGP_FUSED": ("test_gpu_dense", "test_dense_zs_split_and_k_zs"),
    "MGP_FUSED_MIN_CELLS": ("test_gpu_dense", "test_dense_zs_split_and_k_zs"),
    "MGP_GRAPH": ("test_gpu_parity", "test_graph_replay_equals_eager"),
    "MGP_GS": ("test_gpu_parity", "test_grid_stride_half_sweep_equals_one_shot"),
    "MGP_KEEP_PSI_OLD": ("test_gpu_parity", "test_metrics_under_temporally_blocked_finest_level"),
    "MGP_LAZY_ZERO": ("test_gpu_dense", "test_dense_two_fused_levels_zpost_and_lazy_zero"),
    "MGP_LAZY_ZERO_FUSED": (_SW, "test_lazy_zero_fused_off"),
    "MGP_NT": (_SW, "test_nontemporal_finest_half_sweep"),
    "MGP_PAD_BYTES": ("test_gpu_pad", "test_buffer_offsets_do_not_change_results"),
    "MGP_PLANE_PAD": (_SW, "test_plane_pad_level0_engines"),
    "MGP_POST1": ("test_gpu_block", "test_post_first_half_sweep_matches_oracle"),
    "MGP_POST_BLACK": ("test_gpu_block", "test_black_only_prolongation_matches_oracle"),
    "MGP_PRECAPTURE": (_SW, "test_graphs_captured_on_first_use"),
    "MGP_RBSWEEP": ("test_gpu_bres", "test_rbsweep_smoothing_calls_match_oracle"),
    "MGP_RESFW": ("test_gpu_dense_fw", "test_dense_fw_resfw_against_two_passes"),
    "MGP_RR_PAIR_CELLS": (_SW, "test_pair_residual_restrict_on_every_level"),
    "MGP_RR_SCALAR_CELLS": (_SW, "test_vector_residual_restrict_on_every_level"),
    "MGP_TAIL": ("test_gpu_dense", "test_dense_k_tail"),
    "MGP_TAIL_CELLS": (_SW, "test_tail_cells_moves_the_tail"),
    "MGP_TAIL_CUBIC": ("test_gpu_dense", "test_dense_k_tail_c"),
    "MGP_YS_HALF": ("test_gpu_dense", "test_dense_k_ys"),
    "MGP_YS_MIN_CELLS": ("test_gpu_dense", "test_dense_k_ys"),
    "MGP_YS_ROWS": ("test_gpu_parity", "test_ys_phases_match_oracle"),
    "MGP_ZPOST_MIN_CELLS": ("test_gpu_dense", "test_dense_two_fused_levels_zpost_and_lazy_zero"),
    "MGP_ZPOST_PRE": ("test_gpu_zs_split_cl", "test_zpost_level_runs_the_split_pre"),
    "MGP_ZS_FWF": ("test_gpu_dense_fw", "test_dense_fw_fused_into_k_zs_pre"),
    "MGP_ZS_PATCH": (_SW, "test_patch_order_fp32"),
    "MGP_ZS_PATCH_POST": (_SW, "test_patch_order_fp32"),
    "MGP_ZS_PATCH_PRE": (_SW, "test_patch_order_fp32"),
    "MGP_ZS_POST_ZC": (_SW, "test_post_zc_chunks_post_apart_from_pre"),
    "MGP_ZS_SPLIT": ("test_gpu_dense", "test_dense_zs_split_and_k_zs"),
    "MGP_ZS_SPLIT_CL": ("test_gpu_zs_split_cl", "test_revisits_stay_on_k_zs"),
    "MGP_ZS_SPLIT_POST": ("test_gpu_zs_split_post", "test_split_post_selection"),
    "MGP_ZS_SPLIT_POST_MIN_CELLS": ("test_gpu_zs_split_post", "test_split_post_selection"),
    "MGP_ZS_WGS": (_SW, "test_patch_order_fp32"),
    "MGP_ZS_WIDE": ("test_gpu_dense", "test_dense_zs_split_and_k_zs"),
}

# switch -> why no test sets it to compare bits
EXEMPT = {
    "MGP_ROCTX": "needs the profiler's marker library at run time; a process-wide singleton that also turns replay off",
    "MGP_TEST_STALL": "a test hook of the communication deadline, not a setting of the solver",
    "MGP_TEST_FAIL_RANK": "a test hook that makes one rank of a group fail, not a setting of the solver",
    "MGP_STAMP_R": "measurement only: timing builds write wall-clock stamps over a level's f",
    "MGP_COPY_CALIB": "measurement only: extra lane widths of the copy-bandwidth probe",
    "MGP_TRANSPORT": "selects the communication transport of a one-rank context, which test_gpu_rccl.py is about",
}


def _switches_read():
    names = set()
    for fn in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, fn)
        if not os.path.isfile(path):
            continue
        with open(path, encoding="utf-8", errors="replace") as fh:
            for line in fh:
                if "getenv(" in line:  # (one call names two: getenv(dim == 2 ? "MGP_A" : "MGP_B"))
                    names.update(re.findall(r'"(MGP_[A-Z0-9_]+)"', line.split("getenv(", 1)[1]))
    return names


def test_the_scan_finds_the_switches():
    names = _switches_read()
    assert len(names) >= 50, sorted(names)
    assert {"MGP_FUSED", "MGP_YS_MIN_CELLS", "MGP_FUSED_MIN_CELLS", "MGP_RR_SCALAR_CELLS", "MGP_TAIL_CUBIC"} <= names


def test_every_switch_is_tested_or_exempt():
    names = _switches_read()
    both = set(TESTED) & set(EXEMPT)
    assert not both, f"in both tables: {sorted(both)}"
    missing = names - set(TESTED) - set(EXEMPT)
    assert not missing, f"read by the library but in neither table of this file: {sorted(missing)}"
    stale = (set(TESTED) | set(EXEMPT)) - names
    assert not stale, f"listed here but no longer read by the library: {sorted(stale)}"
    assert all(reason.strip() for reason in EXEMPT.values())


def test_the_named_tests_exist_and_name_their_switch():
    sources = {}
    for name, (module, function) in TESTED.items():
        if module not in sources:
            with open(os.path.join(TESTS, module + ".py"), encoding="utf-8") as fh:
                sources[module] = fh.read()
        src = sources[module]
        assert re.search(r"^def %s\(" % re.escape(function), src, re.M), f"{module}.{function} does not exist"
        assert re.search(r"\b%s\b" % name, src), f"{module} never names {name}"


def test_every_tested_switch_is_documented():
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as fh:
        readme = fh.read()
    # (README writes the tile settings of one family as MGP_ZS_PATCH_PRE / MGP_YS_* too: whole names only)
    missing = [n for n in sorted(TESTED) if not re.search(r"\b%s\b" % n, readme)]
    assert not missing, f"not in README.md's switch list: {missing}"
