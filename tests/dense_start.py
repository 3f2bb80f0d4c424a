"""Dense random level-0 start states for whole-cycle parity (test_gpu_dense.py, test_gpu_dense_fw.py, test_gpu_switches.py) and their CPU guard
(test_dense_inputs.py) — TEST INFRASTRUCTURE ONLY.

init_point_charge() leaves one non-zero cell in f and in psi and zeros everywhere else, so a cycle started from it
cannot tell a level-0 load of the wrong f cell (or of u in the first cycle) from the right one: both read a zero.  dense_start()
gives a context, an oracle or a slab rank the same generic fields instead: psi0 and f0 uniform in [-1, 1) from two
seeded generators, cast to the real type.  CASES lists every (box, real, options) the GPU files run, in one place,
so that the CPU guard can hold the reference to the conditions the GPU comparison relies on (finite, no zero and no
subnormal cell, err falling) for exactly those inputs.
"""
from __future__ import annotations

import numpy as np

_PSI, _F = 0, 1  # MGP_FIELD_U / MGP_FIELD_F, and the oracle's `which`


def dense_fields(shape, dtype, seed):
    """(psi0, f0) of a global level-0 shape: uniform(-1, 1) from default_rng(seed) and default_rng(seed + 1)."""
    psi0 = np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(dtype)
    f0 = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, shape).astype(dtype)
    return psi0, f0


def dense_start(x, seed):
    """Set the level-0 psi and f of `x` to the dense fields of `seed` and return them (the global arrays).
    x is an Oracle (set), a Context (set_psi / set_f) or one rank of a slab decomposition, which sets its own
    planes of the same global fields (set_planes)."""
    if hasattr(x, "step"):  # the C oracle
        psi0, f0 = dense_fields(x.shape, x.dtype, seed)
        x.set(_PSI, psi0)
        x.set(_F, f0)
        return psi0, f0
    lv = x.levels[0]
    shape = (lv["nz_global"], lv["ny"], lv["nx"]) if x.opts.dim == 3 else (lv["ny"], lv["nx"])
    psi0, f0 = dense_fields(shape, x.dtype, seed)
    if lv["distributed"]:
        z = slice(lv["z0"], lv["z0"] + lv["nz_local"])
        x.set_planes(_PSI, 0, psi0[z])
        x.set_planes(_F, 0, f0[z])
    else:
        x.set_psi(psi0)
        x.set_f(f0)
    return psi0, f0


RB = dict(smoother="rbgs", nu1=2, nu2=2)
LC = dict(prolong="linear", coarse_bc="consistent")
FW = dict(restriction="full_weighting")
RAW = dict(real="float", arith="double")

# id -> (make_opts / Oracle keywords, seed).  The ids name the engine the GPU file drives with the case; the seeds
# are distinct (seed + 1 seeds f; the reset cases use seed + 10 and seed + 11 for their second pair of fields).
CASES = {
    # 1. k_zs_split / k_zs, fp32, cl = 0 (test_gpu_zs_split.py's BASE and boxes)
    "zs-64x32x16": (dict(dim=3, n=(64, 32, 16), real="float", **RB, **LC), 101),
    "zs-64x32x64": (dict(dim=3, n=(64, 32, 64), real="float", **RB, **LC), 121),
    "zs-128x64x32": (dict(dim=3, n=(128, 64, 32), real="float", **RB, **LC), 141),
    # 2. k_zs, fp64 (FUSED_CONFIGS)
    "zs-f64-128x64x32-pc-zero": (dict(dim=3, n=(128, 64, 32), real="double", prolong="pc", coarse_bc="zero", **RB), 161),
    "zs-f64-64x128x64-warm": (dict(dim=3, n=(64, 128, 64), real="double", coarse_init="warm", **RB, **LC), 181),
    # 3. F-cycle and err_mode = 0 (FUSED_CONFIGS)
    "zs-64-F": (dict(dim=3, n=(64, 64, 64), real="float", cycle="F", **RB, **LC), 201),
    "zs-64x32x128-noerr": (dict(dim=3, n=(64, 32, 128), real="float", prolong="pc", coarse_bc="consistent",
                                err_mode=0, **RB), 221),
    # 4. two fused levels, zpost, the lazy zero (test_lazy_zero_equals_memset's fused box)
    "zs-128": (dict(dim=3, n=(128, 128, 128), real="float", **RB, **LC), 241),
    # 5. k_ys (YS_CONFIGS)
    "ys-1024-f32": (dict(dim=2, n=(1024, 1024, 1), real="float", **RB, **LC), 261),
    "ys-1024x512-f64-zero": (dict(dim=2, n=(1024, 512, 1), real="double", prolong="linear", coarse_bc="zero", **RB), 281),
    "ys-1024-f64-pc": (dict(dim=2, n=(1024, 1024, 1), real="double", prolong="pc", coarse_bc="consistent", **RB), 301),
    "ys-2048x1024-f64-F": (dict(dim=2, n=(2048, 1024, 1), real="double", cycle="F", **RB, **LC), 321),
    # 6. k_blk (BLK_CONFIGS), k_blk2 (test_gpu_blk2.py), k_bres (test_gpu_bres.py), the tail (TAIL_CONFIGS,
    # CUBIC_TAIL_CONFIGS), k_fresh (FRESH_CONFIGS): of each file the smallest 3D and 2D configuration, a non-cubic
    # box wherever the file has one.  (BLK_CONFIGS' only non-square 2D box, 256 x 128 fp32 1 + 2 pc / zero / warm,
    # is left out: from a dense start the reference itself diverges on it, err 0.586, 0.642, 4.65, which
    # test_dense_inputs.py does not admit; the 2D k_blk case is the file's smallest, 128^2.  k_blk2 is 2D only.)
    "blk-64x16x32-f64": (dict(dim=3, n=(64, 16, 32), real="double", smoother="rbgs", nu1=1, nu2=1, prolong="pc",
                              coarse_bc="consistent"), 341),
    "blk-128-f64": (dict(dim=2, n=(128, 128, 1), real="double", smoother="rbgs", nu1=2, nu2=1, **LC), 361),
    "blk2-512x256-f32": (dict(dim=2, n=(512, 256, 1), real="float", prolong="pc", coarse_bc="zero", **RB), 381),
    "bres-64x32x16-f64": (dict(dim=3, n=(64, 32, 16), real="double", prolong="pc", coarse_bc="zero", **RB), 401),
    "bres-128x64-f64": (dict(dim=2, n=(128, 64, 1), real="double", prolong="pc", coarse_bc="zero", smoother="rbgs",
                             nu1=3, nu2=1), 421),
    "tail-64x32x16-f32": (dict(dim=3, n=(64, 32, 16), real="float", smoother="jacobi", nu1=3, nu2=2, cycle="F",
                               prolong="linear", coarse_bc="consistent", coarse_init="warm"), 441),
    "tail-64-f64": (dict(dim=2, n=(64, 64, 1), real="double", coarse_init="warm"), 461),
    "tailc-32x32x64-f64": (dict(dim=3, n=(32, 32, 64), real="double", prolong="pc", coarse_bc="zero", cycle="F",
                                coarse_init="warm", **RB), 481),
    "tailc-128-f64": (dict(dim=2, n=(128, 128, 1), real="double", prolong="pc", coarse_bc="zero", cycle="F",
                           coarse_init="warm", **RB), 501),
    "fresh-32x64x128-f32": (dict(dim=3, n=(32, 64, 128), real="float", smoother="rbgs", nu1=1, nu2=2, **LC), 521),
    # (FRESH_CONFIGS' smaller 2D box, 128^2, has no per-piece level below the finest: 64^2 and below are the
    # tail's, so k_fresh never runs on it; 256^2 has the 128^2 level)
    "fresh-256-f64": (dict(dim=2, n=(256, 256, 1), real="double", cycle="F", **RB, **LC), 541),
    # 7. Jacobi 7 + 7 (the reference configuration) and the lexicographic Gauss-Seidel
    "jacobi-256-f64": (dict(dim=2, n=(256, 256, 1), real="double", smoother="jacobi"), 561),
    "jacobi-32-f64-pc": (dict(dim=3, n=(32, 32, 32), real="double", smoother="jacobi", prolong="pc"), 581),
    "gslex-64-f64": (dict(dim=2, n=(64, 64, 1), real="double", smoother="gs_lex"), 601),
    # 8. level 0 set again in mid-run (k_zs with err: psiOld rotates; per-piece launches)
    "reset-zs-64": (dict(dim=3, n=(64, 64, 64), real="float", **RB, **LC), 621),
    "reset-piece-256-f64": (dict(dim=2, n=(256, 256, 1), real="double"), 641),
    # 9. loopback slabs, world 2 (test_split_loopback_slabs' box)
    "slab-zs-64": (dict(dim=3, n=(64, 64, 64), real="float", **RB, **LC), 661),
    "slab-piece-64-f64": (dict(dim=3, n=(64, 64, 64), real="double", **RB, **LC), 681),
    # ---- test_gpu_dense_fw.py: the two kernel families that have load paths of their own ----
    # 10. the full weighting (FW).  fused into k_zs PRE (LINEAR 2: fp32, cl = 0): one tile with every face a box
    # face, 2 x 2 PRE tiles, two fused levels (level 1 restricts a dense residual from a fresh guess), the F-cycle
    "fw-zs-64x32x16": (dict(dim=3, n=(64, 32, 16), real="float", **RB, **LC, **FW), 701),
    "fw-zs-128x64x32": (dict(dim=3, n=(128, 64, 32), real="float", **RB, **LC, **FW), 721),
    "fw-zs-128-pc-zero": (dict(dim=3, n=(128, 128, 128), real="float", prolong="pc", coarse_bc="zero", **RB, **FW), 741),
    "fw-zs-64-F": (dict(dim=3, n=(64, 64, 64), real="float", cycle="F", **RB, **LC, **FW), 761),
    # fp64: k_zs PRE LINEAR 1 (smoothing only), then k_resfw with 2 x 4 tiles and z-chunk seams
    "fw-zs-f64-128x64x32": (dict(dim=3, n=(128, 64, 32), real="double", **RB, **LC, **FW), 781),
    "fw-zs-f64-128x64x32-zero": (dict(dim=3, n=(128, 64, 32), real="double", prolong="linear", coarse_bc="zero",
                                      **RB, **FW), 801),
    # k_resfw on a per-piece level 0 (3D: two x tiles, two y tiles, four z-chunks; 2D: 2 x 2 tiles) against the
    # two-pass path, and a box with no level k_resfw supports (nx % 64 != 0 on all of them)
    "fw-resfw-128x32x16-f64": (dict(dim=3, n=(128, 32, 16), real="double", **RB, **LC, **FW), 821),
    "fw-resfw-128x32x16-f32-jacobi": (dict(dim=3, n=(128, 32, 16), real="float", smoother="jacobi", nu1=2, nu2=2,
                                           **LC, **FW), 841),
    "fw-resfw-128x64-f64": (dict(dim=2, n=(128, 64, 1), real="double", **RB, **LC, **FW), 861),
    "fw-resfw-128x64-f32-zero": (dict(dim=2, n=(128, 64, 1), real="float", prolong="linear", coarse_bc="zero",
                                      **RB, **FW), 881),
    "fw-two-32x16x8-f32": (dict(dim=3, n=(32, 16, 8), real="float", **RB, **LC, **FW), 901),
    # k_blk's PRE, both coarse tails, k_ys + k_resfw
    "fw-blk-64x16x32-f64": (dict(dim=3, n=(64, 16, 32), real="double", smoother="rbgs", nu1=1, nu2=1, **LC, **FW), 921),
    "fw-blk-128-f64": (dict(dim=2, n=(128, 128, 1), real="double", smoother="rbgs", nu1=2, nu2=1, **LC, **FW), 941),
    "fw-tail-64x32x16-f32": (dict(dim=3, n=(64, 32, 16), real="float", smoother="jacobi", nu1=3, nu2=2, cycle="F",
                                  coarse_init="warm", **LC, **FW), 961),
    "fw-tailc-32x32x64-f64": (dict(dim=3, n=(32, 32, 64), real="double", cycle="F", coarse_init="warm", **RB, **LC,
                                   **FW), 981),
    "fw-ys-1024-f32": (dict(dim=2, n=(1024, 1024, 1), real="float", **RB, **LC, **FW), 1001),
    "fw-ys-1024x512-f64": (dict(dim=2, n=(1024, 512, 1), real="double", **RB, **LC, **FW), 1021),
    # loopback slabs, world 2 (the per-piece case sets its second pair of fields, seed + RESET_SEED_OFFSET, after
    # two cycles)
    "fw-slab-zs-64": (dict(dim=3, n=(64, 64, 64), real="float", **RB, **LC, **FW), 1041),
    "fw-slab-piece-64-f64": (dict(dim=3, n=(64, 64, 64), real="double", **RB, **LC, **FW), 1061),
    # 11. cpu-raw.lua's float arithmetic (float buffers, double expressions): its own kernels on every level
    "raw-64-jacobi": (dict(dim=2, n=(64, 64, 1), **RAW), 1081),  # the reference configuration
    "raw-32x16x8-rbgs": (dict(dim=3, n=(32, 16, 8), **RAW, **RB, **LC), 1101),
    "raw-64x32-gslex": (dict(dim=2, n=(64, 32, 1), smoother="gs_lex", **RAW), 1121),
    "raw-32-fw": (dict(dim=3, n=(32, 32, 32), **RAW, **RB, **LC, **FW), 1141),
    "raw-16x32x16-F-warm": (dict(dim=3, n=(16, 32, 16), smoother="jacobi", nu1=3, nu2=2, cycle="F",
                                 coarse_init="warm", **RAW, **LC), 1161),
    # ---- test_gpu_switches.py ----
    # 12. the tile-patch order of the fused phases: launches of 1024 workgroups (fp32 512 x 512 x 128 and fp64 256^3
    # in 16-plane chunks), the fp32 box with the full weighting fused into PRE as well; the one-tile fp64 box gives
    # the threads per workgroup of the fp64 kernels
    "patch-512x512x128-f32": (dict(dim=3, n=(512, 512, 128), real="float", **RB, **LC), 1201),
    "patch-256-f64": (dict(dim=3, n=(256, 256, 256), real="double", **RB, **LC), 1221),
    "patch-fw-512x512x128-f32": (dict(dim=3, n=(512, 512, 128), real="float", **RB, **LC, **FW), 1241),
    "zs-f64-64x32x16": (dict(dim=3, n=(64, 32, 16), real="double", **RB, **LC), 1381),
    # 13. MGP_PLANE_PAD: level 0's planes hold exactly 2^16 slots, the smallest that takes the padded stride
    "pad-256x256x16-f32": (dict(dim=3, n=(256, 256, 16), real="float", **RB, **LC), 1261),
    "pad-256x256x16-f64": (dict(dim=3, n=(256, 256, 16), real="double", **RB, **LC), 1281),
    "pad-256x256x16-f64-jacobi": (dict(dim=3, n=(256, 256, 16), real="double", smoother="jacobi", nu1=2, nu2=2, **LC), 1301),
    "pad-256x256x16-f32-fw": (dict(dim=3, n=(256, 256, 16), real="float", **RB, **LC, **FW), 1321),
    "pad-256x256x16-f64-gslex": (dict(dim=3, n=(256, 256, 16), real="double", smoother="gs_lex", nu1=2, nu2=2), 1341),
    "pad-slab-256x256x32-f32": (dict(dim=3, n=(256, 256, 32), real="float", **RB, **LC), 1361),
}
RESET_SEED_OFFSET = 10  # the second pair of fields of the cases in SECOND_FIELDS: seed + 10 (psi), seed + 11 (f)
# the cases that set level 0 again in mid-run
SECOND_FIELDS = ("reset-zs-64", "reset-piece-256-f64", "fw-slab-piece-64-f64")


def case(cid):
    """(keywords, seed) of a case; the keywords are a fresh dict."""
    kw, seed = CASES[cid]
    return dict(kw), seed


def oracle_kw(kw):
    """The keywords the oracle takes (it has no err_mode: it computes err every step)."""
    return {k: v for k, v in kw.items() if k != "err_mode"}
