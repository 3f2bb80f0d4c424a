// mgp_internal.h — shared declarations between the C-ABI layer (mgp_api.cpp) and the CDNA4 kernel units:
// mgp_kernels.hip (one launch per piece; k_zs's stage-split variants and the 2D k_ys), mgp_zs.hip / mgp_zs_f64.hip (k_zs, the fused
// phases' planning and dispatch), mgp_tail.hip (coarse tail), mgp_blk.hip / mgp_blk2.hip (tiled phases), mgp_gslex.hip,
// mgp_fw.hip, mgp_bres.hip, mgp_refine.hip, mgp_batch.hip, mgp_krylov.hip, mgp_mean.hip, mgp_fmg.hip, mgp_project.hip, mgp_vc.hip.  The last block holds what the kernel units
// call in each other.  Not part of the public ABI (include/mgpoisson.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace mgp {

// The boundary coefficient c_l of level `level` (ghost = -c_l * boundary cell) for mgp_opts.coarse_bc: the ONE rule
// every reader of cl follows (engine selection, z-chunk planning, the tail, the field views, the norms, the pieces,
// the batch).  0 MGP_BC_ZERO: 0; 1 MGP_BC_CONSISTENT: 0 on level 0, (2^l - 1) / (2^l + 1) below; 2 MGP_BC_FACE: +1
// and 3 MGP_BC_NEUMANN: -1 on every level.
inline double coarse_coef(int coarse_bc, int level)
{
    if (coarse_bc == 2) return 1.0;
    if (coarse_bc == 3) return -1.0;
    if (coarse_bc != 1 || level <= 0) return 0.0;
    const double p = std::ldexp(1.0, level);
    return (p - 1.0) / (p + 1.0);
}

constexpr int kGhost3D = 1;  // ghost planes per side of every 3D level
// ... when a slab-distributed level runs the temporally blocked phases (k_zs): PRE reads 5 planes
// of u and f beyond its slab, POST 4 of u and f and 3 coarse planes of V
constexpr int kGhostZs = 5;
constexpr int kZsHaloPre = 5, kZsHaloPost = 4, kZsHaloCoarse = 3;

// Device layout of one level ("red/black packed").  A level is a stack of planes (one plane in
// 2D).  Each plane holds its red cells ((i + j + gk) even) in the first half and its black cells
// in the second half; a half is ny rows of hw = max(1, nx/2) cells and cell (i, j) sits at
// m = i >> 1 of its row.  Every stencil neighbour of a cell has the other colour, at
// m - 1 + (i & 1) and m + (i & 1) for x-1 / x+1 and at m for y +- 1, z +- 1, so a half-sweep is a
// plain streaming stencil over one half reading the other half.  3D levels carry one ghost plane
// below and above (zeros at the physical boundary, the neighbour rank's plane across a slab
// edge); kernels receive pointers to interior plane 0.
struct Geo {
    int nx, ny;     // cells per row / rows per plane (powers of two)
    int lx, ly;     // log2(nx), log2(ny)
    int hw, lhw;    // cells per half row = max(1, nx / 2), log2(hw)
    int64_t nz;     // local planes (1 in 2D)
    int64_t H;      // cells per half plane = hw * ny
    int64_t P;      // plane stride = 2 H
    int64_t z0;     // global index of local plane 0
    int64_t gnz;    // global planes of this level (1 in 2D)
};

// Kernel-form settings of the one-launch-per-piece cycle, read from the environment ONCE, when a context is created,
// and kept in it (like FusedTuning below); a caller without a context passes the defaults.
struct PieceTuning {
    // MGP_RR_SCALAR_CELLS: residual + restriction below this many coarse cells runs one thread per coarse cell
    // (k_resrestrict_s) instead of one 16-byte vector of them along x (k_resrestrict<T, D>)
    int64_t rr_scalar_cells = (int64_t)1 << 22;
    bool rr_scalar_env = false;  // MGP_RR_SCALAR_CELLS was given (the coefficient path's 16-byte form runs only then)
    // MGP_RR_PAIR_CELLS: from this many coarse cells up to rr_scalar_cells, fp32 runs two coarse cells per thread
    // (k_resrestrict<T, D, 2>); -1: the default rule, 2D from 2^18 and 3D never
    int64_t rr_pair_cells = -1;
    int bres_vn = -1;  // MGP_BRES_VN: cells per thread of k_bres / k_rbsweep (0 the scalar forms, 1 / 2 / 4; -1: 16 bytes)
    bool nt = false;   // MGP_NT=1: the finest level's half-sweep stores non-temporally (k_half<T, D, 2, .>)
};
PieceTuning piece_tuning_from_env();

// Launchers enqueue on `s` and return the launch's hipGetLastError().  rb = sizeof(real),
// dim = 2 or 3.  `fine` selects the finest-level instantiation (a distinct symbol, so rocprofv3
// reports the finest smoother on its own line).
//
// The launchers of the per-piece cycle (half-sweep, residual + restriction, full weighting, prolongation +
// correction, err sum, the residual / errorBuf views and the residual norm) also take rb = kRealF32D:
// float buffers with every expression evaluated in double and rounded once at the store — cpu-raw.lua
// under real = 'float' (cpu-raw.lua:142-153: LuaJIT numbers are doubles; mgp_opts.arith =
// MGP_ARITH_DOUBLE).  Those run the scalar kernels templated on the compute type (C = double).
constexpr int kRealF32D = 12;

// f = -1e6 at global (cx, cy, cz), 0 elsewhere; u = -f (cpu.lua:180-193).
hipError_t launch_init_point_charge(int rb, int dim, void* u, void* f, Geo g, int64_t cx, int64_t cy,
                                    int64_t cz, hipStream_t s);
// lexicographic (x fastest, this rank's planes) <-> packed
hipError_t launch_pack(int rb, const void* lex, void* packed, Geo g, hipStream_t s);
hipError_t launch_unpack(int rb, const void* packed, void* lex, Geo g, hipStream_t s);
// Fingerprint of a packed field (this rank's planes): out_h = sum mod 2^64 of a per-cell mix of the
// bits and the global lexicographic index; out_d = {sum, sum of squares, max |x|} in fp64.
// hpart / dpart: kSumBlocks / 3 * kSumBlocks scratch.
hipError_t launch_field_stats(int rb, const void* packed, Geo g, uint64_t* hpart, double* dpart, uint64_t* out_h,
                              double* out_d, hipStream_t s);

// Computed views for mgp_get_field (cpu-raw.lua's rs / errorBuf): r = f - A u at every packed slot, and
// out = (a - b)^2 elementwise over n packed reals.
hipError_t launch_residual_field(int rb, int dim, const void* u, const void* f, void* r, Geo g, double h, double cl,
                                 hipStream_t s);
hipError_t launch_sqdiff_field(int rb, const void* a, const void* b, void* out, int64_t n, hipStream_t s);

// One colour of a red/black sweep: dst(colour c) = relax(other(1-c), f) (cpu.lua:40-54 update).
// other and dst may be the same buffer (in place) or different (out of place: Jacobi, the first
// sweep of a cycle).  With old != nullptr, sum (dst - old)^2 over colour c goes to one fp64
// partial per workgroup in partials[0 .. half_blocks()).
// gs: large levels use the grid-stride form (kGsBlocks workgroups, XCD-banded)
int half_blocks(int rb, Geo g, bool gs);
hipError_t launch_half_sweep(int rb, int dim, bool fine, int color, const void* other, const void* f, void* dst,
                             const void* old, double* partials, Geo g, double h, double cl, bool gs,
                             const PieceTuning& pt, hipStream_t s);
// The first red/black sweep of a fresh zero guess (cpu.lua:138) in one pass: u (both colours) from f
// alone, bit-identical to the red and black half-sweeps reading u = 0.  Levels with hw >= 16 / rb.
bool fresh_supported(int rb, const Geo& g);
// store_red = false: the red cells are left as they are (a later sweep's red half-sweep replaces them unread).
hipError_t launch_fresh_sweep(int rb, int dim, const void* f, void* u, Geo g, double h, double cl, hipStream_t s,
                              bool store_red = true);
// prolong_correct + the red half of the first post-smoothing sweep in one pass: red cells of u from black u
// + P V (never stored: the black half-sweep that follows replaces the black cells without reading
// them).  Vector levels of one rank's box with coarse nx >= 16 / rb.
bool post1_supported(int rb, const Geo& g, const Geo& gc);
hipError_t launch_post_first(int rb, int dim, int linear, void* u, const void* V, const void* f, Geo g, Geo gc,
                             double h, double cl, double clc, hipStream_t s);
// Fused residual + restriction (calcResidual + reduceResidual): R (coarse packed, pointing at the
// coarse plane of this rank's fine plane 0; its Geo is gc) from u, f of the fine level.
hipError_t launch_residual_restrict(int rb, int dim, const void* u, const void* f, void* R, Geo g, Geo gc, double h,
                                    double cl, const PieceTuning& pt, hipStream_t s);
// The last black half-sweep of a red/black pre-smoothing + residual + restriction in one pass (k_bres): u's black
// cells relaxed in place from its (final) red cells and f, R as launch_residual_restrict would compute it from the
// swept u.  Bit-identical to launch_half_sweep(colour 1, in place) + launch_residual_restrict.  Real arithmetic
// (rb 4 / 8), a replicated level (planes -1 and nz are not read) with nx, ny (and nz) >= 2.
bool bres_supported(int rb, const Geo& g);
hipError_t launch_black_residual_restrict(int rb, int dim, void* u, const void* f, void* R, Geo g, Geo gc, double h,
                                          double cl, const PieceTuning& pt, hipStream_t s);
// One whole red/black sweep in one pass (k_rbsweep): dst's black cells (and with store_red its red ones) = the sweep
// of src, read from src's black cells and f only (src != dst; same shapes as launch_black_residual_restrict).
// Bit-identical to the red and black launch_half_sweep pair.
hipError_t launch_rb_sweep(int rb, int dim, const void* src, const void* f, void* dst, Geo g, double h, double cl,
                           bool store_red, const PieceTuning& pt, hipStream_t s);
// Full-weighting restriction (mgp_opts.restriction, build-defined): r = f - A u of the level's own planes
// into the scratch r (same packed layout and ghost planes as the level), then R (coarse packed, Geo gc)
// from r, which must have current planes -1 and g.nz (zero at the physical boundary, the neighbours'
// planes across a slab edge).  clc: the coarse level's boundary coefficient (face weight 3 - clc).
hipError_t launch_residual_field_v(int rb, int dim, const void* u, const void* f, void* r, Geo g, double h, double cl,
                                   hipStream_t s);
hipError_t launch_fw_restrict(int rb, int dim, const void* r, void* R, Geo g, Geo gc, double clc, hipStream_t s);
// calcResidual + the full weighting in one z-streamed pass from u and f (k_resfw, mgp_fw.hip): R of the coarse
// level (gc) bit-identical to launch_residual_field_v + launch_fw_restrict, without the level-sized residual.
// gz: readable ghost planes of u / f per side (a slab level needs u two and f one plane deep: resfw_supported).
bool resfw_supported(int rb, int dim, const Geo& g, int gz, bool dist);
hipError_t launch_resfw(int rb, int dim, const void* u, const void* f, void* R, Geo g, Geo gc, double h, double cl,
                        double clc, int gz, hipStream_t s);
// u += P V (expandResidual + addTo); V points at the coarse plane gc.z0, which must correspond to
// this rank's fine plane 0; planes -1 and gc.nz of V must be readable for the linear kind.
// black_only: the black cells only (before a red/black post-smoothing: its red half-sweep replaces
// every red cell without reading it).
hipError_t launch_prolong_correct(int rb, int dim, int linear, void* u, const void* V, Geo g, Geo gc, double clc,
                                  hipStream_t s, bool black_only = false);
// The passes of the full multigrid start (mgp_fmg.hip; rb = 4 / 8, one rank's whole box: z0 = 0, every plane local).
// launch_restrict_field: R (coarse packed, Geo gc) = the 2^d average of the stored field f in reduceResidual's term
// order (the full weighting of a stored field is launch_fw_restrict).  launch_fmg_prolong: every cell of u = P3 V, the
// separable cubic interpolation (x, y, z passes; ghosts -clc times the mirrored in-box line; mgp_fmg.hip's header has
// the expressions).  V's and u's ghost planes are not read.
hipError_t launch_restrict_field(int rb, int dim, const void* f, void* R, Geo g, Geo gc, hipStream_t s);
hipError_t launch_fmg_prolong(int rb, int dim, void* u, const void* V, Geo g, Geo gc, double clc, hipStream_t s);
// launch_fmg_prolong's vector form on the B members of a batch (mgp_batch.hip) in one launch: member m's u / V start
// m * us / m * vs reals into the buffers; active (device, may be nullptr: every member) skips the members whose entry
// is 0.  The vector form needs coarse rows of at least 16 bytes of reals: the batch tests that itself and runs its
// scalar form on smaller levels, so hipErrorInvalidValue (that condition, or inconsistent geometries or strides) is
// an error to it like any other.
hipError_t launch_fmg_prolong_batch(int rb, int dim, void* u, const void* V, Geo g, Geo gc, double clc, int B, int64_t us,
                                    int64_t vs, const int* active, hipStream_t s);
// Deterministic two-pass fp64 sum of (a - b)^2 over n elements into *out (ctr != nullptr: into
// out[*ctr], then ++*ctr on the device).
// lev (here and in launch_metrics): a and b are whole levels of that layout, n = lev->P * planes.  The sum then runs
// over the level's own slots in the order of an unpadded plane stride, so MGP_PLANE_PAD does not change its bits.
hipError_t launch_sqdiff_sum(int rb, const void* a, const void* b, int64_t n, double* partials, double* out,
                             hipStream_t s, int* ctr = nullptr, const Geo* lev = nullptr);
// out[0..2] = {sum |1 - psi/psiOld| over nonzero entries, their count, sum (psi - psiOld)^2}
// over n elements; partials needs 3 * kSumBlocks doubles.
// Debugging check (cpu-raw.lua:126-140, gpu.lua:269-284): *first = min(*first, id) if p[0, n) holds a NaN or inf.
hipError_t launch_nonfinite_check(int rb, const void* p, int64_t n, int id, int* first, hipStream_t s);
hipError_t launch_metrics(int rb, const void* psi, const void* old, int64_t n, double* partials, double* out,
                          hipStream_t s, const Geo* lev = nullptr);
// out[0] = sum (f - A u)^2, out[1] = sum f^2 over the level's cells (fp64, wave-level then fixed-order
// reductions).  partials: 2 * (resnorm_blocks() + sum_scratch(resnorm_blocks())) doubles.
int resnorm_blocks(int rb, Geo g);
hipError_t launch_residual_norm(int rb, int dim, const void* u, const void* f, Geo g, double h, double cl,
                                double* partials, double* out, hipStream_t s);
// Fixed-order fp64 sum of n partials into *out.  Needs sum_scratch(n) doubles of scratch right
// after partials[n - 1].
int sum_scratch(int n);
hipError_t launch_sum_partials(const double* partials, int n, double* out, hipStream_t s, int* ctr = nullptr);

// Mixed-precision defect correction on level 0 (mgp_refine.hip, mgp_refine_*): fp64 psi64 / f64 in level 0's packed
// layout (same element offsets and ghost planes as the fp32 fields; pointers to interior plane 0).
// launch_defect: r = f64 - A psi64 in double (Op<double, DIM>::residual with level 0's cl: bit for bit
// launch_residual_field(rb = 8); cl != 0 runs an instantiation of its own), (float)r to r32, +0.0f to u32_or_null when set (every packed slot, as a memset
// would leave it); out[0] = sum r^2 (before narrowing), out[1] = sum f64^2, fp64 in fixed order.
// launch_refine_add: psi64 += (double)e32 over the interior planes; out[0] = sum e32^2.
// partials: refine_partials() doubles.  Rows of >= 4 cells take the 16-byte form (grid-stride and XCD-banded from
// 2^20 two-cell items: defect_blocks() == 2048), shorter rows a thread per slot.
int defect_blocks(Geo g);
int refine_add_blocks(Geo g);
int refine_partials();
hipError_t launch_defect(int dim, const double* psi64, const double* f64, float* r32, float* u32_or_null, Geo g,
                         double h, double cl, double* partials, double* out, hipStream_t s);
hipError_t launch_refine_add(double* psi64, const float* e32, Geo g, double* partials, double* out, hipStream_t s);
// exact widening / round-to-nearest narrowing of n packed reals
hipError_t launch_refine_widen(const float* src, double* dst, int64_t n, hipStream_t s);
hipError_t launch_refine_narrow(const double* src, float* dst, int64_t n, hipStream_t s);

// Removing a field's mean (mgp_mean.hip, mgp_remove_mean / mgp_refine_remove_mean).  p: interior plane 0 of a packed
// field of layout g, rb = 4 / 8.  launch_mean_sum: out[0] = the fp64 sum of this rank's cells in a fixed order (per
// wave, per workgroup, then launch_sum_partials); pad slots, ghost planes and the empty slots of nx = 1 rows do not
// enter it.  partials: kSumBlocks doubles.  launch_mean_sub: out[1] = out[0] / cells (the global count; out[0] all-
// reduced first on a distributed level), then every cell becomes RN((double)x - out[1]), 16 bytes per access where
// the rows allow.
hipError_t launch_mean_sum(int rb, const void* p, Geo g, double* partials, double* out, hipStream_t s);
hipError_t launch_mean_sub(int rb, void* p, Geo g, double cells, double* out, hipStream_t s);

// The operators of a MAC-grid projection (mgp_project.hip; mgp_divergence / mgp_gradient in include/mgpoisson.h have the
// definitions).  rb = 4 / 8, one rank's whole box; f / u: interior plane 0 of level 0's packed f / psi (layout g); vx,
// vy, vz: the caller's lexicographic face arrays in device memory ((nx+1) ny nz, nx (ny+1) nz, nx ny (nz+1) reals; vz
// is not touched in 2D).  launch_divergence writes every cell of f and nothing else of it; launch_gradient stores G psi
// into the faces or (subtract) subtracts it from them, with the ghosts -cl times the boundary cell.
hipError_t launch_divergence(int rb, int dim, const void* vx, const void* vy, const void* vz, void* f, Geo g, hipStream_t s);
hipError_t launch_gradient(int rb, int dim, bool subtract, const void* u, void* vx, void* vy, void* vz, Geo g, double cl,
                           hipStream_t s);
// The same two on nm consecutive members of a batch (mgp_batch.hip) in ONE launch each: g is one member's box (z0 = 0,
// P = 2 H, a power-of-two number of slots nz * P), f / u the first of those members' packed field (the next member
// nz * P reals on), vx / vy / vz those members' face arrays, member slowest and contiguous ((nx+1) ny nz etc. reals per
// member).  The vector form runs when launch_divergence's conditions hold for the first member and the member strides of
// the packed field and of vy / vz are multiples of 16 bytes, the scalar form otherwise.  hipErrorInvalidValue: nm < 1 or
// g is no member box.
hipError_t launch_divergence_batch(int rb, int dim, const void* vx, const void* vy, const void* vz, void* f, Geo g, int nm,
                                   hipStream_t s);
hipError_t launch_gradient_batch(int rb, int dim, bool subtract, const void* u, void* vx, void* vy, void* vz, Geo g, double cl,
                                 int nm, hipStream_t s);

// The variable-coefficient operator A_beta u = div(beta grad u) (mgp_vc.hip; mgp_set_coefficients in
// include/mgpoisson.h has the definition).  rb = 4 / 8, one rank's whole box.  A level's coefficients: b[axis] = interior
// plane 0 of an array in the level's packed layout (ghost planes as u has them) that holds each cell's LOWER face of
// that axis, the faces z = nz in its upper ghost plane; wx = the faces x = nx as [k][j] (ny nz reals); wy = the faces
// y = ny as [k][i & 1][i >> 1] (2 hw nz reals).  b[2] is not touched in 2D.
struct VcCoef {
    void* b[3];
    void* wx;
    void* wy;
};
// bad |= bit when one of p[0, n) is not finite and > 0
hipError_t launch_vc_check(int rb, const void* p, int64_t n, int* bad, int bit, hipStream_t s);
// lex: the faces of `axis` in mgp_divergence's lexicographic layout (device memory)
hipError_t launch_vc_pack(int rb, int dim, int axis, const void* lex, VcCoef vc, Geo g, hipStream_t s);
hipError_t launch_vc_unpack(int rb, int dim, int axis, VcCoef vc, void* lex, Geo g, hipStream_t s);
// the coarse level's (gc) faces of `axis`: the mean of the 2^(d-1) fine faces that tile each
hipError_t launch_vc_coarsen(int rb, int dim, int axis, VcCoef fine, Geo g, VcCoef coarse, Geo gc, hipStream_t s);
// The pieces, as launch_half_sweep / launch_residual_restrict / launch_residual_field / launch_residual_norm /
// launch_gradient define them, on A_beta.  The half-sweep's err partials: half_blocks_vc() per colour; the norm's
// scratch: 2 * (resnorm_blocks_vc() + sum_scratch(resnorm_blocks_vc())) doubles.
int half_blocks_vc(int rb, Geo g);
hipError_t launch_half_sweep_vc(int rb, int dim, int color, const void* other, const void* f, void* dst, const void* old,
                                double* partials, Geo g, double h, double cl, VcCoef vc, hipStream_t s);
hipError_t launch_residual_restrict_vc(int rb, int dim, const void* u, const void* f, void* R, Geo g, Geo gc, double h,
                                       double cl, VcCoef vc, const PieceTuning& pt, hipStream_t s);
hipError_t launch_residual_field_vc(int rb, int dim, const void* u, const void* f, void* r, Geo g, double h, double cl,
                                    VcCoef vc, hipStream_t s);
int resnorm_blocks_vc(Geo g);
hipError_t launch_residual_norm_vc(int rb, int dim, const void* u, const void* f, Geo g, double h, double cl, VcCoef vc,
                                   double* partials, double* out, hipStream_t s);
hipError_t launch_gradient_vc(int rb, int dim, bool subtract, const void* u, void* vx, void* vy, void* vz, Geo g,
                              double cl, VcCoef vc, hipStream_t s);

// Temporally blocked smoothing phases of a replicated 3D red/black level (ns = 2 sweeps):
//   pre : dst = nu1 sweeps of src; R (coarse packed, Geo gc) = restrict(residual(dst))
//   post: dst = nu2 sweeps of (src + P V); with partials, sum (dst - dst_before)^2 per workgroup
// src and dst are different buffers (tiles read each other's halos of src).
// Tile settings of the temporally blocked phases (k_zs / k_ys), read from the environment ONCE, when a context is
// created, and kept in it: the sizes planned then (z-chunks, the err partials buffer, mgp_plan's engines) are the
// ones every later launch uses (they used to be re-read per launch).
struct FusedTuning {
    bool wide = true;    // MGP_ZS_WIDE=0: POST on the narrow 64 x 32 tile
    int ys_half = -1;    // MGP_YS_HALF: 2D segment width rule (-1 auto, 0 full, 1 half)
    int ys_rows = 32;    // MGP_YS_ROWS: 2D rows per workgroup chunk
    int64_t wgs = 256;   // MGP_ZS_WGS: z-chunks are halved until a launch has this many workgroups
    // tile order of launches of > 512 workgroups: px | py << 8 patches of tiles per XCD band, 0 = tile rows
    // (MGP_ZS_PATCH=px,py sets both phases, MGP_ZS_PATCH_PRE / MGP_ZS_PATCH_POST one; "0" off; -1: POST's default,
    // 4 x 8 on planes of >= 4096 tiles)
    int patch_pre = 0, patch_post = -1;
    bool fwf = true;     // MGP_ZS_FWF=0: the full weighting after the fused PRE instead of inside it
    int post_zc = 256;   // MGP_ZS_POST_ZC: POST's z-chunks hold at most this many planes (0: no limit)
    bool split = true;   // MGP_ZS_SPLIT=0: fp32 cl = 0 PRE (2^3 average) on k_zs instead of the stage-split k_zs_split
    // MGP_ZS_SPLIT_CL=1: a fused cl != 0 level's fp32 PRE from a fresh guess on k_zs_split_cl instead of k_zs (off:
    // on the slab workloads its gain, 1.4-1.9 % per interleaved pair, stayed inside the round-to-round drift)
    bool split_cl = false;
    // MGP_ZPOST_PRE=0: the PRE of a `zpost` level one launch per piece, also where k_zs_split_cl applies (on: the
    // 256^3 level of the 512^3 box, 87 -> 57 us)
    bool zpost_pre = true;
    // MGP_ZS_SPLIT_POST=0: fp32 cl = 0 POST (trilinear P, the wide tile) on k_zs instead of the stage-split
    // k_zs_split_post; MGP_ZS_SPLIT_POST_MIN_CELLS: the smallest level (cells per rank) that takes it
    bool split_post = true;
    int64_t split_post_min_cells = (int64_t)1 << 27;
    bool stamp_r = false;  // MGP_STAMP_R=1 (ZS_STAMP timing builds only): POST's wall-clock stamps go to level l+1's f
};
FusedTuning fused_tuning_from_env();

// What a launcher actually launched: the kernel's symbol as rocprofv3 prints it (template arguments included)
// and its grid in work-items (rocprofv3's Grid_Size), so measured PMC traffic can be matched to this launch
// (bench.py) instead of being re-derived from the options.
struct LaunchInfo {
    char name[96];
    int64_t grid;
};

struct FusedArgs {
    FusedTuning tu;
    LaunchInfo* info;  // optional out: the launched kernel
    bool pre;
    int linear;  // POST: linear prolongation; PRE: 1 = no restriction (both colours stored, full weighting after),
                 // 2 = the full-weighting restriction fused (fused_fwf_supported)
    const void* src;
    const void* f;
    void* dst;
    const void* old;  // POST + err: psiOld (nullptr: dst, overwritten plane by plane as the output is stored)
    void* R;
    const void* V;
    double* partials;
    Geo g, gc;
    double h, cl, clc;
    int zc;
    int ghost;  // readable ghost planes per side of src / f / dst
};
bool fused_supported(int rb, int dim, int ns, const Geo& g, const FusedTuning& tu);
// Raise the dynamic-LDS limit of the fused and tail kernels (once per context, before any capture).
hipError_t prepare_kernels(int rb);
// clz: the level's operator has no boundary modification (cl == 0): PRE's tile may differ otherwise
int fused_zc(int rb, const Geo& g, bool pre, bool clz, const FusedTuning& tu);
int fused_blocks(int rb, const Geo& g, int zc, bool clz, const FusedTuning& tu);
hipError_t launch_fused(int rb, const FusedArgs& a, hipStream_t s);
// PRE with the full weighting fused (FusedArgs::linear = 2): fp32, cl = 0, a replicated level (MGP_ZS_FWF=0: off)
bool fused_fwf_supported(int rb, int dim, bool clz, bool dist, const FusedTuning& tu);

// Tiled smoothing phases of a small replicated red/black level (k_blk: one launch per phase, the 3D
// or 2D tile and its halo in LDS):
//   pre : dst = ns sweeps of src; R (coarse packed, Geo gc) = restrict(residual(dst))
//   post: dst = ns sweeps of (src + P V)
// src == nullptr reads u = 0 (a fresh coarse guess).  src != dst.
constexpr int kBlkMaxSweeps = 2;
constexpr int kBlkTile = 8;     // 3D owned tile edge (every axis of a tiled level is a multiple)
constexpr int kBlkTile2D = 32;  // 2D owned tile edge
struct BlockArgs {
    bool pre;
    int linear;  // POST: linear prolongation; PRE: 1 = full-weighting restriction (face weight 3 - clc)
    int ns;
    const void* src;
    const void* f;
    void* dst;
    void* R;
    const void* V;
    Geo g, gc;
    double h, cl, clc;
};
bool block_supported(int rb, int dim, int ns, const Geo& g);
hipError_t launch_block(int rb, int dim, const BlockArgs& a, hipStream_t s);

// PRE (POST) of two consecutive small 2D levels in one launch (mgp_blk2.hip): level l (g) smoothed and restricted, then
// level l + 1 (g1) smoothed from its guess and restricted onto level l + 2 (g2); POST: level l + 1 corrected from
// level l + 2 and smoothed, then level l corrected from it and smoothed
struct Block2Args {
    bool pre;          // false: POST of level l + 1 then of level l (k_blk2_post)
    int ns;
    int linear;        // POST: linear prolongation
    const void* src;   // level l's u (PRE: nullptr = a fresh zero guess)
    const void* f;
    void* dst;         // level l's smoothed u (PRE: black cells; POST: both colours)
    void* f1;          // level l + 1's f (PRE: written, both colours; POST: read)
    const void* src1;  // level l + 1's u (PRE: the warm guess, nullptr = a fresh zero guess)
    void* dst1;        // level l + 1's smoothed u
    void* R;           // level l + 2's f
    const void* V2;    // POST: level l + 2's u (the correction prolongated into level l + 1)
    Geo g, g1, g2;
    double h, cl, cl1, cl2;  // h of level l (level l + 1: 2 h); the coarse-boundary coefficients of levels l .. l + 2
};
bool block2_supported(int rb, int dim, int ns, const Geo& g, const Geo& g1, const Geo& g2);
hipError_t launch_block2(int rb, int dim, const Block2Args& a, hipStream_t s);
hipError_t blk2_attr(int rb);

// Coarse-level tail: the sub-cycle below one level as a single one-workgroup launch with every
// level in LDS.  ops[] = (op | level << 4 | arg << 8), levels relative to the tail's first level.
constexpr int kTailMaxLevels = 8;
constexpr int kTailMaxOps = 192;
constexpr size_t kTailMaxLds = 160 * 1024;  // gfx950 LDS per workgroup
// (TAIL_FMG_*: the batch's LDS ascent only, mgp_batch.hip: f of level + 1 = R f of level; u of level = P3 u of level + 1)
enum TailOp { TAIL_SMOOTH = 1, TAIL_RR = 2, TAIL_ZERO = 3, TAIL_PROLONG = 4, TAIL_FMG_RESTRICT = 5, TAIL_FMG_PROLONG = 6 };
struct TailSpec {
    int nlev, nops, jacobi, linear;
    int zero_first;  // the first level's u is logically 0 (a fresh guess): loaded as zeros
    int fw;          // TAIL_RR restricts by full weighting (mgp_opts.restriction)
    void* u[kTailMaxLevels];  // interior plane 0 of each level's u / f (global)
    void* f[kTailMaxLevels];
    Geo g[kTailMaxLevels];
    double h[kTailMaxLevels];
    double cl[kTailMaxLevels];
    uint32_t ops[kTailMaxOps];
};
size_t tail_lds_bytes(int rb, int dim, int jacobi, const Geo* g, int nlev);
hipError_t launch_tail(int rb, int dim, const TailSpec& t, hipStream_t s);

// Conjugate gradients on a level's operator (mgp_krylov.hip; converge-multigrid-vs-krylov.lua:38-69).
// Packed level vectors x (in/out), b, and scratch r, p, q; scratch holds cg_scratch_doubles() doubles.
struct CgArgs {
    Geo g;
    double h, cl;
    void *x, *r, *p, *q;
    const void* b;
    double* scratch;
    bool x0_neg_b;    // x0 = -b (the reference's start) instead of x's content
    int maxiter;
    double epsilon;   // stop when rSq / bSq < epsilon
    double* linf;     // optional: |x|_inf after each iteration (maxiter entries)
    int iters;        // out
    double err;       // out: final rSq / bSq
};
int cg_scratch_doubles();
hipError_t launch_cg(int rb, int dim, CgArgs& a, hipStream_t s);

// 16-byte streaming copy of `bytes` (a multiple of 16) for the copy-bandwidth probe; kind 0..2 (kCopyKinds):
// grid-stride / one pass / one pass non-temporal; kinds 3 and 4 (calibration only): 8- and 4-byte lanes
constexpr int kCopyKinds = 3, kCopyCalibKinds = 5;
hipError_t launch_copy16(int kind, const void* src, void* dst, int64_t bytes, hipStream_t s);

// One in-place lexicographic Gauss-Seidel sweep (cpu.lua:24-37) of a whole replicated level, bit-identical to the
// sequential ascending-order sweep: tiles in tile-hyperplane order, one launch per tile-hyperplane (k_gslex).
hipError_t launch_gslex_sweep(int rb, int dim, void* u, const void* f, Geo g, double h, double cl, hipStream_t s);

// Test hook of the communication deadline (MGP_TEST_STALL): one wave that holds stream s until *flag (host-pinned,
// mapped) is non-zero, and in any case at most max_s seconds of wall clock (every wave reaches that exit).
hipError_t launch_stall(const int* flag, double max_s, hipStream_t s);

constexpr int kSumBlocks = 1024;

// ---- between the kernel units; not used by mgp_api.cpp ---------------------------------------------------------
// An anonymous-namespace kernel cannot be named from another unit, so each unit launches its own kernels and raises
// their dynamic-LDS limit itself; prepare_kernels (mgp_zs.hip) chains these with blk2_attr.
hipError_t zs_split_attr(int rb);  // mgp_kernels.hip
hipError_t zs_attr_f64();          // mgp_zs_f64.hip (k_zs's fp64 instantiations; the fp32 ones: mgp_zs.hip)
hipError_t tail_attr(int rb);      // mgp_tail.hip
hipError_t blk_attr(int rb);       // mgp_blk.hip
// fused_dispatch's (mgp_zs.hip) stage-split launches (mgp_kernels.hip), fp32: PRE on a cl = 0 level (from src, or from
// a fresh zero guess when it is null), PRE on a cl != 0 level from a fresh zero guess, POST (err with partials)
hipError_t launch_zs_split(const FusedArgs& a, hipStream_t s);
hipError_t launch_zs_split_cl(const FusedArgs& a, hipStream_t s);
hipError_t launch_zs_split_post(const FusedArgs& a, hipStream_t s);
// launch_fused on a 2D level (k_ys, mgp_kernels.hip), and its segment planning for fused_supported / fused_zc /
// fused_blocks
hipError_t launch_fused_f64(const FusedArgs& a, hipStream_t s);  // launch_fused on a 3D fp64 level (mgp_zs_f64.hip)
hipError_t launch_fused_2d(int rb, const FusedArgs& a, hipStream_t s);
int ys_rows(const Geo& g, const FusedTuning& tu);
int ys_tx(int rb, const Geo& g, const FusedTuning& tu);

}  // namespace mgp
