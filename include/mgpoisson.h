/*
 * mgpoisson.h — C ABI of libmgpoisson.so, the MI355X (gfx950) multigrid Poisson hot path.
 *
 * This is the drop-in boundary for the reference's solver classes.  The reference has no
 * native FFI (it is Lua): its boundary is the Lua class protocol of cpu.lua / cpu-raw.lua /
 * gpu.lua.  Each entry point below names the reference interface it replaces;
 * the Lua-side binding (LuaJIT ffi.cdef of this header) is in INTEGRATION.md and
 * lua-multigrid-poisson_amd/lua/multigrid-poisson/hip.lua, the Python mirror in
 * lua-multigrid-poisson_amd/mgpoisson/.
 *
 * Conventions
 *  - Every function returning int returns MGP_OK (0) or a negative mgp_status; the message is
 *    in mgp_last_error(ctx) (or mgp_last_error(NULL) when mgp_create itself failed).  No C++
 *    exception or longjmp crosses this ABI.
 *  - A context owns one HIP stream and all device memory; it is not thread-safe.  Calls are
 *    synchronous at return except where stated.  Host buffers are borrowed for the call.
 *  - Layout is the reference's: x fastest, index = i + nx*(j + ny*k) (cpu-raw.lua:9, gpu.lua:72),
 *    0-based, real = float or double (gpu.lua:32).  With world > 1 a rank owns the z-slab
 *    [z0, z0 + nz_local) of every distributed level (mgp_level_info).
 */
#ifndef MGPOISSON_H
#define MGPOISSON_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGP_API_VERSION 3  /* 2: mgp_opts.restriction; 3: mgp_opts.arith and .api_version appended (232 bytes) */
#define MGP_COMM_ID_BYTES 128 /* == NCCL_UNIQUE_ID_BYTES */

typedef enum mgp_status {
    MGP_OK = 0,
    MGP_ERR_ARG = -1,   /* invalid argument / unsupported configuration */
    MGP_ERR_HIP = -2,   /* HIP runtime error (no device, launch failure, ...) */
    MGP_ERR_RCCL = -3,  /* RCCL error (communicator init, send/recv, collective) */
    MGP_ERR_OOM = -4,   /* device allocation failed */
    MGP_ERR_STATE = -5  /* call not valid in the context's current state */
} mgp_status;

/* cpu.lua:56-57 inPlaceIterativeSolver: Jacobi (cpu.lua:40-54), red/black GS (build-defined, the temporally blocked
 * engines), lexicographic in-place GS (cpu.lua:24-37 GaussSeidel, bit-identical hyperplane-ordered sweeps; one
 * rank's whole box; with MGP_ARITH_DOUBLE cpu-raw.lua:22-32's GaussSeidel over float images) */
enum { MGP_JACOBI = 0, MGP_RBGS = 1, MGP_GS_LEX = 2 };
enum { MGP_CYCLE_V = 0, MGP_CYCLE_F = 1 };             /* twoGrid recursion (gamma 1) / F-cycle */
enum { MGP_PROLONG_PC = 0, MGP_PROLONG_LINEAR = 1 };   /* cpu.lua:142-150 injection / (tri)linear */
enum { MGP_COARSE_FRESH = 0, MGP_COARSE_WARM = 1 };    /* cpu.lua:138 zeros / cpu-raw.lua:221 Vs */
/* Box boundary, through the per-level coefficient c_l of ghost = -c_l * (boundary cell):
 *   MGP_BC_ZERO        the ghost cell CENTRE is 0 on every level (the reference, cpu.lua:28-33): c_l = 0
 *   MGP_BC_CONSISTENT  the same on level 0; the coarse levels' zero moved to that place: c_l = (2^l - 1) / (2^l + 1)
 *   MGP_BC_FACE        u = 0 ON the box face (build-defined): ghost = -u, c_l = +1 on every level, level 0 included
 *   MGP_BC_NEUMANN     du/dn = 0 on the box face (build-defined; the ghost the reference carries commented out as
 *                      `--u[i][j]` on every stencil line, cpu.lua:28-31, 45-48, 114-117, and its "periodic? neumann"
 *                      branch of the one-cell solve, cpu.lua:79-86): ghost = +u, c_l = -1 on every level.  psi is
 *                      determined up to a constant and f must sum to 0 (remove its mean first).  The one-cell level's
 *                      diagonal is 0: a cell whose diagonal is 0 is relaxed to +0 whatever f holds (the minimum-norm
 *                      choice).  The cycle itself does not project.
 * The diagonal of a cell with nb faces on the box is (-2 dim - nb c_l) / h^2, the linear prolongation reads an
 * out-of-box coarse value as -c_l * (boundary value) per axis, the full weighting's face weight is 3 - c_l. */
enum { MGP_BC_ZERO = 0, MGP_BC_CONSISTENT = 1, MGP_BC_FACE = 2, MGP_BC_NEUMANN = 3 };
/* restriction: the 2^dim cell average of cpu.lua:127-135 (reduceResidual) or the cell-centred full
 * weighting (north_star "full-weighting restriction"): the adjoint of the linear prolongation, per axis
 * (1, 3, 3, 1) / 8 over fine cells 2I-1 .. 2I+2, face weight (3 - c) next to the box boundary */
enum { MGP_RESTRICT_AVERAGE = 0, MGP_RESTRICT_FULL_WEIGHTING = 1 };
/* arith: the arithmetic of real = float (no effect on double).  The reference's two float paths disagree:
 *   MGP_ARITH_REAL   every operation rounded to float, gpu.lua's OpenCL `real` (gpu.lua:32) — the default,
 *                    and the arithmetic of the north-star configurations
 *   MGP_ARITH_DOUBLE float buffers, every expression evaluated in double and rounded once where the
 *                    reference stores into a buffer: cpu-raw.lua under real = 'float' (cpu-raw.lua:142-153,
 *                    LuaJIT numbers are doubles; Jacobi :34-44, calcResidual :46-57, reduceResidual :59-63,
 *                    addTo :83-85), err from the float errorBuf (calcFrobErr :96-100, summed in double
 *                    :249-254).  Every level then runs one launch per piece (no fused / tiled / tail engines). */
enum { MGP_ARITH_REAL = 0, MGP_ARITH_DOUBLE = 1 };
/* Fields of a level, by cpu-raw.lua's names (cpu-raw.lua:148-171).  U and F are the stored, writable
 * state; the others are read-only views computed on request from it:
 *   MGP_FIELD_U          psi on level 0, Vs[L] below (the coarse correction)
 *   MGP_FIELD_F          f on level 0, Rs[L] below (the restricted residual)
 *   MGP_FIELD_RESIDUAL   rs[L] = f - A u (calcResidual, cpu.lua:108-123)
 *   MGP_FIELD_CORRECTION vs[L] = P Vs[L/2] (expandResidual, cpu.lua:142-150), the prolonged correction
 *   MGP_FIELD_PSI_OLD    psiOld (level 0): the iterate before the last outer iteration (cpu.lua:200)
 *   MGP_FIELD_ERROR      errorBuf (level 0) = (psi - psiOld)^2 per cell (calcFrobErr, gpu.lua:189-200)
 *   MGP_FIELD_TMP        tmpU: the Jacobi target buffer (cpu-raw.lua:153, 176-184)
 * PSI_OLD / ERROR need err_mode 1 (MGP_ERR_STATE otherwise; a temporally blocked finest level keeps psiOld
 * in a buffer of its own, unless the environment sets MGP_KEEP_PSI_OLD=0).  TMP: MGP_ERR_STATE when the
 * level has no second buffer (red/black Gauss-Seidel works in place). */
enum { MGP_FIELD_U = 0, MGP_FIELD_F = 1, MGP_FIELD_RESIDUAL = 2, MGP_FIELD_CORRECTION = 3, MGP_FIELD_PSI_OLD = 4,
       MGP_FIELD_ERROR = 5, MGP_FIELD_TMP = 6, MGP_FIELD_KINDS = 7 };
enum { MGP_MEM_HOST = 0, MGP_MEM_DEVICE = 1 };         /* where a caller buffer lives */

typedef struct mgp_opts {
    int32_t struct_size;   /* sizeof(mgp_opts), checked by mgp_create */
    int32_t dim;           /* 2 or 3 */
    int64_t n[3];          /* GLOBAL cells per axis, powers of two (n[2] = 1 in 2D) */
    int32_t real_bytes;    /* 4 = float, 8 = double (gpu.lua:32 "real") */
    int32_t nu1, nu2;      /* pre/post sweeps (cpu.lua:20 smooth = 7) */
    int32_t smoother;      /* MGP_JACOBI | MGP_RBGS | MGP_GS_LEX */
    int32_t cycle;         /* MGP_CYCLE_V | MGP_CYCLE_F */
    int32_t prolong;       /* MGP_PROLONG_PC | MGP_PROLONG_LINEAR */
    int32_t coarse_init;   /* MGP_COARSE_FRESH | MGP_COARSE_WARM */
    int32_t coarse_bc;     /* MGP_BC_ZERO | _CONSISTENT | _FACE | _NEUMANN */
    int32_t coarse_sweeps; /* sweeps on a coarsest level with more than one cell */
    int32_t err_mode;      /* 1: psiOld snapshot + RMS update per cycle (cpu.lua:200-203); 0: off */
    int32_t device;        /* HIP device ordinal; -1 = current device */
    int32_t rank, world;   /* slab-z domain decomposition over `world` GPUs (3D only) */
    int32_t restriction;   /* MGP_RESTRICT_AVERAGE (reference) | MGP_RESTRICT_FULL_WEIGHTING */
    int64_t gather_cells;  /* a level with <= this many cells is replicated on every rank */
    uint8_t comm_id[MGP_COMM_ID_BYTES]; /* from mgp_comm_unique_id() on rank 0 (world > 1) */
    int32_t arith;         /* MGP_ARITH_REAL (gpu.lua) | MGP_ARITH_DOUBLE (cpu-raw.lua's real = 'float') */
    int32_t api_version;   /* MGP_API_VERSION of the header the caller was built with (mgp_opts_default sets it) */
} mgp_opts;
/* The layout is part of the ABI (LuaJIT cdef, ctypes mirror): a change must bump MGP_API_VERSION and append
 * fields, so that struct_size changes with it.  mgp_create rejects a struct_size or api_version that is not
 * this library's: fill the struct with the library's own mgp_opts_default before setting fields. */
#ifdef __cplusplus
static_assert(sizeof(mgp_opts) == 232, "mgp_opts layout changed");
#else
_Static_assert(sizeof(mgp_opts) == 232, "mgp_opts layout changed");
#endif

typedef struct mgp_ctx mgp_ctx;

int         mgp_version(void);
/* Defaults = the reference cpu.lua configuration: 2D, double, Jacobi 7+7, V, PC, fresh, zero. */
void        mgp_opts_default(mgp_opts* o);
/* RCCL unique id for a world > 1 context (call on rank 0, broadcast the bytes).  With the environment variable
 * MGP_TRANSPORT=rccl when it is created, a world-1 context (or a one-device group) takes the multi-GPU code
 * path on a one-rank RCCL communicator of its own (3D: its levels are "distributed" slabs without neighbours),
 * so that every RCCL call of a cycle executes on a one-GPU machine; results equal the plain world-1 run.
 * A context on its own RCCL communicator (one process per GPU, or MGP_TRANSPORT=rccl) waits for its streams under
 * a deadline, MGP_COMM_TIMEOUT_S seconds at creation (default 600, 0 = block): when it expires the call prints and
 * returns MGP_ERR_RCCL naming the rank and the first exchange / collective that has not completed (its level and
 * stream), after ncclCommAbort of the context's communicators; the context then refuses every exchange (destroy
 * it).  MGP_TEST_STALL=k (tests): the context's k-th halo exchange first holds its stream like an absent peer. */
int         mgp_comm_unique_id(void* out, int64_t nbytes);

/* Replaces MultigridCPU:init{size,...} (cpu.lua:173-194) / MultigridCPURaw:init(size, real)
 * (cpu-raw.lua:142-174) / MultigridGPU:init (gpu.lua:26-245): allocates the level hierarchy. */
int         mgp_create(mgp_ctx** out, const mgp_opts* o);
void        mgp_destroy(mgp_ctx* c);
const char* mgp_last_error(const mgp_ctx* c);

/* Level hierarchy.  info[0..7] = {nx, ny, nz_global, nz_local, z0, distributed, engine, exchanges}; engine =
 * how a cycle runs the level's smoothing phases: 0 one launch per piece, 1 inside the single-launch coarse
 * tail (LDS-resident levels), 2 temporally blocked z-streamed phases, 3 3D-tiled one-launch phases, 4 POST
 * temporally blocked, PRE one launch per piece or, where supported (fp32, 2^3-average restriction, one rank's whole
 * level, from a fresh guess; MGP_ZPOST_PRE=0: never), the stage-split temporally blocked PRE; exchanges =
 * halo exchanges (grouped send/recv with the z-neighbours) of this level so far on this rank. */
int         mgp_num_levels(const mgp_ctx* c);
int         mgp_level_info(const mgp_ctx* c, int level, int64_t info[8]);
/* The same plan without a device (host logic only): fills up to max_levels rows of 8 int64s. */
int         mgp_plan(const mgp_opts* o, int64_t* rows, int max_levels);

/* f = -1e6 at 0-based (n/2, n/2[, n/2]), psi = -f (cpu.lua:180-193, cpu-raw.lua:8-20, gpu.lua:41-59). */
int         mgp_init_point_charge(mgp_ctx* c);
/* Copy a level's field in/out (this rank's slab on distributed levels; count in elements).
 * Replaces direct access to mg.psi / mg.f (cpu.lua) and .psi.buffer / .f.buffer (cpu-raw.lua). */
int         mgp_set_field(mgp_ctx* c, int level, int which, const void* src, int64_t count, int mem);
int         mgp_get_field(const mgp_ctx* c, int level, int which, void* dst, int64_t count, int mem);

/* Plane ranges of a level's field: local planes [z_begin, z_begin + nz) of this rank's slab, nz * ny * nx
 * reals, x fastest.  Host transfers stream through a bounded staging buffer (~256 MiB), so fields
 * far larger than host-convenient (a 4096 x 4096 x 512 fp32 slab is 34 GB) can be read piecewise. */
int         mgp_set_planes(mgp_ctx* c, int level, int which, int64_t z_begin, int64_t nz, const void* src, int mem);
int         mgp_get_planes(const mgp_ctx* c, int level, int which, int64_t z_begin, int64_t nz, void* dst, int mem);
/* Device-side fingerprint of this rank's part of a field, for comparing runs that cannot come to the
 * host: *hash = sum mod 2^64 over cells of mix64(bits(x) ^ mix64(global lexicographic index)) (order-
 * and decomposition-independent: the ranks' hashes add up to the global one, and two fields hash
 * equal when they are bit-identical), stats = {sum x, sum x^2, max |x|} in fp64. */
int         mgp_field_stats(const mgp_ctx* c, int level, int which, uint64_t* hash, double stats[3]);

/* One outer iteration = MultigridCPU:step() (cpu.lua:196-206): psiOld = psi; one V/F-cycle from
 * the finest level with h = 1/n; *err_out = sqrt(sum (psi - psiOld)^2 / N) (NaN if err_mode 0). */
int         mgp_cycle(mgp_ctx* c, double* err_out);
/* k outer iterations back to back with one host synchronisation at the end (the loop of
 * MultigridCPURaw:run, cpu-raw.lua:245, without early exit); errs[k] may be NULL. */
int         mgp_cycles(mgp_ctx* c, int32_t k, double* errs);

/* MultigridCPURaw:twoGrid(h, u, f, L) (cpu-raw.lua:186; gpu.lua:296): one cycle from the level of
 * size L with spacing h on caller buffers of L^dim reals (mem = MGP_MEM_HOST | MGP_MEM_DEVICE);
 * u is updated in place, f is read only.  The level's own u / f (on the finest size the solver's psi and f) and
 * psiOld of the last outer iteration (mgp_metrics, MGP_FIELD_PSI_OLD / _ERROR) are unchanged on every engine; the
 * levels below are the cycle's scratch (rs, Rs, vs, Vs) and do change.  Single-GPU contexts only. */
int         mgp_two_grid(mgp_ctx* c, double h, void* u, const void* f, int64_t L, int mem);

/* Level-granular pieces of twoGrid (cpu-raw.lua:198-236), for hybrid hand-off (cpu-gpu.lua:17-52)
 * and kernel-level tests.  h of level l is 2^l / n[0]. */
int         mgp_smooth(mgp_ctx* c, int level, int sweeps);          /* inPlaceIterativeSolver x sweeps */
int         mgp_residual_restrict(mgp_ctx* c, int level);           /* calcResidual + reduceResidual -> f of level+1 */
int         mgp_prolong_correct(mgp_ctx* c, int level);             /* expandResidual + addTo from level+1 */
int         mgp_coarse_solve(mgp_ctx* c);                           /* L == 1 branch of twoGrid */

int         mgp_sync(mgp_ctx* c);

/* Coarse-engine switch, the MI355X form of cpu-gpu.lua's cpuDepth (cpu-gpu.lua:61): the levels of
 * nx <= size run as ONE launch of the LDS-resident coarse engine (levels of <= 4096 cells by
 * default).  size 0 turns the engine off.  MGP_ERR_ARG if that sub-hierarchy does not fit one
 * workgroup's LDS. */
int         mgp_set_coarse_level(mgp_ctx* c, int64_t size);
/* Hybrid hand-off (cpu-gpu.lua:17-52).  When the cycle reaches the level of nx = size it copies
 * that level's u and f to host buffers (lexicographic, size^dim reals), calls fn(user, h, u, f,
 * size), which runs the coarse cycle in place on u (e.g. the reference's MultigridCPURaw:twoGrid),
 * and copies u and f back.  fn returns 0 on success.  fn == NULL removes the hand-off.  Replicated
 * levels >= 1 only; hipGraph replay is off while a hand-off is set. */
typedef int (*mgp_coarse_fn)(void* user, double h, void* u, const void* f, int64_t size);
int         mgp_set_coarse_handoff(mgp_ctx* c, int64_t size, mgp_coarse_fn fn, void* user);

/* The reference's convergence metrics of the last outer iteration, on the device
 * (gpu.lua:173-200 calcRelErr / calcFrobErr, test-gpu-obj.lua:216-247 relErr / count / frobErr):
 * rel_err = mean of |1 - psi/psiOld| over the cells where it is nonzero, count = their number,
 * frob = sqrt(sum (psi - psiOld)^2 / N).  Needs err_mode 1. */
int         mgp_metrics(mgp_ctx* c, double* rel_err, int64_t* count, double* frob);

/* Residual norm of a level (north star: "wavefront-level reductions for the residual norm"):
 * *rnorm = ||f - A u||_2 with the level's operator (calcResidual, cpu.lua:108-123, never materialised),
 * *fnorm = ||f||_2; squares summed in fp64 per wave (butterfly), per workgroup and then in a fixed
 * order, all-reduced over the ranks on a distributed level.  Level 0 after a cycle gives the
 * converged relative residual ||r|| / ||f||. */
int         mgp_residual_norm(mgp_ctx* c, int level, double* rnorm, double* fnorm);

/* Removing a field's mean (build-defined; a plain field operation under every boundary).  MGP_BC_NEUMANN determines
 * psi up to a constant and needs sum f = 0: remove f's mean before the first cycle and psi's after the last one (the
 * cycle itself does not project, so err, psiOld and graph replay are those of the other boundaries).  which =
 * MGP_FIELD_U | MGP_FIELD_F of any level.  S = the fp64 sum of the field's cells in a fixed order (per wave, per
 * workgroup, then fixed; all-reduced over the ranks on a distributed level: mgp_field_stats' and mgp_residual_norm's
 * scheme), m = S / N in double over the level's N global cells, every cell becomes RN((double)x - m), *mean = m
 * (mean may be NULL).  One reduction pass and one 16-byte streaming pass on the packed layout; pad cells and ghost
 * planes do not enter the sum.  Afterwards the field counts as written (its ghost planes are exchanged again on a
 * slab level), and on level 0 psiOld and the metrics are invalid until the next outer iteration (mgp_metrics,
 * MGP_FIELD_PSI_OLD / _ERROR: MGP_ERR_STATE).  While refinement is active level 0 is refused (MGP_ERR_STATE): use
 * mgp_refine_remove_mean. */
int         mgp_remove_mean(mgp_ctx* c, int level, int which, double* mean);

/* Full multigrid start (FMG, nested iteration; build-defined, no reference counterpart).  mgp_fmg reads level 0's f,
 * ignores the stored psi, and
 *   1. restricts f down the hierarchy (f of l+1 = R f of l, l = 0 .. last-1);
 *   2. zeroes the coarsest u and runs the coarse solve (mgp_coarse_solve's sweeps);
 *   3. for l = last-1 .. 1: u of l = P3 u of l+1; u of l+1 = 0 (under both coarse_init values); cycles_per_level >= 1
 *      cycles of the context's kind (V / F) from level l with h = 2^l / n[0], on the engines the cycle runs there;
 *   4. the same onto level 0: psi = P3 u of 1, u of 1 = 0;
 *   5. final_cycles >= 0 ordinary outer iterations (mgp_cycles' path: graph replay, fused err, psiOld), errs
 *      [final_cycles] as mgp_cycles returns them (may be NULL).
 * One host synchronisation, at the end.  A cycle from level l writes no f at level l or above, so every level's
 * restricted f is intact when the ascent arrives there.  With final_cycles = 0, psiOld and the metrics are invalid
 * until the next outer iteration (mgp_metrics, MGP_FIELD_PSI_OLD / _ERROR: MGP_ERR_STATE, as after mgp_remove_mean).
 *
 * Arithmetic: every expression in the field's real type T, each operation rounded, no contraction.
 * R is the context's `restriction` applied to f itself: the 2^d average in reduceResidual's term order
 *     R = 1/8 (((((((f000 + f100) + f010) + f110) + f001) + f101) + f011) + f111)      (x fastest; 2D: 1/4 of four)
 * or the full weighting with face weight 3 - c_{l+1} (the restriction mgp_residual_restrict applies to the residual).
 * P3 REPLACES every cell of u (it does not add).  It is separable, one pass per active axis in the order x, y, z, each
 * on the result of the pass before (2D: z is not touched).  Along one axis the coarse line A[0 .. m) is extended by two
 * ghosts per side, mc = -(T)c_{l+1} (c: the boundary coefficient of coarse_bc, mgp_level_info):
 *     E[-1] = mc E[0],  E[-2] = mc E[1],  E[m] = mc E[m-1],  E[m+1] = mc E[m-2]
 *     (m = 1: E[-1] = E[1] = mc A[0], E[-2] = E[2] = mc (mc A[0])).
 * Each ghost is one multiplication, always performed; the ghost lines of the y and z passes are mc times the already
 * x- (x, y-) interpolated in-box line.  The two children of coarse cell I are
 *     child 2I     = ((wp E[I] + wn E[I-1]) + wq E[I+1]) + wr E[I-2]
 *     child 2I + 1 = ((wp E[I] + wn E[I+1]) + wq E[I-1]) + wr E[I+2]
 * with wp = 105/128, wn = 35/128, wq = -7/128, wr = -5/128: the cubic Lagrange weights at -+1/4 of a coarse cell.
 * Under MGP_BC_FACE / _NEUMANN / _CONSISTENT one cycle per level and one final cycle leave an algebraic error below
 * the discretisation error on smooth problems; under MGP_BC_ZERO the coarse operators are inconsistent with level 0
 * (the known mismatch) and no accuracy is claimed.
 *
 * The pieces (for tests and hybrid drivers) synchronise like mgp_residual_restrict: mgp_fmg_restrict_rhs writes f of
 * level + 1 from f of level; mgp_fmg_prolong writes u of level from u of level + 1 (on level 0 psiOld and the metrics
 * become invalid).  Under mgp_set_debug(1) every piece's output is checked and named like the cycle's phases.
 *
 * Refused: NULL context, bad level, cycles_per_level < 1, final_cycles < 0, an MGP_ARITH_DOUBLE context: MGP_ERR_ARG;
 * world > 1, loopback and group ranks, MGP_TRANSPORT=rccl ("single-GPU contexts only"), active refinement, and (mgp_fmg)
 * a coarse hand-off: MGP_ERR_STATE.  Limits: no slab or group contexts (the cubic stencil needs a second coarse ghost
 * plane), no mixed-precision refinement, the ascent is not captured in a hipGraph (only the final outer iterations
 * replay one), and the ascent runs the levels of the LDS coarse engine with its launches, not inside it (a batch,
 * mgp_batch_fmg, does both: one captured ascent whose LDS levels are one launch). */
int         mgp_fmg_restrict_rhs(mgp_ctx* c, int level);   /* f of level+1 = R f of level */
int         mgp_fmg_prolong(mgp_ctx* c, int level);        /* u of level = P3 u of level+1 (replaces u) */
int         mgp_fmg(mgp_ctx* c, int32_t cycles_per_level, int32_t final_cycles, double* errs);

/* MAC-grid pressure projection (build-defined, no reference counterpart): the divergence D of a staggered vector field
 * into level 0's f, the gradient G of level 0's psi onto the faces, and the one-call composition v <- v - G A^-1 D v
 * (incompressible flow's pressure projection, MHD's divergence cleaning).  Both operators are single fused passes on
 * the packed layout.
 *
 * Level 0 has nx x ny x nz cells (2D: nz = 1).  T is the context's real type and ih = (T)n[0] (= 1/h, a power of two);
 * every operation is rounded in T, with no contraction.
 * Face arrays are lexicographic, x fastest and contiguous, owned by the caller, in host or device memory (mem; e.g. a
 * PyTorch tensor's data_ptr()), and must not overlap:
 *     vx[k][j][i], i in [0, nx]: the x face between cells i-1 and i; (nx+1) ny nz reals
 *     vy[k][j][i], j in [0, ny]: nx (ny+1) nz reals
 *     vz[k][j][i], k in [0, nz]: nx ny (nz+1) reals; 3D only, ignored (may be NULL) in 2D
 * Divergence D writes level 0's f:
 *     f[i,j,k] = (((vx[i+1] - vx[i]) + (vy[j+1] - vy[j])) + (vz[k+1] - vz[k])) ih     (2D: without the z term)
 * Gradient G, per axis, on the line of psi extended by one ghost per side: mc = -(T)c_0, c_0 level 0's boundary
 * coefficient (0 zero / consistent, +1 face, -1 Neumann; mgp_level_info);
 *     E[-1] = mc psi[0],  E[n] = mc psi[n-1]     (one multiplication each, always performed)
 *     g(face i) = (E[i] - E[i-1]) ih,  i in [0, n]
 * and a one-cell axis takes both ghosts from its one cell.  op = MGP_GRAD_STORE: the arrays receive g;
 * MGP_GRAD_SUBTRACT: every face becomes v - g.  So under Neumann a wall face has g = +0 and keeps its bits (a -0 stays
 * -0), under face Dirichlet the wall gradient is 2 psi / h, and in exact arithmetic D(v - G psi) = f - A psi with A the
 * level-0 operator (diagonal (-2 dim - nb c_0) / h^2): the projected field is divergence-free to the solver's residual.
 *
 * mgp_divergence: its state effects are those of mgp_set_field(c, 0, MGP_FIELD_F, ...): psi, psiOld and the metrics
 * are untouched; pad slots and ghost planes of f are not written.
 * mgp_gradient reads the psi that mgp_get_field(c, 0, MGP_FIELD_U, ...) returns and changes nothing in the context.
 * mgp_project, with one host synchronisation at the end:
 *   1. f = D v;
 *   2. under MGP_BC_NEUMANN, f's mean is removed (mgp_remove_mean's arithmetic and state effects);
 *   3. fmg_cycles >= 1: mgp_fmg(fmg_cycles, cycles); otherwise cycles >= 0 ordinary outer iterations from the stored
 *      psi (the warm start from the last time step; cycles = 0 leaves psi as stored);
 *   4. v -= G psi.
 * norms (may be NULL: the pass is skipped) receives {||f||_2, ||f - A psi||_2}, computed like mgp_residual_norm: the
 * field's divergence norm before the projection and, by the identity, after it.  psi's mean is not removed: G does not
 * see it.
 * Host memory: the arrays go through device buffers allocated for the call (MGP_ERR_OOM if that fails, nothing stays
 * allocated); device memory is the hot path.  Under mgp_set_debug(c, 1) f after mgp_divergence and the faces after
 * mgp_gradient are scanned: "found a nan: mgp_divergence" / "found a nan: mgp_gradient, axis a" (MGP_ERR_STATE).
 *
 * Refused: NULL context, NULL vx or vy (vz in 3D), unknown mem or op, fmg_cycles < 0 or cycles < 0, an
 * MGP_ARITH_DOUBLE context: MGP_ERR_ARG; world > 1, loopback and group ranks, MGP_TRANSPORT=rccl ("single-GPU contexts
 * only") and active refinement: MGP_ERR_STATE; mgp_project with fmg_cycles >= 1: also whatever mgp_fmg refuses.
 * Limits: no batches (mgp_batch_*) through these three entry points: a batch has its own, mgp_batch_divergence,
 * mgp_batch_gradient and mgp_batch_project below, with the same definitions per member; no slab or group contexts, no
 * mixed-precision refinement (real = 'mixed'), no cell-centred vector fields, and the wall value of the pressure is
 * zero (face Dirichlet).  Variable density: mgp_set_coefficients below (a context, not a batch). */
enum { MGP_GRAD_STORE = 0, MGP_GRAD_SUBTRACT = 1 };
int         mgp_divergence(mgp_ctx* c, const void* vx, const void* vy, const void* vz, int mem);
int         mgp_gradient(mgp_ctx* c, int op, void* vx, void* vy, void* vz, int mem);
int         mgp_project(mgp_ctx* c, void* vx, void* vy, void* vz, int mem, int32_t fmg_cycles, int32_t cycles,
                        double norms[2]);

/* Variable coefficients: div(beta grad psi) = f with positive coefficients beta on the cell faces (a two-phase or
 * stratified flow's pressure equation div((dt / rho) grad p) = div v, electrostatics with a permittivity, Darcy flow).
 * While a context has coefficients, every level of its cycle runs one launch per piece on kernels of their own
 * (mgp_vc.hip), and the pieces, the norms and the projection use A_beta u = div(beta grad u).  A context that never
 * sets coefficients is unchanged, and mgp_clear_coefficients returns a context to its engines and its bits.
 *
 * Definition.  T is the context's real type; every operation is rounded in T, without contraction.
 * Face arrays: mgp_divergence's layout, one set per level l with that level's nx, ny, nz: bx[k][j][i], i in [0, nx], is
 * beta on the x face between cells i - 1 and i; by has j in [0, ny]; bz has k in [0, nz] (3D only).
 * Coarse coefficients: all axes halve together, as the hierarchy does.  A coarse face takes the arithmetic mean of the
 * 2^(d-1) fine faces that tile it, the lower tangential axis fastest: the 3D x face (I, J, K) is
 *   (((b(2I,2J,2K) + b(2I,2J+1,2K)) + b(2I,2J,2K+1)) + b(2I,2J+1,2K+1)) * (T)0.25,
 * y faces over (x, z) and z faces over (x, y) in the same way; 2D: (b0 + b1) * (T)0.5.
 * Operator: for cell (i, j, k) of level l, with its six face coefficients bxl, bxr, byl, byr, bzl, bzr (lower and upper
 * face per axis), its neighbours' values xl .. zr (an out-of-box neighbour is the value +0), inv_hSq = 1 / h_l^2 (exact)
 * and c = (T)c_l, the boundary coefficient of the level under the context's coarse_bc (all four values):
 *   s      = ((((bxl xl + bxr xr) + byl yl) + byr yr) + bzl zl) + bzr zr       (2D: the first four terms)
 *   S_all  = ((((bxl + bxr) + byl) + byr) + bzl) + bzr
 *   S_wall = the same sum in the same order with every face that is not on the box replaced by +0
 *   dg     = ((-S_all) - c S_wall) / hSq
 *   relax:    a = f - s inv_hSq;  u = (dg == 0) ? +0 : RN(a / dg)     (IEEE division)
 *   residual: r = f - (s inv_hSq + dg u)
 * With beta = 1 everywhere this is the constant operator's arithmetic term for term (dg = ((T)(-2 dim) - nb c) / hSq), so
 * a context with all-ones coefficients gives the constant context's bits under every boundary; the one-cell Neumann
 * level has dg = 0 and relaxes to +0.  Restriction (the 2^d average in reduceResidual's order) and prolongation
 * (piecewise constant or (tri)linear) are the constant cycle's kernels: they do not see beta.  Smoothing is red/black
 * Gauss-Seidel with nu1 / nu2; V and F cycles, fresh and warm guesses and coarse_sweeps all apply; err / psiOld as in
 * the per-piece cycle.
 * Gradient with coefficients: g as defined for mgp_gradient; MGP_GRAD_STORE writes beta_face g, MGP_GRAD_SUBTRACT
 * v - (beta_face g), the product rounded first.  In exact arithmetic D (v - beta G psi) = f - A_beta psi, wall faces
 * included (their term is beta_w (1 + c_0) psi / h^2), so mgp_project with fmg_cycles = 0 is the variable-density
 * projection and its norms are {||f||, ||f - A_beta psi||}.  mgp_divergence is unchanged.
 *
 * mgp_set_coefficients reads level 0's faces from host or device memory (bz is ignored in 2D), checks on the device
 * that every value is finite and > 0 (otherwise MGP_ERR_ARG, "coefficient not positive and finite: axis a", and the
 * context is exactly as before the call: earlier coefficients, if any, stay in force), builds every level's coefficients
 * (one launch per level and axis), drops the captured cycle graphs (re-captured on first use) and synchronises once.
 * MGP_ERR_OOM leaves the context unchanged.  Setting again replaces the coefficients.  mgp_get_coefficients returns
 * any level's array of `axis` (0 x, 1 y, 2 z) in the face layout; count = its number of reals; MGP_ERR_STATE when none
 * are set.  While coefficients are set mgp_level_info reports engine 0 on every level, and mgp_cycle(s), mgp_smooth,
 * mgp_residual_restrict, mgp_prolong_correct, mgp_coarse_solve, mgp_residual_norm, mgp_get_field(MGP_FIELD_RESIDUAL /
 * _CORRECTION), mgp_metrics, mgp_remove_mean (unchanged: A_beta keeps the constant null space, so Neumann still needs
 * sum f = 0) and mgp_set_debug follow beta.
 * Refused by mgp_set_coefficients, MGP_ERR_ARG: an MGP_ARITH_DOUBLE context, a smoother other than MGP_RBGS,
 * MGP_RESTRICT_FULL_WEIGHTING, a NULL array, an unknown mem; MGP_ERR_STATE: world > 1, loopback and group ranks,
 * MGP_TRANSPORT=rccl ("single-GPU contexts only"), active refinement, a coarse hand-off that is set.  Refused with
 * MGP_ERR_STATE while coefficients are set: mgp_two_grid, mgp_cg_solve, mgp_fmg, mgp_fmg_restrict_rhs, mgp_fmg_prolong,
 * mgp_project with fmg_cycles >= 1 (before f is written), mgp_refine_begin, mgp_set_coarse_handoff with a function,
 * mgp_set_coarse_level with size > 0.
 * Limits: no batches, slabs, full multigrid start, refinement, Jacobi or lexicographic Gauss-Seidel with coefficients.
 * Sharp coefficient jumps slow the plain cycle down (the README has figures); a Krylov wrapper is future work. */
int         mgp_set_coefficients(mgp_ctx* c, const void* bx, const void* by, const void* bz, int mem);
int         mgp_clear_coefficients(mgp_ctx* c);
int         mgp_has_coefficients(const mgp_ctx* c);                 /* 0 / 1 */
int         mgp_get_coefficients(const mgp_ctx* c, int level, int axis, void* dst, int64_t count, int mem);

/* The reference's Krylov cross-check (test/converge-multigrid-vs-krylov.lua:38-69, solver.conjgrad) on
 * the device, as an independent second oracle for the converged multigrid answer: matrix-free
 * conjugate gradients on the finest level's operator (same 5-/7-point stencil and box boundary) from
 * x0 = -f with b = f, fp64 dot products, stopping when rSq / bSq < epsilon or after maxiter
 * iterations.  The solution goes to x_out (level-0 cells, x fastest; may be NULL); linf_hist (maxiter
 * doubles, may be NULL) gets |x|_inf after every iteration, the quantity the reference plots.  The
 * solver's own psi / f are not changed.  Single-GPU contexts only. */
int         mgp_cg_solve(mgp_ctx* c, double epsilon, int32_t maxiter, void* x_out, int mem, int32_t* iters,
                         double* err, double* linf_hist);

/* Mixed-precision defect correction (iterative refinement): the outer loop of cpu.lua:196-216 with real = 'double'
 * — fp64 psi and f, err = sqrt(sum (psi - psiOld)^2 / N) in double — around the fp32 cycles of a real_bytes = 4,
 * MGP_ARITH_REAL context.  One outer step: r = f - A psi in double (calcResidual, cpu.lua:108-123, on the fp64
 * fields), narrowed to float into level 0's f; `inner` ordinary cycles of the context on A e = r from e = 0 in
 * level 0's u; psi += (double)e.  The fp32 hierarchy, its engines and their bit-exactness are unchanged; no
 * reference counterpart for the split itself (build-defined).  Limits: r is not rescaled before it is narrowed, so a
 * right-hand side whose defect leaves float's normal range is out of scope; one GPU only.  Measured time to
 * ||r|| / ||f|| <= 1e-12 against a real_bytes = 8 context (tools/refine_time.py, profiles/refine_time.json, one
 * MI355X): 3D 512^3 0.75 / 0.79 / 0.81 of the double time with inner = 2 / 4 / 6; 2D 4096^2 0.89 / 1.27 / 1.77.
 *
 * mgp_refine_begin allocates the fp64 psi / f (level 0's shape) and fills them with the exact widening of level 0's
 * current u / f.  MGP_ERR_ARG for real_bytes = 8 or MGP_ARITH_DOUBLE; MGP_ERR_STATE for world > 1, a loopback
 * context, a group's rank context, MGP_TRANSPORT=rccl, or when already active; MGP_ERR_OOM leaves the context as it
 * was.  While active, level 0's fp32 f / u are the scratch of the inner solve (mgp_get_field returns the last
 * narrowed defect / the last correction e); mgp_cycle, mgp_cycles, mgp_two_grid, mgp_metrics, mgp_cg_solve,
 * level-0 mgp_set_field / mgp_set_planes and reads of MGP_FIELD_PSI_OLD / _ERROR (the outer iteration is the fp64
 * one, whose psiOld is not stored; after mgp_refine_end they need a new outer iteration) return MGP_ERR_STATE;
 * mgp_init_point_charge also sets the fp64 fields.
 * mgp_refine_end stores the round-to-nearest narrowing of psi / f into level 0's u / f and frees the fp64 fields
 * (mgp_destroy frees them as well): an ordinary fp32 context again.  Every mgp_refine_* call but begin returns
 * MGP_ERR_STATE while refinement is not active. */
enum { MGP_REFINE_PSI = 0, MGP_REFINE_F = 1 };
int         mgp_refine_begin(mgp_ctx* c);
int         mgp_refine_end(mgp_ctx* c);
/* mg.psi / mg.f of the double solver (cpu.lua:179-193): the whole fp64 field, x fastest; count = level 0's cells;
 * host or device memory, through the bounded staging buffer. */
int         mgp_refine_set(mgp_ctx* c, int which, const double* src, int64_t count, int mem);
int         mgp_refine_get(const mgp_ctx* c, int which, double* dst, int64_t count, int mem);
/* mgp_remove_mean of the fp64 psi (MGP_REFINE_PSI) or f (MGP_REFINE_F). */
int         mgp_refine_remove_mean(mgp_ctx* c, int which, double* mean);
/* *rnorm = ||f - A psi||_2, *fnorm = ||f||_2 of the fp64 fields (fp64 sums: per wave, per workgroup, fixed order);
 * psi is not changed (level 0's fp32 f receives the narrowed defect). */
int         mgp_refine_residual(mgp_ctx* c, double* rnorm, double* fnorm);
/* One outer step = MultigridCPU:step() (cpu.lua:196-206) of the double solver with `inner` >= 1 fp32 cycles in place
 * of its one twoGrid: the defect from a zero guess, the cycles (the path mgp_cycles takes: graph replay, or eager
 * under mgp_timing / mgp_set_debug / a hand-off; their own errs are discarded), the add; one host synchronisation.
 * *rnorm / *fnorm: of the defect, i.e. before this step's correction; *err = sqrt(sum e^2 / N) (cpu.lua:203: psi -
 * psiOld is e).  With mgp_set_debug(1) the narrowed defect and every phase of the cycles are scanned: a NaN or inf
 * in the fp64 fields fails the step with "found a nan" (MGP_ERR_STATE). */
int         mgp_refine_step(mgp_ctx* c, int32_t inner, double* rnorm, double* fnorm, double* err);
/* MultigridCPU:solve() (cpu.lua:208-216) over that step: computes the defect and stops when rnorm <= rtol * fnorm
 * (checked before any cycle is spent), when a step's err < epsilon, when a norm or err is not finite, or after
 * maxouter steps.  rel_hist (maxouter + 1 doubles, may be NULL): rnorm / fnorm of every defect computed; err_hist
 * (maxouter doubles, may be NULL): each step's err; *steps: steps done. */
int         mgp_refine_solve(mgp_ctx* c, int32_t inner, double rtol, double epsilon, int32_t maxouter,
                             int32_t* steps, double* rel_hist, double* err_hist);

/* Loopback transport (tests only): the `world` ranks of a slab decomposition as contexts of ONE
 * process on one GPU, each driven by its own host thread.  Halo exchanges, the all-gather and the
 * err all-reduce become device copies ordered by events and a host barrier instead of RCCL calls;
 * everything else runs the multi-GPU code path unchanged.  A rank that stops calling makes the
 * others fail with MGP_ERR_STATE after 120 s instead of hanging. */
typedef struct mgp_loopback mgp_loopback;
int         mgp_loopback_create(mgp_loopback** out, int world);
void        mgp_loopback_destroy(mgp_loopback* lb);
int         mgp_create_loopback(mgp_ctx** out, const mgp_opts* o, mgp_loopback* lb);
/* Single-process multi-GPU group (the form of cpu-gpu.lua:55-72's one host object
 * owning several engines): ONE host process drives `ngpu` GPUs of the node.  The library creates
 * the RCCL communicators with ncclCommInitAll over devices[0..ngpu) (NULL = 0..ngpu-1) and one
 * context per rank (rank r = z-slab r of the box, opts->rank / opts->world / opts->device are set
 * by the group); every group call runs the ranks' work in one host thread per device inside the
 * library and returns when all are done.  When all devices[] are equal the ranks share that GPU
 * through the loopback transport (tests).  Field I/O is in the global x-fastest layout. */
typedef struct mgp_group mgp_group;
int         mgp_group_create(mgp_group** out, const mgp_opts* o, int ngpu, const int* devices);
void        mgp_group_destroy(mgp_group* g);
const char* mgp_group_last_error(const mgp_group* g);
int         mgp_group_size(const mgp_group* g);
mgp_ctx*    mgp_group_rank(mgp_group* g, int rank);   /* per-rank context (its slab, its stream) */
int         mgp_group_init_point_charge(mgp_group* g);
int         mgp_group_cycle(mgp_group* g, double* err_out);
int         mgp_group_cycles(mgp_group* g, int32_t k, double* errs);
int         mgp_group_set_field(mgp_group* g, int level, int which, const void* src, int64_t count, int mem);
int         mgp_group_get_field(mgp_group* g, int level, int which, void* dst, int64_t count, int mem);
int         mgp_group_residual_norm(mgp_group* g, int level, double* rnorm, double* fnorm);
int         mgp_group_field_stats(mgp_group* g, int level, int which, uint64_t* hash, double stats[3]);
int         mgp_group_remove_mean(mgp_group* g, int level, int which, double* mean);   /* mgp_remove_mean on every rank */

/* Batched solves (build-defined; the reference solves one box): B independent members of ONE shape in one
 * hierarchy on one GPU.  Every kernel of a cycle covers all members in one launch (the launches per cycle do not
 * depend on B), and in mgp_batch_solve each member stops on its own.  Per member the cycle and the outer loop are
 * the ordinary context's (cpu.lua:70-165, 196-216): a member's psi equals mgp_cycles' bit for bit.  The levels of
 * <= 4096 cells run as one launch with one workgroup per member from LDS (engine 1), the levels above one launch
 * per piece (engine 0).  A batch owns one stream and replays ONE captured cycle (MGP_GRAPH=0: eager launches,
 * identical results); it is not thread-safe.
 * Options (`o` describes one member): dim 2 / 3, power-of-two axes, real_bytes 4 / 8 with MGP_ARITH_REAL, MGP_JACOBI
 * or MGP_RBGS, V / F, both prolongations, fresh / warm, every coarse_bc, coarse_sweeps, err_mode 0 / 1.
 * MGP_ERR_ARG naming the field, before any device call: batch < 1, world != 1, MGP_GS_LEX, MGP_ARITH_DOUBLE,
 * MGP_RESTRICT_FULL_WEIGHTING, a member (n) of more than 2^24 level-0 cells (one such box fills the GPU: use
 * mgp_create), batch * cells >= 2^31.  MGP_ERR_OOM leaves nothing allocated.
 * Measured (tools/batch_time.py, profiles/batch_time.json): README "Many small boxes at once". */
typedef struct mgp_batch mgp_batch;
int         mgp_batch_create(mgp_batch** out, const mgp_opts* o, int32_t batch);
void        mgp_batch_destroy(mgp_batch* b);
/* The message of the last failed call on b; b == NULL: of the failed mgp_batch_create / mgp_batch_plan. */
const char* mgp_batch_last_error(const mgp_batch* b);
int         mgp_batch_size(const mgp_batch* b);
/* The member hierarchy without a device (host logic only), validated like mgp_batch_create: up to max_levels rows
 * of 8 int64 in mgp_plan's columns {nx, ny, nz, nz, 0, 0, engine, 0}, engine 0 = one launch per piece, 1 = the
 * LDS engine.  Returns the number of levels; the rows do not depend on batch. */
int         mgp_batch_plan(const mgp_opts* o, int32_t batch, int64_t* rows, int max_levels);
/* mgp_init_point_charge on every member. */
int         mgp_batch_init_point_charge(mgp_batch* b);
/* Copy a level's field in / out.  member >= 0: one member, count = the level's cells; member == -1: all members,
 * count = B * cells, member slowest, then x fastest as everywhere.  which: MGP_FIELD_U / MGP_FIELD_F on any level;
 * on level 0 also MGP_FIELD_PSI_OLD (get only, err_mode 1; MGP_ERR_STATE otherwise).  mem: MGP_MEM_HOST |
 * MGP_MEM_DEVICE (e.g. a PyTorch tensor's data_ptr()). */
int         mgp_batch_set_field(mgp_batch* b, int member, int level, int which, const void* src, int64_t count, int mem);
int         mgp_batch_get_field(const mgp_batch* b, int member, int level, int which, void* dst, int64_t count, int mem);
/* k outer iterations (mgp_cycles) of EVERY member with one host synchronisation (one per 2^20 / B cycles);
 * errs (may be NULL): k * B doubles, errs[it * B + m] (NaN with err_mode 0). */
int         mgp_batch_cycles(mgp_batch* b, int32_t k, double* errs);
/* MultigridCPU:solve() (cpu.lua:208-216) per member: member m stops after the first iteration whose err < epsilon
 * or is not finite, or after maxiter; a stopped member's fields are not touched again (every kernel of the later
 * cycles returns at once for it).  The stop state lives on the device; the host enqueues cycles in chunks that
 * never pass maxiter and reads the number of active members after each.  iters[B], last_err[B] (either may be
 * NULL).  MGP_ERR_STATE with err_mode 0. */
int         mgp_batch_solve(mgp_batch* b, double epsilon, int32_t maxiter, int32_t* iters, double* last_err);
/* Per member mgp_residual_norm of level 0: rnorm[m] = ||f - A u||_2, fnorm[m] = ||f||_2 (fp64 sums: per wave,
 * per workgroup, then in a fixed order); either may be NULL. */
int         mgp_batch_residual_norm(mgp_batch* b, double* rnorm, double* fnorm);
/* mgp_remove_mean per member (stopped members included): means[B] (may be NULL); each member's sum per wave, then
 * per workgroup in a fixed order. */
int         mgp_batch_remove_mean(mgp_batch* b, int level, int which, double* means);
/* Kernel launches (graph nodes included) one cycle of the last mgp_batch_cycles / mgp_batch_solve enqueued. */
int         mgp_batch_launches(const mgp_batch* b, int64_t* per_cycle);
/* Full multigrid start of EVERY member: per member mgp_batch_fmg is mgp_fmg's definition above (steps 1-5) with the same
 * arithmetic (every operation rounded in the real type, no contraction; R the 2^d average in reduceResidual's term order;
 * P3 with the ghost rule mc = -(T)c_{l+1}, the weights 105, 35, -7, -5 over 128 and the pass order x, y, z; the level
 * below set to a real zero after each P3 under both coarse_init values), so a member's u and f on every level equal,
 * bit for bit, what mgp_fmg leaves on an ordinary context with that member's f.  The stored psi is ignored: no u of any
 * level is read before the call has written it.  All members are armed as mgp_batch_cycles arms them (a stop state
 * left by mgp_batch_solve excludes nobody); errs (may be NULL): final_cycles * B doubles, errs[it * B + m] (NaN with
 * err_mode 0).  One host synchronisation, at the end, in every call after the first use of a cycles_per_level value;
 * that first use also builds and uploads the LDS program and captures the ascent's graph (blocking copies, one more
 * synchronisation).
 * Engines: the restrictions of f down to the first LDS level T run one launch per level; the levels from T down are ONE
 * launch with one workgroup per member (the restriction of f from T, the coarse solve, every P3 and every per-level
 * cycle, all in LDS; only level T's f is read from memory); the levels above run one launch per piece, the P3 onto a
 * level whose coarse rows hold 16 bytes of reals in mgp_fmg's marching vector form over all members.  The ascent is one
 * captured graph (a single chain, kept for the last cycles_per_level; MGP_GRAPH=0: eager launches, identical bits);
 * the final iterations replay the cycle's graph.  The LDS program's length grows with cycles_per_level; it lives in a
 * device array of its own, built on the first use of a cycles_per_level value and kept for the last one.  A program of
 * more than 4096 ops (cycles_per_level <= 2 never is) runs the LDS levels' ascent per piece as well, with identical
 * bits.  MGP_TAIL=0: every level per piece.
 * After final_cycles = 0 (and after mgp_batch_fmg_prolong onto level 0) psiOld describes an iterate that is gone: a
 * read of MGP_FIELD_PSI_OLD returns MGP_ERR_STATE until the next outer iteration, as on the ordinary context.
 * The two pieces run on every member (stopped ones included) and synchronise like mgp_batch_remove_mean.
 * mgp_batch_fmg_launches: the kernel launches (graph nodes included) of the last call's ascent, without the final outer
 * iterations; it does not depend on B.
 * MGP_ERR_ARG: NULL batch, a level outside [0, levels - 2], cycles_per_level < 1, final_cycles < 0.  Out of scope: slab
 * and group contexts, mixed-precision refinement, the full weighting (batches refuse it), a per-member stop inside the
 * ascent.  Measured (tools/batch_fmg_time.py, profiles/batch_fmg_time.json): README "Many small boxes at once". */
int         mgp_batch_fmg_restrict_rhs(mgp_batch* b, int level);  /* every member: f of level+1 = R f of level */
int         mgp_batch_fmg_prolong(mgp_batch* b, int level);       /* every member: u of level = P3 u of level+1 (replaces u) */
int         mgp_batch_fmg(mgp_batch* b, int32_t cycles_per_level, int32_t final_cycles, double* errs);
int         mgp_batch_fmg_launches(const mgp_batch* b, int64_t* ascent);
/* MAC-grid projection of the members: per member the definitions are those of mgp_divergence / mgp_gradient /
 * mgp_project above (the same term order, every operation rounded in the real type T with no contraction, ih = (T)n[0],
 * mc = -(T)c_0 with c_0 the level-0 boundary coefficient of the batch's coarse_bc, each ghost one multiplication that is
 * always performed, a one-cell axis taking both ghosts from its one cell), so a member's f after mgp_batch_divergence
 * and its faces after mgp_batch_gradient equal, bit for bit, what an ordinary context of the member's shape produces
 * from the member's data.
 * Face arrays: member slowest, then exactly the ordinary layout: vx[m][k][j][i] with (nx+1) ny nz reals per member, vy
 * nx (ny+1) nz, vz nx ny (nz+1) (3D only; ignored and may be NULL in 2D); contiguous, owned by the caller, in host or
 * device memory (mem), not overlapping.  member as in mgp_batch_set_field: >= 0 addresses one member and the arrays
 * hold that member's faces, -1 all B members.  Host arrays go through device buffers allocated for the call
 * (MGP_ERR_OOM if that fails, nothing stays allocated); device memory is the hot path.
 * Each operator is ONE launch for any B and any member argument: its work is the flat list members x items (an item: 16
 * bytes of each colour of a row, or one cell where rows are shorter than that or a pointer or member stride is not
 * 16-byte aligned), so no workgroup is tied to one member and small members fill their workgroups.
 * mgp_batch_divergence has the state effects of mgp_batch_set_field(member, 0, MGP_FIELD_F, ...): psi, psiOld and the
 * stop state are untouched.  mgp_batch_gradient (op: MGP_GRAD_STORE / MGP_GRAD_SUBTRACT) reads the psi that
 * mgp_batch_get_field(member, 0, MGP_FIELD_U, ...) returns and changes nothing in the batch.  Both act on stopped
 * members too, as mgp_batch_remove_mean does, and synchronise once before returning.
 * mgp_batch_project acts on all members, with one host synchronisation at the end (the first use of an fmg_cycles value
 * adds the one mgp_batch_fmg documents):
 *   1. f = D v on every member;
 *   2. under MGP_BC_NEUMANN every member's f loses its own mean (mgp_batch_remove_mean's kernels and arithmetic);
 *   3. fmg_cycles >= 1: mgp_batch_fmg(fmg_cycles, cycles)'s path (the captured ascent, the final iterations replaying
 *      the cycle's graph, psiOld invalid after cycles = 0 as there); otherwise cycles >= 0 outer iterations from the
 *      stored psi, mgp_batch_cycles' path (fmg_cycles = 0 and cycles = 0: psi stays as stored).  All members are armed:
 *      a stop state left by mgp_batch_solve excludes nobody;
 *   4. v -= G psi on every member.
 * div_before / div_after (B doubles each; either may be NULL, both NULL skips the pass): ||f||_2 and ||f - A psi||_2
 * per member, with the bits mgp_batch_residual_norm returns at that point (under Neumann "before" is the norm after
 * the mean removal, as in mgp_project).
 * MGP_ERR_ARG, with the entry point's name in mgp_batch_last_error: NULL vx or vy (vz in 3D) "NULL face array",
 * "unknown mem", "unknown op", member outside [-1, B), fmg_cycles < 0 or cycles < 0; a NULL batch: MGP_ERR_ARG.
 * Out of scope: a per-member stop inside the projection, variable density, cell-centred vector fields, a non-zero wall
 * pressure, and a debug scan (batches have none).  Measured (tools/batch_project_time.py,
 * profiles/batch_project_time.json): README "Batched MAC-grid projection". */
int         mgp_batch_divergence(mgp_batch* b, int member, const void* vx, const void* vy, const void* vz, int mem);
int         mgp_batch_gradient(mgp_batch* b, int member, int op, void* vx, void* vy, void* vz, int mem);
int         mgp_batch_project(mgp_batch* b, void* vx, void* vy, void* vz, int mem, int32_t fmg_cycles, int32_t cycles,
                              double* div_before, double* div_after);

/* The reference's debugging check (MultigridCPURaw.debugging / MultigridGPU.debugging: show / showAndCheck after
 * every sweep and piece of twoGrid, error "found a nan" on a non-finite cell; cpu-raw.lua:126-140,
 * gpu.lua:269-284).  mode 1: every phase of every cycle (pre-smoothing, the restricted residual, the coarse solve
 * or tail, prolongation + post-smoothing, per level) is followed by a device-side scan of its output; mgp_cycle /
 * mgp_cycles then return MGP_ERR_STATE naming the FIRST phase whose output holds a NaN or inf ("found a nan: cycle
 * c, level l (nx x ny x nz), <phase>").  Cycles run eagerly while it is on.  mode 0: off (the default). */
int         mgp_set_debug(mgp_ctx* c, int mode);

/* Kernel and communication timing with HIP events on the stream the work runs on.  mgp_timing(c, 1) resets
 * and enables (cycles then run eagerly, without hipGraph replay, so each launch can be bracketed).
 * Timed kinds; the first three on level 0 only:
 *   MGP_TIMING_HALF_SWEEP  plain red/black (or Jacobi) half-sweeps (not the err-fused last ones);
 *                          1.5 reals per cell per launch
 *   MGP_TIMING_FUSED_PRE   temporally blocked nu1 sweeps + residual + restriction: ALGORITHMIC bytes
 *                          (2 + 2^-dim) reals per cell (read black u and f, write black u and R / 2^dim;
 *                          2.5 with the full weighting, which restricts after the phase)
 *   MGP_TIMING_FUSED_POST  temporally blocked prolongation + correction + nu2 sweeps (+ err): (2.5 + 2^-dim
 *                          [+ 1 psiOld]) reals per cell
 *   MGP_TIMING_FUSED_PRE_SUB / _POST_SUB  the same two phases on the levels >= 1 that run them temporally blocked,
 *                          timed, counted and named (mgp_timing_kernel) exactly as the level-0 kinds
 *   MGP_TIMING_EXCHANGE    every halo exchange of any level (grouped send/recv with the z-neighbours, on the
 *                          compute or the side stream); bytes = what this rank sends
 *   MGP_TIMING_COLLECTIVE  the agglomeration all-gather and the err all-reduce; bytes = what this rank sends
 *   MGP_TIMING_REFINE_DEFECT / _ADD  the two fp64 passes of mgp_refine_residual / _step / _solve (with their
 *                          final sums): 24 (20 without the zero guess) and 20 bytes per cell
 * mgp_timing_read returns, for one kind, the summed milliseconds, the number of timed launches / calls and
 * their bytes (algorithmic for the kernels: SURVEY.md §8d, not measured traffic). */
enum { MGP_TIMING_HALF_SWEEP = 0, MGP_TIMING_FUSED_PRE = 1, MGP_TIMING_FUSED_POST = 2, MGP_TIMING_EXCHANGE = 3,
       MGP_TIMING_COLLECTIVE = 4, MGP_TIMING_REFINE_DEFECT = 5, MGP_TIMING_REFINE_ADD = 6, MGP_TIMING_FUSED_PRE_SUB = 7,
       MGP_TIMING_FUSED_POST_SUB = 8, MGP_TIMING_KINDS = 9 };
int         mgp_timing(mgp_ctx* c, int enable);
int         mgp_timing_read(mgp_ctx* c, int kind, double* ms_total, int64_t* launches, double* bytes);
/* The kernel the last timed launch of a kind ran (MGP_TIMING_FUSED_PRE / _POST: level 0; _PRE_SUB / _POST_SUB: the
 * last such launch of a level >= 1): its symbol with the
 * template arguments as rocprofv3 prints it (NUL-terminated, truncated to cap bytes) and its grid in work-items
 * (rocprofv3's Grid_Size), so that PMC counters measured separately can be matched to exactly this launch.
 * MGP_ERR_STATE when no launch of that kind was timed since mgp_timing(c, 1).  No reference counterpart
 * (measurement only). */
int         mgp_timing_kernel(mgp_ctx* c, int kind, char* name, int cap, int64_t* grid);

/* The exchanges and collectives this rank has issued since creation or the last reset (reset != 0 clears after
 * reading), in issue order: up to max_rows rows of 5 int64 {op, side, level, msgs, bytes}, op 0 = halo exchange
 * (msgs per neighbour and direction, bytes sent per neighbour), 1 = agglomeration all-gather (bytes of this
 * rank's part), 2 = err all-reduce (8 bytes); side 1 = issued on the side stream (under RCCL on its own communicator, split off
 * the context's at creation).  Returns the
 * number of rows recorded (which may exceed max_rows).  Every rank of a decomposition must issue the same
 * sequence per communicator (RCCL matches calls in order); tests compare the ranks' logs. */
int         mgp_comm_log(mgp_ctx* c, int64_t* rows, int max_rows, int reset);
/* The same log for `cycles` outer iterations of a context mgp_create(o) would build, computed on the host
 * without a device (the cycle's host logic runs with every device and RCCL call skipped): what each rank of a
 * world > 1 decomposition will issue per cycle.  GPU tests check it against the executed mgp_comm_log. */
int         mgp_plan_comm(const mgp_opts* o, int32_t cycles, int64_t* rows, int max_rows);

/* Measurement helper (BASELINE.md "a measured copy-kernel peak"): the best of `reps` 16-byte streaming copies
 * of `bytes` between two fresh device buffers on `device` (-1: current), over three copy-kernel shapes
 * (grid-stride, one pass, one pass non-temporal), in GB/s of read + write bytes. */
int         mgp_copy_bandwidth(int device, int64_t bytes, int32_t reps, double* gbps);

#ifdef __cplusplus
}
#endif
#endif /* MGPOISSON_H */
