// mgp_zs.h — the 3D temporally blocked smoothing phases (k_zs): the build knobs, the tile and shape structs, the
// per-column device helpers and the kernel template, and what the launchers of k_zs and of its stage-split variants
// share (zs_patch, zs_grid), and k_zs's launcher, dispatch and LDS attributes as templates on the real type: mgp_zs.hip
// instantiates the fp32 ones, mgp_zs_f64.hip the fp64 ones.  The stage-split variants and the 2D k_ys, which are built on
// the same helpers, are in mgp_kernels.hip.
#pragma once
#include "mgp_device.h"

#include <cstdio>
#include <type_traits>
#include <utility>

namespace mgp {
namespace {

// ---- z-streamed temporally blocked smoothing (3D, red/black 2+2) -------------------------------
//
// k_zs applies a whole smoothing phase of a level in ONE pass over HBM:
//   PRE : 2 RB-GS sweeps, then residual + restriction (smooth(l, 2) + residual_restrict(l))
//   POST: prolongation + correction, then 2 RB-GS sweeps (+ err) (prolong_correct + smooth(l, 2))
// A workgroup owns an x-y tile (plus a halo of H rows and S::HX >= H cells per side) and a chunk of zc
// planes and streams through z.  Every thread owns one column of the extended tile: N consecutive
// cells of each colour of one row.  At step p:
//   stage 0   plane p of the input's BLACK cells (POST: plus the prolongation, k_prolong_v's
//             expressions).  Red cells are never loaded: half-sweep 1 overwrites them, and a
//             Gauss-Seidel update does not read the value it replaces.
//   stage k   half-sweep k (k = 1..4, red first) on plane p - k.
//   last      the smoothed plane p - 4 is stored; PRE: residual + restriction of plane p - 5
//             (k_resrestrict's expressions, children summed in the reference order, the odd row's
//             residuals handed to the even row through LDS); POST: (psi - psiOld)^2 partials.
// The z-neighbours of stage k's inputs are the thread's own registers (a window of 3-4 planes per
// stage).  The in-plane neighbours (rows above / below, the neighbouring groups of the row) come
// from LDS, where every stage leaves the plane it computed; stage k reads the plane stage k-1
// wrote one step earlier, so a step issues its LDS reads up front and needs one barrier.  Cells
// outside the box are never written to LDS (they read as 0 there: the Dirichlet ghost) and
// planes outside it are forced to 0; halo cells are recomputed by every tile that needs them (the
// trapezoid shrinks by one cell per stage).  Plane indices are clamped to the readable planes, so
// the loads need no branches.  On a slab-distributed level the z-halo comes from H ghost planes per
// side (u: black cells, f).  HBM traffic per cell: PRE reads black u and f and writes u and R/8
// (2.625 reals), POST reads black u, V/8, f and psiOld and writes u (3.625 reals), against 8.125
// and 9.125 for the launch-per-piece path.

// (lds_barrier: mgp_device.h)
#ifdef ZS_NOCHAIN  // timing experiment only: each stage's newest z-neighbour is an older ring entry,
#define ZS_NC 1    // so the stages of a step do not depend on each other (results are wrong)
#else
#define ZS_NC 0
#endif
#ifdef ZS_NOLOAD  // timing experiment only: every plane reads plane 0 (cache-resident)
#define ZS_PLANE(q) 0
#else
#define ZS_PLANE(q) (q)
#endif

// Tile and column width: N cells of each colour per thread.  fp32 PRE uses 16-byte columns (7 waves,
// fewest instructions per cell: 576 us against 762 us with 8-byte columns at 512^3); fp32 POST,
// whose prolongation and err make it VALU-bound, uses 8-byte columns (14 waves: 642 against
// 756 us).  exp/run.sh A/B; ZS_NPRE_F32 / ZS_NPOST_F32 override.
#ifndef ZS_NPRE_F32
#define ZS_NPRE_F32 4
#endif
// Row-parity-uniform waves (ZS_PSPLIT, see ZsShape) and x-edge operands read raw at the extended tile's
// outer groups (ZS_XRAW: those cells lie in the halo that every stage shrinks by one cell, so their
// values never reach an owned cell and need no zeroing select)
#ifndef ZS_PSPLIT
#define ZS_PSPLIT 0
#endif
#ifndef ZS_PSPLIT_PRE
#define ZS_PSPLIT_PRE ZS_PSPLIT
#endif
#ifndef ZS_PSPLIT_POST
#define ZS_PSPLIT_POST ZS_PSPLIT
#endif
#ifndef ZS_XRAW
#define ZS_XRAW 1
#endif
#ifndef ZS_YROLE
#define ZS_YROLE 1
#endif
#ifndef ZS_XROLE  // (with ZS_YROLE: the tile rows' x-halo column groups in waves of their own)
#define ZS_XROLE 1
#endif
#ifndef ZS_XPAIR  // (with ZS_XROLE: tile rows r and r + 4 in each 16-lane pass of a tile wave)
#define ZS_XPAIR 1
#endif
#ifndef ZS_FHALO
#define ZS_FHALO 1
#endif
#ifndef ZS_NPOST_F32
#define ZS_NPOST_F32 2
#endif
// PRE tile height: 64 (less y halo, 12 waves) spills at the 168-VGPR cap and measured slower
// (640 against 578 us).  fp64 PRE: 32 x 32 tiles (8 waves, 216 VGPRs) instead of 64 x 16 (9 waves,
// spilling at the 168-VGPR cap): 1111 -> 800 us at 512^3; fp64 POST stays 64 x 16 (890 us against
// 999 / 1536 us for 32 x 32 / 32 x 16).
#ifndef ZS_TYPRE_F32
#define ZS_TYPRE_F32 32
#endif
#ifndef ZS_TYPOST_F32
#define ZS_TYPOST_F32 32
#endif
#ifndef ZS_TXPRE_F32
#define ZS_TXPRE_F32 64
#endif
#ifndef ZS_TXPOST_F32
#define ZS_TXPOST_F32 64
#endif
// PRE on a level with a boundary-modified operator (cl != 0): its own tile (the boundary diagonals cost
// registers: at the level-0 shape the variant spills)
#ifndef ZS_TXPRE_CL_F32
#define ZS_TXPRE_CL_F32 ZS_TXPRE_F32
#endif
#ifndef ZS_TYPRE_CL_F32
#define ZS_TYPRE_CL_F32 ZS_TYPRE_F32
#endif
#ifndef ZS_NPRE_CL_F32
#define ZS_NPRE_CL_F32 ZS_NPRE_F32
#endif
// POST's wide tile (levels with cl = 0 whose box it divides; MGP_ZS_WIDE=0 turns it off): a 64-wide tile's row
// of one colour is one 128-byte line, and its x halo (2 packed cells per side) touches the two neighbouring
// lines, so every row costs 3 line requests per field for 1 line of data; 128 x 16 tiles cost 4 for 2.
// 512^3 POST 480 -> 436 us (round 4).  Its 14 waves leave 128 VGPRs (a few spill).
#ifndef ZS_TXPOST_W_F32
#define ZS_TXPOST_W_F32 128
#endif
#ifndef ZS_TYPOST_W_F32
#define ZS_TYPOST_W_F32 16
#endif
#ifndef ZS_NPOST_W_F32  // (4: 128 x 16 POST at 18 x 24 threads measured 439 against 434 us)
#define ZS_NPOST_W_F32 ZS_NPOST_F32
#endif
template <typename T>
struct ZsTile;
template <>
struct ZsTile<float> {
    static constexpr int TXPRE = ZS_TXPRE_F32, TXPOST = ZS_TXPOST_F32, TYPRE = ZS_TYPRE_F32, TYPOST = ZS_TYPOST_F32,
                         NPRE = ZS_NPRE_F32, NPOST = ZS_NPOST_F32;
    static constexpr int TXPRE_CL = ZS_TXPRE_CL_F32, TYPRE_CL = ZS_TYPRE_CL_F32, NPRE_CL = ZS_NPRE_CL_F32;
    static constexpr int TXPOST_W = ZS_TXPOST_W_F32, TYPOST_W = ZS_TYPOST_W_F32, NPOST_W = ZS_NPOST_W_F32;
};
#ifndef ZS_TXPRE_F64
#define ZS_TXPRE_F64 32
#endif
#ifndef ZS_TXPOST_F64
#define ZS_TXPOST_F64 64
#endif
#ifndef ZS_TYPRE_F64
#define ZS_TYPRE_F64 32
#endif
#ifndef ZS_TYPOST_F64
#define ZS_TYPOST_F64 16
#endif
template <>
struct ZsTile<double> {
    static constexpr int TXPRE = ZS_TXPRE_F64, TXPOST = ZS_TXPOST_F64, TYPRE = ZS_TYPRE_F64, TYPOST = ZS_TYPOST_F64,
                         NPRE = 2, NPOST = 2;
    static constexpr int TXPRE_CL = TXPRE, TYPRE_CL = TYPRE, NPRE_CL = NPRE;
    static constexpr int TXPOST_W = TXPOST, TYPOST_W = TYPOST, NPOST_W = NPOST;  // (no wide fp64 variant is instantiated)
};
// Streaming (non-temporal) level-0 loads / stores of the phases: timing experiments (ZS_NT bit 0:
// loads, bit 1: stores), so that the level-0 stream does not evict the coarse level it writes
#ifndef ZS_NT
#define ZS_NT 0
#endif
// bit 2: psiOld loads only (read once per launch: nothing else in the launch reads them)
constexpr bool kZsNTL = (ZS_NT & 1) != 0, kZsNTS = (ZS_NT & 2) != 0, kZsNTO = (ZS_NT & 5) != 0;
#ifndef ZS_PRE_RED_STORE  // timing experiment: PRE stores its (unread) red cells too
#define ZS_PRE_RED_STORE 0
#endif
constexpr bool kZsPreRed = ZS_PRE_RED_STORE != 0;

// FWF (PRE only): the full-weighting restriction fused into the phase (k_zs LINEAR = 2): the residual is needed one
// cell beyond the tile (the full weighting's 4-cell stencil), so the trapezoid is one stage deeper (H = 6)
// NF != 0: that column width instead of the tile's (k_zs_split_post: 16-byte columns on POST's wide tile)
template <typename T, bool PRE, bool CLZ = true, bool WIDE = false, bool FWF = false, int NF = 0>
struct ZsShape {
    static constexpr int N = NF ? NF
                                : (PRE ? (CLZ ? ZsTile<T>::NPRE : ZsTile<T>::NPRE_CL)
                                       : (WIDE ? ZsTile<T>::NPOST_W : ZsTile<T>::NPOST));
    static constexpr int TX = PRE ? (CLZ ? ZsTile<T>::TXPRE : ZsTile<T>::TXPRE_CL)
                                  : (WIDE ? ZsTile<T>::TXPOST_W : ZsTile<T>::TXPOST);
    static constexpr int TY = PRE ? (CLZ ? ZsTile<T>::TYPRE : ZsTile<T>::TYPRE_CL)
                                  : (WIDE ? ZsTile<T>::TYPOST_W : ZsTile<T>::TYPOST);
    static constexpr int H = PRE ? (FWF ? 6 : 5) : 4;  // y/z halo = stages that read neighbours
    // x halo cells per side: the trapezoid depth H in whole column groups (2 N cells of x each)
#ifdef ZS_HX_FIXED  // timing experiment: the round-1 fixed 8-cell x halo
    static constexpr int HX = ZS_HX_FIXED;
#else
    static constexpr int HX = 2 * N * ((H + 2 * N - 1) / (2 * N));
#endif
    static constexpr int HWE = (TX + 2 * HX) / 2;      // reals per LDS half-row
    static constexpr int G = HWE / N;                  // column groups per row
    static constexpr int HXG = HX / 2 / N;             // halo groups per side
    static constexpr int YE = TY + 2 * H;
    static constexpr int NT = G * YE;                  // threads with a column
    // ZS_PSPLIT: the even extended rows in waves [0, NPAR / 64), the odd ones in the waves after them, so
    // that a wave's row parity is uniform and steady steps know every cell's colour at compile time
    static constexpr int YEV = (YE + 1) / 2;           // even extended rows
    static constexpr int NPAR = (G * YEV + 63) / 64 * 64;
    static constexpr bool PS = PRE ? ZS_PSPLIT_PRE != 0 : ZS_PSPLIT_POST != 0;
    static constexpr int NTL = PS ? 2 * NPAR : (NT + 63) / 64 * 64;  // launched threads
    // PRE, ZS_YROLE: threads ordered by their row's distance d from the tile in y (tile rows first, then d = 1..3,
    // then d = 4..5 from a wave boundary), so that whole waves hold only halo rows: stage k (half-sweep k) is needed
    // on rows d <= H - k and the residual on d = 0, so a wave of rows d >= 4 runs stage 1 only and a wave of rows
    // d in 1..3 skips the residual (a third of the step's VALU for the halo waves; only where it costs no wave)
    static constexpr int YT0 = TY * G, YT1 = YT0 + 6 * G, YT2S = (YT1 + 63) / 64 * 64, YT2 = YT2S + 4 * G;
    static constexpr bool YROLE = ZS_YROLE && PRE && !PS && H == 5 && (YT2 + 63) / 64 * 64 <= NTL;
    // ZS_XROLE: the tile rows' own columns (TC threads, whole waves) first, then their x-halo column groups (HXG per
    // side; those need stages 1..4 but no residual, role 1), so that the waves that run everything are TC / 64 (4 of
    // 7 at 64 x 32: one per SIMD, where 5 put two on one SIMD)
    static constexpr int GC = G - 2 * HXG, TC = TY * GC;
    static constexpr bool XROLE = YROLE && ZS_XROLE && TC % 64 == 0;
    // ZS_XPAIR (XROLE with 8 column groups per tile row and HWE = 40): a tile wave's 64 lanes hold 8 rows x 8
    // groups so that every 16-byte LDS access is conflict-free (MI355X_MICROARCH.md §LDS: ds_read_b128 serves the
    // lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32) with banks (a/4) mod 64, ds_write_b128 8
    // contiguous lanes with banks (a/4) mod 32).  Rows r and r + 4 start 160 words apart (32 mod 64), so each read
    // group holds two whole rows (lanes 0-31: rows 0, 4 and 1, 5; lanes 32-63: 2, 6 and 3, 7), and each write block
    // of 8 lanes holds 4 cells of each of two rows whose slots (mod 8) do not meet; row order / neighbour offsets
    // move every lane alike, so the x and y neighbour reads stay conflict-free.  (Row-major 8 x 8 lanes: 2-way.)
    static constexpr bool XPAIR = XROLE && ZS_XPAIR && GC == 8 && TY % 8 == 0 && HWE == 40;
    // lane l of a tile wave: quad q = (l & 31) >> 2 -> row xp_row(q) + 2 (l >> 5), group (xp_gx(q) + (l & 3)) & 7
    static __device__ __forceinline__ int xp_row(int q) { return (0x54450110 >> (4 * q)) & 15; }  // 0 1 1 0 5 4 4 5
    static __device__ __forceinline__ int xp_gx(int q) { return (0x64024620 >> (4 * q)) & 15; }   // 0 2 6 4 2 0 4 6
    // extended row (0 .. YE - 1) of thread t (-1: no row) and the role of wave w (0: tile rows, every stage and the
    // residual; 1: rows d <= 3 (XROLE: and the tile rows' x-halo groups), stages 1..4; 2: rows d >= 4, stage 1)
    static __device__ __forceinline__ int yrow(int t)
    {
        if (!YROLE) return t < NT ? t / G : -1;
        if (XPAIR && t < TC) return H + 8 * (t >> 6) + xp_row((t & 31) >> 2) + 2 * ((t >> 5) & 1);
        if (t < YT0) return H + (XROLE ? (t < TC ? t / GC : (t - TC) / (2 * HXG)) : t / G);
        // rows d = 1..3 (role 1) and d = 4, 5 (role 2): the ones above the tile, then the ones below, each in LDS row
        // order (conflict-free 16-byte accesses, where alternating above / below rows overlapped banks)
        if (t < YT1) {
            const int r = (t - YT0) / G;
            return r < 3 ? H - 3 + r : H + TY + r - 3;
        }
        if (t >= YT2S && t < YT2) {
            const int r = (t - YT2S) / G;
            return r < 2 ? H - 5 + r : H + TY + r + 1;
        }
        return -1;
    }
    static __device__ __forceinline__ int ycol(int t)
    {
        if (XROLE && t < YT0) {
            if (t < TC) return HXG + (XPAIR ? ((xp_gx((t & 31) >> 2) + (t & 3)) & 7) : t % GC);
            const int k = (t - TC) % (2 * HXG);
            return k < HXG ? k : GC + k;
        }
        return YROLE && t >= YT2S ? (t - YT2S) % G : t % G;
    }
    static constexpr int wave_role(int w)
    {
        return !YROLE || 64 * w < (XROLE ? TC : YT0) ? 0 : (64 * w < YT1 ? 1 : 2);
    }
    static constexpr int SLOT = YE * HWE;              // reals per LDS slot (one colour of a plane)
    // stage-3 slots: PRE's residual reads 2 back (3 needed; 4 while LDS allows: power-of-2 ring)
    static constexpr int NS3 = PRE ? (TY > 32 ? 3 : 4) : 2;
    static constexpr int OFF1 = 2 * SLOT, OFF2 = 4 * SLOT, OFF3 = 6 * SLOT, OFF4 = OFF3 + NS3 * SLOT;
    static constexpr int OFFX = OFF4 + (PRE ? 2 * SLOT : 0);
    static constexpr int XPAIRS = YE / 2 + 1;          // row pairs of the residual hand-off
    static constexpr int XSLOT = PRE ? XPAIRS * G * 2 * N : 0;
    // POST: coarse rows J in [Y0/2 - 3, Y0/2 + TY/2 + 3) and cells I in [X0/2 - 8, X0/2 + TX/2 + 8)
    // of 4 coarse planes around the stream position, unpacked (x order, both colours)
    static constexpr int CJ = PRE ? 0 : TY / 2 + 6, CI = PRE ? N : TX / 2 + 16;
    static constexpr int CSLOT = CJ * CI, CPAIRS = CSLOT / 2;
    static constexpr int OFFC = OFFX + 2 * XSLOT;
    // FWF: the residual rows in x order (RXSLOT per step parity), their x-combinations (AXSLOT per step parity) and a
    // ring of the y-combinations of 4 fine planes per coarse cell of the tile (AYSLOT per plane)
    static constexpr int RXSLOT = FWF ? YE * G * 2 * N : 0, AXSLOT = FWF ? YE * G * N : 0,
                         AYSLOT = FWF ? (TY / 2) * (TX / 2) : 0;  // (item i's N cells at i N)
    static constexpr int OFFRX = OFFC + 4 * CSLOT, OFFAX = OFFRX + 2 * RXSLOT, OFFAY = OFFAX + 2 * AXSLOT;
    // FWF: the wave running the y-combinations (the 4th when the workgroup has 7 waves: alone on its SIMD) and its
    // items per lane
    static constexpr int FWY = NTL >= 4 * 64 ? 3 : 0;
    static constexpr int FWYI = FWF ? (TY / 2) * (TX / (2 * N)) / 64 : 0;
    static_assert(!FWF || ((TY / 2) * (TX / (2 * N)) % 64 == 0 && FWY * 64 + 64 <= NTL), "FWF: whole waves of y items");
    static constexpr size_t lds_bytes = (size_t)(OFFAY + 4 * AYSLOT) * sizeof(T);
    static_assert(CPAIRS <= 2 * NTL, "coarse staging: two pairs per thread");
    static_assert(CI % N == 0 && OFFC % N == 0, "coarse rows must hold aligned groups");
    static_assert(NTL <= 1024, "too many threads");
    static_assert(2 * N * HXG >= H, "x halo too small");
    static_assert(HWE % N == 0, "LDS row must hold whole groups");
};

template <typename T, int N>
struct ZsPrefetch {
    Vec<T, N> u;                                       // stage 0: black cells of the input at plane p
    Vec<T, 2> cv[2];                                   // POST: this thread's coarse pairs for the ring
    Vec<T, N> f1, f2;  // f of half-sweeps 1 (red, plane p - 1) and 2 (black, plane p - 2); sweeps 3
                       // and 4 reuse them two steps later
    Vec<T, N> o0, o1;  // POST + ERR: psiOld (red, black) of plane p - 4, the plane step p finalizes
};

// Pin a prefetched vector: the compiler must have waited for its load before this point, and no
// memory access is moved across it.  Used at the top of a step so that the wait for plane p's loads
// (a vmcnt(0) once stores are pending: gfx9 counts loads and stores together) comes before plane
// p + 1's prefetch is issued, not after it.
template <typename T, int N>
__device__ __forceinline__ void zs_hold(const Vec<T, N>& a)
{
#pragma unroll
    for (int e = 0; e < N; ++e) asm volatile("" ::"v"(a.v[e]));
}

struct ZsCol {
    int lrow, lym, lyp, lxm, lxp, gm;
    bool x_first, x_last;
    bool xin;  // no cell of the group touches the x faces of the box (or the column is outside it)
};

// In-plane operands of one stage's cells: the other colour in the rows above / below and the x
// neighbours beyond my group (last cell of the left group, first of the right group).  Stage k
// reads them from the LDS slot stage k-1 filled one step earlier.
template <typename T, int N>
struct ZsNb {
    Vec<T, N> yl, yr;
    T ep, en;
};

template <typename T, int N>
__device__ __forceinline__ void zs_nb_load(ZsNb<T, N>& nb, const T* s_in, const ZsCol& c)
{
#ifdef ZS_NOLDSREAD  // timing experiment only: results are wrong
    nb.yl = nb.yr = vzero<T, N>();
    nb.ep = nb.en = (T)c.lrow;
    return;
#endif
    nb.yl = vload<T, N>(s_in + c.lym);
    nb.yr = vload<T, N>(s_in + c.lyp);
    // whole neighbouring groups (conflict-free), of which one cell each is used
    const Vec<T, N> l = vload_lds_whole<T, N>(s_in + c.lxm), r = vload_lds_whole<T, N>(s_in + c.lxp);
    nb.ep = (c.x_first && !ZS_XRAW) ? (T)0 : l.v[N - 1];
    nb.en = (c.x_last && !ZS_XRAW) ? (T)0 : r.v[0];
}

// xl + xr of my N cells of x parity o (IEEE addition commutes, so the pair sums are shared
// between the two parities)
template <typename T, int N>
__device__ __forceinline__ void zs_xsum(const Vec<T, N>& cen, const ZsNb<T, N>& nb, int o, T (&s)[N])
{
    const T edge = o == 0 ? nb.ep : nb.en;
    T m[N + 1];
    m[0] = edge + cen.v[0];
#pragma unroll
    for (int e = 0; e + 1 < N; ++e) m[e + 1] = cen.v[e] + cen.v[e + 1];
    m[N] = cen.v[N - 1] + edge;
#pragma unroll
    for (int e = 0; e < N; ++e) s[e] = o == 0 ? m[e] : m[e + 1];
}

// ((((xl + xr) + yl) + yr) + zl) + zr of my N cells
template <typename T, int N>
__device__ __forceinline__ void zs_nbsum(const Vec<T, N>& zl, const Vec<T, N>& cen, const Vec<T, N>& zr,
                                         const ZsNb<T, N>& nb, int o, T (&t)[N])
{
    zs_xsum<T, N>(cen, nb, o, t);
#pragma unroll
    for (int e = 0; e < N; ++e) {
        t[e] = t[e] + nb.yl.v[e];
        t[e] = t[e] + nb.yr.v[e];
        t[e] = t[e] + zl.v[e];
        t[e] = t[e] + zr.v[e];
    }
}

// Steady-step diagonals of a level with a boundary-modified operator (cl != 0): inside the z-range
// of the steady steps a cell's face count is nby (its row on a y face) plus 1 for the x-face cell,
// which can only be the first cell of a group at the left edge (x parity 0) or the last at the right
// edge (x parity 1).  db / yb = dg[nby] / RN(1/dg[nby]), de / ye = dg[nby + 1] / RN(1/dg[nby + 1]):
// the table Markstein division of Op::relax without selects over the whole table.
template <typename T>
struct ZsDiag {
    T db, yb, de, ye;
    bool left, right;
};

// dz's diagonals as register values.  Without the opaque copy the compiler turns `edge ? dz.de : dz.db`
// into a select of the two members' addresses and keeps dz in private memory: six scratch loads per
// step on every cl != 0 PRE step (5x the launch's vector memory reads, 670 against 407 us for the
// same launch with the cl = 0 code at 1024^2 x 128).
template <typename T>
__device__ __forceinline__ void zs_dvals(const ZsDiag<T>& dz, T& db, T& yb, T& de, T& ye)
{
    db = dz.db;
    yb = dz.yb;
    de = dz.de;
    ye = dz.ye;
    asm("" : "+v"(db), "+v"(yb), "+v"(de), "+v"(ye));
}

// The diagonals of a step's cells: the steady ones (dz), or, in a generic step (TAB), the row's table entries for
// its nbyz y / z faces (Op::row_diag: the table Markstein form of Op::relax, no IEEE division and no divergent
// boundary path; dz.left / dz.right mark the x-face cell as in the steady steps)
template <typename T, bool ST>
__device__ __forceinline__ void zs_diag(const Op<T, 3>& op, const ZsDiag<T>& dz, int nbyz, T& db, T& yb, T& de, T& ye)
{
    if (ST)
        zs_dvals(dz, db, yb, de, ye);
    else
        row_diag_fast(op, nbyz, db, yb, de, ye);
}

// One half-sweep of my N cells of one colour (x parity o) from the other colour's window
// (zl, cen, zr) and its in-plane operands: k_half's expressions.  Waves whose cells all have the
// interior diagonal (every wave of a level with cl = 0) take the reciprocal form, which is what
// Op::relax computes there.
// ask: the cells' neighbour sums times 1/h^2 (the askew of k_resrestrict's expression, same operands and
// order): a PRE black cell's residual one step later sees exactly these neighbours (zs_residual_a)
template <typename T, int N, bool CLZ, bool ST = false, bool TAB = false>
__device__ __forceinline__ Vec<T, N> zs_relax_a(const Vec<T, N>& zl, const Vec<T, N>& cen, const Vec<T, N>& zr,
                                                const ZsNb<T, N>& nb, const Vec<T, N>& fv, const ZsCol& c, int o,
                                                int nbyz, int nx, const Op<T, 3>& op, const ZsDiag<T>& dz,
                                                T (&ask)[N])
{
    Vec<T, N> out;
    T t[N];
    zs_nbsum<T, N>(zl, cen, zr, nb, o, t);
#pragma unroll
    for (int e = 0; e < N; ++e) ask[e] = t[e] * op.inv_hSq;
    if (!CLZ && (ST || TAB)) {
        T db, yb, de, ye;
        zs_diag<T, ST>(op, dz, nbyz, db, yb, de, ye);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const bool edge = (e == 0 && o == 0 && dz.left) || (e == N - 1 && o == 1 && dz.right);
            out.v[e] = div_rn(fv.v[e] - ask[e], edge ? de : db, edge ? ye : yb);
        }
    } else if (CLZ || __all(nbyz == 0 && c.xin)) {
#pragma unroll
        for (int e = 0; e < N; ++e) out.v[e] = div_rn(fv.v[e] - ask[e], op.adiag, op.yadiag);
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int i = 2 * (c.gm + e) + o;
            out.v[e] = op.relax_direct(t[e], fv.v[e], nbyz + (i == 0) + (i == nx - 1));
        }
    }
    return out;
}

template <typename T, int N, bool CLZ, bool ST = false, bool TAB = false>
__device__ __forceinline__ Vec<T, N> zs_relax(const Vec<T, N>& zl, const Vec<T, N>& cen, const Vec<T, N>& zr,
                                              const ZsNb<T, N>& nb, const Vec<T, N>& fv, const ZsCol& c, int o,
                                              int nbyz, int nx, const Op<T, 3>& op, const ZsDiag<T>& dz)
{
    T ask[N];
    return zs_relax_a<T, N, CLZ, ST, TAB>(zl, cen, zr, nb, fv, c, o, nbyz, nx, op, dz, ask);
}

// Residual of my N cells of one colour (x parity o) at one plane: k_resrestrict's expressions.
template <typename T, int N, bool CLZ, bool ST = false, bool TAB = false>
__device__ __forceinline__ void zs_residual(const Vec<T, N>& zl, const Vec<T, N>& cen, const Vec<T, N>& zr,
                                            const ZsNb<T, N>& nb, const Vec<T, N>& uc, const Vec<T, N>& fv,
                                            const ZsCol& c, int o, int nbyz, int nx, const Op<T, 3>& op,
                                            const ZsDiag<T>& dz, T (&rr)[N])
{
    T t[N];
    zs_nbsum<T, N>(zl, cen, zr, nb, o, t);
    if (!CLZ && (ST || TAB)) {
        T db, yb, de, ye;
        zs_diag<T, ST>(op, dz, nbyz, db, yb, de, ye);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const bool edge = (e == 0 && o == 0 && dz.left) || (e == N - 1 && o == 1 && dz.right);
            const T askew = t[e] * op.inv_hSq;
            const T a_u = askew + (edge ? de : db) * uc.v[e];
            rr[e] = fv.v[e] - a_u;
        }
    } else if (CLZ || __all(nbyz == 0 && c.xin)) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const T askew = t[e] * op.inv_hSq;
            const T a_u = askew + op.adiag * uc.v[e];
            rr[e] = fv.v[e] - a_u;
        }
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int i = 2 * (c.gm + e) + o;
            rr[e] = op.residual_direct(t[e], fv.v[e], uc.v[e], nbyz + (i == 0) + (i == nx - 1));
        }
    }
}

// The same residual from the cells' askew (zs_relax_a of the half-sweep that last saw these neighbours)
template <typename T, int N, bool CLZ, bool ST = false, bool TAB = false>
__device__ __forceinline__ void zs_residual_a(const T (&ask)[N], const Vec<T, N>& uc, const Vec<T, N>& fv,
                                              const ZsCol& c, int o, int nbyz, int nx, const Op<T, 3>& op,
                                              const ZsDiag<T>& dz, T (&rr)[N])
{
    if (!CLZ && (ST || TAB)) {
        T db, yb, de, ye;
        zs_diag<T, ST>(op, dz, nbyz, db, yb, de, ye);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const bool edge = (e == 0 && o == 0 && dz.left) || (e == N - 1 && o == 1 && dz.right);
            const T a_u = ask[e] + (edge ? de : db) * uc.v[e];
            rr[e] = fv.v[e] - a_u;
        }
    } else if (CLZ || __all(nbyz == 0 && c.xin)) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const T a_u = ask[e] + op.adiag * uc.v[e];
            rr[e] = fv.v[e] - a_u;
        }
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int i = 2 * (c.gm + e) + o;
            const T a_u = ask[e] + op.diag_direct(nbyz + (i == 0) + (i == nx - 1)) * uc.v[e];
            rr[e] = fv.v[e] - a_u;
        }
    }
}

// uv += P V for my N cells of x parity o in one fine row (k_prolong_v's expressions).  Waves with
// no cell next to a face of the coarse box take the interior form (every factor is 1 there).
template <typename T, int N>
struct ZsCoarse {
    T c00[N + 2], c10[N + 2], c01[N + 2], c11[N + 2];  // [z: K / Kn][y: J / Jn], cells I0-1 .. I0+N
};

template <typename T, int N, int LINEAR>
__device__ __forceinline__ void zs_correct(Vec<T, N>& uv, const ZsCoarse<T, N>& cur, int o, int I0, int cx, bool oy,
                                           bool oz, T cl, bool fast)
{
    const T w0 = (T)0.75, w1 = (T)0.25;
    if (!LINEAR) {
#pragma unroll
        for (int e = 0; e < N; ++e) uv.v[e] = uv.v[e] + cur.c00[e + 1];
        return;
    }
    if (fast) {  // __all(!oy && !oz && I0 > 0 && I0 + N < cx), from the caller
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int pe = e + 1;
            const T nb00 = o ? cur.c00[e + 2] : cur.c00[e];
            const T nb10 = o ? cur.c10[e + 2] : cur.c10[e];
            const T nb01 = o ? cur.c01[e + 2] : cur.c01[e];
            const T nb11 = o ? cur.c11[e + 2] : cur.c11[e];
            const T a00 = w0 * cur.c00[pe] + w1 * nb00;
            const T a10 = w0 * cur.c10[pe] + w1 * nb10;
            const T a01 = w0 * cur.c01[pe] + w1 * nb01;
            const T a11 = w0 * cur.c11[pe] + w1 * nb11;
            const T b0 = w0 * a00 + w1 * a10;
            const T b1 = w0 * a01 + w1 * a11;
            uv.v[e] = uv.v[e] + (w0 * b0 + w1 * b1);
        }
        return;
    }
    auto sv = [&](T val, bool fx, bool fy, bool fz) {
        T s = (T)1;
        if (fx) s = -cl * s;
        if (fy) s = -cl * s;
        if (fz) s = -cl * s;
        return s == (T)1 ? val : s * val;
    };
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int pe = e + 1;
        const bool ox = (o == 0 && I0 + e == 0) || (o == 1 && I0 + e == cx - 1);
        auto col = [&](const T (&cc)[N + 2]) { return ox ? cc[pe] : (o ? cc[e + 2] : cc[e]); };
        const T a00 = w0 * cur.c00[pe] + w1 * sv(col(cur.c00), ox, false, false);
        const T a10 = w0 * sv(cur.c10[pe], false, oy, false) + w1 * sv(col(cur.c10), ox, oy, false);
        const T a01 = w0 * sv(cur.c01[pe], false, false, oz) + w1 * sv(col(cur.c01), ox, false, oz);
        const T a11 = w0 * sv(cur.c11[pe], false, oy, oz) + w1 * sv(col(cur.c11), ox, oy, oz);
        const T b0 = w0 * a00 + w1 * a10;
        const T b1 = w0 * a01 + w1 * a11;
        uv.v[e] = uv.v[e] + (w0 * b0 + w1 * b1);
    }
}

// The y-interpolated half of zs_correct for one coarse plane: b[e] = w0 a(J) + w1 a(Jn) with a = the
// x-interpolation of coarse row c0 (J) / c1 (Jn) (zs_correct's b0, or b1 with oz = false: the same
// expressions over the other plane).  A thread's rows J, Jn and its columns never change, so k_zs
// evaluates it once per coarse plane and x parity and keeps it in registers for the four fine planes
// that read the plane.
template <typename T, int N>
__device__ __forceinline__ void zs_bq(T (&b)[N], const T (&c0)[N + 2], const T (&c1)[N + 2], int o, int I0, int cx,
                                      bool oy, T cl, bool fast)
{
    const T w0 = (T)0.75, w1 = (T)0.25;
    if (fast) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const T nb0 = o ? c0[e + 2] : c0[e];
            const T nb1 = o ? c1[e + 2] : c1[e];
            const T a0 = w0 * c0[e + 1] + w1 * nb0;
            const T a1 = w0 * c1[e + 1] + w1 * nb1;
            b[e] = w0 * a0 + w1 * a1;
        }
        return;
    }
    auto sv = [&](T val, bool fx, bool fy) {
        T s = (T)1;
        if (fx) s = -cl * s;
        if (fy) s = -cl * s;
        return s == (T)1 ? val : s * val;
    };
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int pe = e + 1;
        const bool ox = (o == 0 && I0 + e == 0) || (o == 1 && I0 + e == cx - 1);
        auto col = [&](const T (&cc)[N + 2]) { return ox ? cc[pe] : (o ? cc[e + 2] : cc[e]); };
        const T a0 = w0 * c0[pe] + w1 * sv(col(c0), ox, false);
        const T a1 = w0 * sv(c1[pe], false, oy) + w1 * sv(col(c1), ox, oy);
        b[e] = w0 * a0 + w1 * a1;
    }
}

// (block_partial_t: mgp_device.h)

// src: the level's u before the phase; dst: the phase's output; old (POST with ERR): psiOld, either dst
// itself (read plane by plane just before the output overwrites it) or a buffer of its own (kept for the
// reference's metrics, mgp_metrics / psiOld / errorBuf).  V/gc: coarse correction (POST); R/gc: restricted residual (PRE); both point at the
// coarse plane of local fine plane 0 (gc.z0 = g.z0 / 2).  zc: planes per z-chunk.  gz: readable
// ghost planes per side of src / f / dst (on a distributed level they must hold the neighbours'
// current H planes).  CLZ: the level operator has no boundary modification (cl == 0, level 0).
#ifndef ZS_WPE_PRE
#define ZS_WPE_PRE 2
#endif
// Prefetch distance in planes: step p issues the loads of plane p + PFD into one of PFD + 1 register
// buffers (the loop unrolls lcm(PFD + 1, 4) steps, so every buffer and ring index is static)
#ifndef ZS_PFD_PRE
#define ZS_PFD_PRE 2
#endif
#ifndef ZS_PFD_POST
#define ZS_PFD_POST 1
#endif
// PRE on a level with a boundary-modified operator (cl != 0, the coarser fused levels): distance 1 — at 2 the
// variant needed 54 (fp64: 33) VGPRs beyond the 256 of two waves per SIMD and spilled to scratch
#ifndef ZS_PFD_PRE_CL
#define ZS_PFD_PRE_CL 1
#endif
template <typename F, int... K>
__device__ __forceinline__ void zs_unroll_impl(F& f, std::integer_sequence<int, K...>)
{
    (f(std::integral_constant<int, K>()), ...);
}
// f(integral_constant<int, k>) for k = 0 .. U - 1, in order
template <int U, typename F>
__device__ __forceinline__ void zs_unroll(F&& f)
{
    zs_unroll_impl(f, std::make_integer_sequence<int, U>());
}
#ifndef ZS_BQ
#define ZS_BQ 1  // POST: per-thread cache of the coarse planes' y-interpolation (zs_bq)
#endif
// PRE: the black cells' residual reuses the askew of the stage-4 half-sweep that relaxed them one step earlier
// (the same red neighbours, sum order and scaling) instead of re-reading and re-summing those neighbours
#ifndef ZS_RASK
#define ZS_RASK 1
#endif
constexpr bool kZsRask = ZS_RASK != 0;
#ifndef ZS_WPE_POST
#define ZS_WPE_POST 4
#endif
// Tile (tx, ty) of a launch's tile index; patch != 0: the tiles an XCD runs at once form px x py patches (host:
// px | tiles_x, py | tiles_y; zs_patch)
__device__ __forceinline__ void zs_tile_xy(int tile, int tiles_x, int patch, int& tx, int& ty)
{
    tx = tile % tiles_x;
    ty = tile / tiles_x;
    if (patch) {
        const int px = patch & 255, py = patch >> 8, per = px * py, prow = tiles_x / px;
        const int pi = tile / per, q = tile % per;
        tx = (pi % prow) * px + q % px;
        ty = (pi / prow) * py + q / px;
    }
}

// PRE's 2^3-average restriction of one thread's residuals rr[x parity][e] of fine plane q (dq = q - Z0; the odd row's
// residuals xr of plane q - 1 come from the row's partner through xw's other half, see k_zs): the odd rows hand
// theirs to the even row, which sums the eight children in the reference order and stores R / 8 when the coarse
// plane (q - 1) / 2 is complete.
template <typename T, int N>
__device__ __forceinline__ void zs_restrict_avg(const T (&rr)[2][N], const T (&xr)[2 * N], T (&acc)[N], int dq, int zc,
                                                bool even_row, T* xw, T* __restrict__ R, int K, int J, int gm, int cz0,
                                                const Geo& gc)
{
    if (!even_row) {
        if (dq < zc) {
#pragma unroll
            for (int e = 0; e < N; ++e) {
                xw[e] = rr[0][e];
                xw[N + e] = rr[1][e];
            }
        }
    } else {
        if (dq >= 1) {  // the odd row's children of plane q - 1
#pragma unroll
            for (int e = 0; e < N; ++e) {
                acc[e] = acc[e] + xr[e];
                acc[e] = acc[e] + xr[N + e];
            }
            if ((dq & 1) == 0) {  // coarse plane (q - 1) / 2 complete (K, J: global)
                T* rowc = R + (int64_t)(K - cz0) * gc.P + (int64_t)J * gc.hw;
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const int I = gm + e;
                    rowc[((I + J + K) & 1) * gc.H + (I >> 1)] = (T)0.125 * acc[e];
                }
            }
        }
        if (dq < zc) {
#pragma unroll
            for (int e = 0; e < N; ++e) {
                if ((dq & 1) == 0) {
                    acc[e] = rr[0][e] + rr[1][e];
                } else {
                    acc[e] = acc[e] + rr[0][e];
                    acc[e] = acc[e] + rr[1][e];
                }
            }
        }
    }
}

#ifndef ZS_ALL_GENERIC  // timing experiment: every step generic (the price of the box-face steps)
#define ZS_ALL_GENERIC 0
#endif
// timing experiment only (wrong at the box's z faces): on cl != 0 levels a chunk at a z face runs the steps of an
// interior chunk (the z-face tests off, the steady loads through the plane clamp): the most that cheaper face steps
// can win
#ifndef ZS_FACE_AS_INTERIOR
#define ZS_FACE_AS_INTERIOR 0
#endif

template <typename T, bool PRE, int LINEAR, bool ERR, bool CLZ, bool WIDE = false>
__global__ __launch_bounds__((ZsShape<T, PRE, CLZ, WIDE, PRE && LINEAR == 2>::NTL))
__attribute__((amdgpu_waves_per_eu(1, PRE ? ZS_WPE_PRE : ZS_WPE_POST))) void k_zs(const T* __restrict__ src, const T* __restrict__ f,
                                                                T* __restrict__ dst, const T* old, T* __restrict__ R,
                                                                const T* __restrict__ V, double* __restrict__ partials,
                                                                Geo g, Geo gc, Op<T, 3> op, T clc, int zc, int gz,
                                                                int patch)
{
    // PRE: LINEAR selects the restriction: 0 = residual + 2^3 average here; 1 = none (both colours of the
    // smoothed level stored; the host runs the full-weighting restriction after the phase); 2 = residual + the full
    // weighting here (FWF)
    constexpr bool FWF = PRE && LINEAR == 2;
    using S = ZsShape<T, PRE, CLZ, WIDE, FWF>;
    constexpr int N = S::N, H = S::H, HWE = S::HWE, G = S::G, YE = S::YE, SLOT = S::SLOT, TX = S::TX,
                  TY = S::TY, NS3 = S::NS3, NTL = S::NTL;
    constexpr bool RR = PRE && LINEAR == 0;
    // PRE with ERR (which only POST uses): the input is a fresh zero guess, never loaded (src may be null); this
    // replaces the memset of a fused coarse level's u before its PRE
    constexpr bool ZSRC = PRE && ERR;
    using VT = Vec<T, N>;
    using PF = ZsPrefetch<T, N>;
    constexpr int PFD = PRE ? (CLZ ? ZS_PFD_PRE : ZS_PFD_PRE_CL) : ZS_PFD_POST, NPF = PFD + 1, UNR = NPF == 3 ? 12 : 4;
    static_assert(PFD >= 1 && PFD <= 3, "prefetch distance 1..3");
    // cl != 0: the generic steps (the box's z faces) take the row's table diagonals (zs_diag), as k_zs_split_cl's do:
    // bit-identical to relax_direct / residual_direct (mgp_device.h) without their divergent IEEE division
    constexpr bool TAB = !CLZ;
    constexpr bool FAI = ZS_FACE_AS_INTERIOR && !CLZ;
    extern __shared__ __align__(16) unsigned char zs_smem[];
    T* const lds = reinterpret_cast<T*>(zs_smem);
    const int tid = threadIdx.x;

    const int tiles_x = g.nx / TX, tiles_y = g.ny / TY;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile = b % (tiles_x * tiles_y);
    const int Z0 = (b / (tiles_x * tiles_y)) * zc;
    int tx_, ty_;
    zs_tile_xy(tile, tiles_x, patch, tx_, ty_);
    const int X0 = tx_ * TX, Y0 = ty_ * TY;
    const int hw = g.hw, Hh = (int)g.H;
    const int z0 = (int)g.z0, gnz = (int)g.gnz, cz0 = (int)gc.z0;
    const int64_t P = g.P;
    const int qlo = -gz, qhi = (int)g.nz - 1 + gz;  // readable local planes

    // my column of the extended tile; ZS_PSPLIT: wcls = my wave's row parity (even / odd extended rows)
    const int wcls = S::PS ? __builtin_amdgcn_readfirstlane(tid >= S::NPAR ? 1 : 0) : 0;
    const int rt_ = S::PS ? tid - wcls * S::NPAR : tid;
    const int yr_ = S::PS ? 0 : S::yrow(tid);
    const bool on = S::PS ? rt_ < G * (wcls ? YE / 2 : S::YEV) : yr_ >= 0;
    const int gx = on ? (S::PS ? rt_ % G : S::ycol(tid)) : 0, ye = S::PS ? (on ? 2 * (rt_ / G) + wcls : wcls) : (on ? yr_ : 0);
    const int gy = Y0 - H + ye;
    const int m0 = gx * N;
    ZsCol col;
    // LDS row of extended row y: ZS_PSPLIT stores the even rows first, then the odd ones, so that the rows
    // of one wave stay contiguous in LDS (conflict-free vector reads)
    auto lr = [&](int y) { return S::PS ? (y & 1) * S::YEV + (y >> 1) : y; };
    col.lrow = lr(ye) * HWE + m0;
    col.lym = lr(ye > 0 ? ye - 1 : ye) * HWE + m0;
    col.lyp = lr(ye < YE - 1 ? ye + 1 : ye) * HWE + m0;
    col.gm = (X0 - S::HX) / 2 + m0;  // global packed m of my first cell
    col.x_first = gx == 0;
    col.x_last = gx == G - 1;
    col.lxm = col.x_first ? col.lrow : col.lrow - N;
    col.lxp = col.x_last ? col.lrow : col.lrow + N;
    const bool in_xy = on && gy >= 0 && gy < g.ny && col.gm >= 0 && col.gm < hw;
    col.xin = !in_xy || (col.gm > 0 && 2 * (col.gm + N) < g.nx);
    // columns outside the box load from a clamped in-plane position; their results never reach
    // LDS or HBM
    const int cgy = gy < 0 ? 0 : (gy >= g.ny ? g.ny - 1 : gy);
    const int cgm = col.gm < 0 ? 0 : (col.gm > hw - N ? hw - N : col.gm);
#if defined(ZS_HALO_ALIAS)  // timing experiment only (wrong results): the halo's loads read the tile's own lines
    // bit 0: x-halo column groups load from owned columns; bit 1: y-halo rows load from owned rows
    const int agm = (ZS_HALO_ALIAS & 1) ? (gx < S::HXG ? cgm + S::HXG * N : (gx >= G - S::HXG ? cgm - S::HXG * N : cgm)) : cgm;
    const int agy = (ZS_HALO_ALIAS & 2) ? (ye < H ? cgy + H : (ye >= H + TY ? cgy - H : cgy)) : cgy;
    const int goff = agy * hw + agm;
#else
    const int goff = cgy * hw + cgm;  // in-plane offset (nx * ny < 2^31)
#endif
    const bool tile_xy = on && ye >= H && ye < H + TY && gx >= S::HXG && gx < G - S::HXG;
    // ZS_FHALO: the y-halo rows load only the f their stages can use: stage k is needed on rows d <= H - k from the
    // tile, so f1 (red f: stages 1 and 3) only on d <= H - 1 and f2 (black f: stages 2, 4, the residual) only on
    // d <= H - 2; the others keep zeros (their outputs lie outside every later stage's region)
    const int ydist = ye < H ? H - ye : (ye >= H + TY ? ye - (H + TY) + 1 : 0);
    // (POST only: in PRE it measured slower, 335.5 -> 341 us, against POST 435 -> 432 us at 512^3)
    const bool need_f1 = !ZS_FHALO || PRE || ydist <= H - 1, need_f2 = !ZS_FHALO || PRE || ydist <= H - 2;
    const int zlo = Z0 - H;
    ZsDiag<T> dz;
    {
        const int nby = (gy == 0) + (gy == g.ny - 1);  // 0 .. 2 (ny >= 2)
        dz.db = nby == 0 ? op.dg[0] : (nby == 1 ? op.dg[1] : op.dg[2]);
        dz.yb = nby == 0 ? op.ydg[0] : (nby == 1 ? op.ydg[1] : op.ydg[2]);
        dz.de = nby == 0 ? op.dg[1] : (nby == 1 ? op.dg[2] : op.dg[3]);
        dz.ye = nby == 0 ? op.ydg[1] : (nby == 1 ? op.ydg[2] : op.ydg[3]);
        dz.left = col.gm == 0;
        dz.right = col.gm + N == hw;
    }
    // (FWF: the x- and y-combinations of the full weighting follow the residual of plane p - 5 one and two steps later)
    const int p_end = Z0 + zc + (PRE ? (FWF ? 7 : 5) : 3);
    auto inz = [&](int q) { return FAI || (z0 + q >= 0 && z0 + q < gnz); };  // inside the global box
    auto pcl = [&](int q) { return q < qlo ? qlo : (q > qhi ? qhi : q); };
    // ring slot of plane q (q may be negative; ns = 3 as q mod 3)
    auto slot = [&](int off, int ns, int q) {
        const int r = ns == 3 ? ((q % 3) + 3) % 3 : (q & (ns - 1));
        return lds + off + r * SLOT;
    };
    auto nbyz = [&](int q) {
        return CLZ ? 0 : (gy == 0) + (gy == g.ny - 1) + (FAI ? 0 : (z0 + q == 0) + (z0 + q == gnz - 1));
    };
    const int rowpar = (gy + z0) & 1;
    const int wrole = S::YROLE ? __builtin_amdgcn_readfirstlane(S::wave_role(tid >> 6)) : 0;  // (ZS_YROLE)
    const T* const src_black = ZSRC ? nullptr : src + Hh;

    for (int i = tid; i < (int)(S::lds_bytes / sizeof(T)); i += NTL) lds[i] = (T)0;
    __syncthreads();

    // ---- POST: coarse staging ring, plane K in slot K & 3 (planes clamped to the box) ----
    const int Ia = X0 / 2 - 8, Ja = Y0 / 2 - 3;
    auto ckl = [&](int K) { return K < 0 ? 0 : (K >= gc.gnz ? gc.gnz - 1 : K); };
    auto cslot = [&](int K) { return lds + S::OFFC + (K & 3) * S::CSLOT; };
    auto cload = [&](PF& r, int K) {
        K = ckl(K);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t = tid + i * NTL;
            const int J = Ja + t / (S::CI / 2), I = Ia + 2 * (t % (S::CI / 2));
            r.cv[i].v[0] = r.cv[i].v[1] = (T)0;
            if (t < S::CPAIRS && J >= 0 && J < gc.ny && I >= 0 && I < gc.nx) {
                // I even: cells I and I + 1 sit at m = I / 2 of the two colour halves
                const T* row = V + (int64_t)(K - cz0) * gc.P + (int64_t)J * gc.hw + (I >> 1);
                const int ce = (I + J + K) & 1;
                r.cv[i].v[0] = row[ce * gc.H];
                r.cv[i].v[1] = row[(ce ^ 1) * gc.H];
            }
        }
    };
    auto cstore = [&](const PF& r, int K) {
        T* const sl = cslot(ckl(K));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t = tid + i * NTL;
            if (t < S::CPAIRS) vstore<T, 2>(sl + 2 * t, r.cv[i]);  // pair t: cells 2t, 2t + 1 of the region
        }
    };
    auto crow = [&](int K, int J, T (&c)[N + 2]) {  // cells cgm - 1 .. cgm + N of coarse row J, plane K
        const T* const sl = cslot(ckl(K)) + (J - Ja) * S::CI + (cgm - Ia);
        const Vec<T, N> mid = vload<T, N>(sl);
        c[0] = vload_lds_whole<T, N>(sl - N).v[N - 1];
#pragma unroll
        for (int e = 0; e < N; ++e) c[e + 1] = mid.v[e];
        c[N + 1] = vload_lds_whole<T, N>(sl + N).v[0];
    };

    // ST (steady): every plane the step touches lies inside the box, the readable planes and the
    // chunk, so the plane clamps and the box / chunk tests drop out and a step is one basic block
    // the scheduler can interleave (LDS reads of all stages up front).
    // In steady steps z0, Z0 and zc are even (checked before the steady loop), so the parity of p
    // is static within a step pair: zz0 / the caller's p carry it as known low bits and the parity
    // tests below fold away.
    auto prefetch = [&](auto st, PF& r, int p) {
        constexpr bool ST = decltype(st)::value;
        const int zz0 = ST ? (z0 & ~1) : z0;
        // POST: fine plane 2m + 1 is the first to need coarse plane m + 1; it is loaded with the
        // prefetch of plane 2m and put in the ring at the top of step 2m
        if (!PRE && ((zz0 + p) & 1) == 0) cload(r, ((zz0 + p) >> 1) + 1);
        if (ST && !FAI) {  // one 64-bit plane offset, the others by subtraction
#ifdef ZS_NOLOAD
            const int64_t pP = 0, Pz = 0;  // every plane reads plane 0
#else
            const int64_t pP = (int64_t)p * P, Pz = P;
#endif
            if constexpr (ZSRC)
                r.u = vzero<T, N>();
            else
                r.u = gload<T, N, kZsNTL>(src_black + pP + goff);
            if (need_f1) r.f1 = gload<T, N, kZsNTL>(f + (pP - Pz) + goff);
            if (need_f2) r.f2 = gload<T, N, kZsNTL>(f + (pP - 2 * Pz) + Hh + goff);
            if (!PRE && ERR && tile_xy) {  // psiOld of plane p - 4, for the tile's own columns only
                const T* dp = old + (pP - 4 * Pz);
                r.o0 = gload<T, N, kZsNTO>(dp + goff);
                r.o1 = gload<T, N, kZsNTO>(dp + Hh + goff);
            }
        } else {
            if constexpr (ZSRC)
                r.u = vzero<T, N>();
            else
                r.u = gload<T, N, kZsNTL>(src_black + (int64_t)ZS_PLANE(pcl(p)) * P + goff);
            if (need_f1) r.f1 = gload<T, N, kZsNTL>(f + (int64_t)ZS_PLANE(pcl(p - 1)) * P + goff);
            if (need_f2) r.f2 = gload<T, N, kZsNTL>(f + (int64_t)ZS_PLANE(pcl(p - 2)) * P + Hh + goff);
            if (!PRE && ERR && tile_xy) {
                const T* dp = old + (int64_t)pcl(p - 4) * P;
                r.o0 = gload<T, N, kZsNTO>(dp + goff);
                r.o1 = gload<T, N, kZsNTO>(dp + Hh + goff);
            }
        }
    };

    const VT vz = vzero<T, N>();
    // Register rings of four planes: plane q lives in slot (q - zlo) & 3.  Every loop runs whole
    // groups of four steps, so each step knows its slot offset R = (p - zlo) & 3 at compile time and
    // the rings never move (no register rotation).
    VT W0[4], W1[4], W2[4], W3[4], W4[4], FR[4], FB[4];
    T AS[2][N];  // PRE (ZS_RASK): stage 4's askew of the last two steps (plane p - 4 at slot RS & 1)
#pragma unroll
    for (int e = 0; e < N; ++e) AS[0][e] = AS[1][e] = (T)0;
#pragma unroll
    for (int i = 0; i < 4; ++i) W0[i] = W1[i] = W2[i] = W3[i] = W4[i] = FR[i] = FB[i] = vz;
    // W0: A0 black at p-2 .. p; W1: A1 red at p-3 .. p-1; W2: A2 black at p-4 .. p-2;
    // W3: A3 red at p-6 .. p-3; W4: A4 black at p-6 .. p-4; FR: red f (cur.f1) of planes p-5 .. p-2;
    // FB: black f (cur.f2) of planes p-5 .. p-3
    T acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = (T)0;
    double err = 0.0, err1 = 0.0;
    const bool even_row_l = (gy & 1) == 0;
    T* const xbase = lds + S::OFFX + (((ye + (H & 1)) >> 1) * G + gx) * 2 * N;
    auto xs = [&](int q) { return xbase + (q & 1) * (S::XPAIRS * G * 2 * N); };

    // cur: plane p (loaded one step earlier); nxt: the buffer plane p + 1 is loaded into
    // POST: the per-lane half of the interior test of the coarse correction (loop invariant)
    const bool corr_lane = !PRE && (cgy >> 1) + ((cgy & 1) ? 1 : -1) >= 0 && (cgy >> 1) + ((cgy & 1) ? 1 : -1) < gc.ny &&
                           cgm > 0 && cgm + N < gc.nx;
    const bool corr_fast = __all(corr_lane);
    // POST, linear P, steady steps: BQ[K & 1][q][e] = zs_bq of coarse plane K for the black cells of the
    // fine planes of parity 1 ^ q (x parity q ^ (cgy & 1)).  Plane K + 1 is evaluated at odd step 2K + 1,
    // its first reader; fine plane p reads planes K and Kn = K +- 1, the two slots.
    T BQ[2][2][N];
#pragma unroll
    for (int i = 0; i < 2 * 2 * N; ++i) (&BQ[0][0][0])[i] = (T)0;
    const int bq_J = cgy >> 1;
    int bq_Jn = (cgy & 1) ? bq_J + 1 : bq_J - 1;
    const bool bq_oy = !PRE && (bq_Jn < 0 || bq_Jn >= gc.ny);
    if (bq_oy) bq_Jn = bq_J;
    auto bq_fill = [&](auto rp, T (&bq)[2][N], int K) {
        constexpr int RP = decltype(rp)::value;  // static row parity (>= 0) or runtime (-1)
        const int cp = RP >= 0 ? RP : (cgy & 1);
        T c0[N + 2], c1[N + 2];
        crow(K, bq_J, c0);
        crow(K, bq_Jn, c1);
#pragma unroll
        for (int q = 0; q < 2; ++q)
            zs_bq<T, N>(bq[q], c0, c1, q ^ cp, cgm, gc.nx, bq_oy, clc, corr_fast);
    };
    auto step = [&](auto st, auto rt, auto rp, auto ro, const PF& cur, PF& nxt, int p) __attribute__((always_inline)) {
        constexpr bool ST = decltype(st)::value;
        constexpr int RS = decltype(rt)::value;  // (p - zlo) & 3
        (void)ro;
        // my wave's role (ZsShape::wave_role, wave-uniform; every generic step runs the full work)
        const int RO = ST ? wrole : 0;
        // RP >= 0: my wave's row parity rowpar, known statically (ZS_PSPLIT steady steps: z0 and Y0 even, so
        // it is also the parity of gy); -1: per lane
        constexpr int RP = decltype(rp)::value;
        static_assert(RP < 0 || ST, "static row parity in steady steps only");
        auto par = [&](int q) { return RP >= 0 ? ((RP ^ q) & 1) : (rowpar ^ (q & 1)); };
        const bool even_row = RP >= 0 ? RP == 0 : even_row_l;
        // ring slot of plane p - k
        auto sl = [](int k) constexpr { return (RS - k) & 3; };
        // steady: Z0 even, so p's parity is zlo's plus RS
        if (ST) p = (p & ~1) | ((H + RS) & 1);
        const int zz0 = ST ? (z0 & ~1) : z0;
        zs_hold<T, N>(cur.u);
        zs_hold<T, N>(cur.f1);
        zs_hold<T, N>(cur.f2);
        if (!PRE && ERR) {
            zs_hold<T, N>(cur.o0);
            zs_hold<T, N>(cur.o1);
        }
        if (!PRE) {
            zs_hold<T, 2>(cur.cv[0]);
            zs_hold<T, 2>(cur.cv[1]);
        }
        asm volatile("" ::: "memory");
        // POST: the coarse plane cur's prefetch loaded (first read one step on; the slot it replaces
        // was last read three steps back)
        if (!PRE && ((zz0 + p) & 1) == 0) cstore(cur, ((zz0 + p) >> 1) + 1);
        if (ST || p + PFD <= p_end) prefetch(st, nxt, p + PFD);

        // Every LDS read of a step hits a slot filled in the previous step (the writes come after
        // the stages), so the compiler may schedule them as early as registers allow.
        ZsNb<T, N> n1, n2, n3, n4, nr, nk;

        // ---- stage 0: black cells of plane p ----
        VT a0 = cur.u;
        if constexpr (!PRE && ST && LINEAR == 1 && ZS_BQ) {
            // (z0 + Z0) % 4 == 0 in steady steps: K & 1 and p & 1 are static
            constexpr int KS = (RS >> 1) & 1, Q = 1 ^ (RS & 1);
            if constexpr ((RS & 1) != 0) bq_fill(rp, BQ[KS ^ 1], ((zz0 + p) >> 1) + 1);
            const T w0 = (T)0.75, w1 = (T)0.25;
#pragma unroll
            for (int e = 0; e < N; ++e) a0.v[e] = a0.v[e] + (w0 * BQ[KS][Q][e] + w1 * BQ[KS ^ 1][Q][e]);
        } else if (!PRE && (ST || inz(p))) {
            const int J = cgy >> 1, K = (zz0 + p) >> 1;
            int Jn = (cgy & 1) ? J + 1 : J - 1;
            int Kn = ((zz0 + p) & 1) ? K + 1 : K - 1;
            const bool oy = Jn < 0 || Jn >= gc.ny, oz = !ST && (Kn < 0 || Kn >= gc.gnz);
            if (oy) Jn = J;
            if (oz) Kn = K;
            ZsCoarse<T, N> cc;
            crow(K, J, cc.c00);
            if (LINEAR) {
                crow(K, Jn, cc.c10);
                crow(Kn, J, cc.c01);
                crow(Kn, Jn, cc.c11);
            }
            zs_correct<T, N, LINEAR>(a0, cc, 1 ^ ((cgy + zz0 + p) & 1), cgm, gc.nx, oy, oz, clc,
                                     ST ? corr_fast : __all(!oy && !oz && cgm > 0 && cgm + N < gc.nx));
        }
        if (!ST && !inz(p)) a0 = vz;
        W0[sl(0)] = a0;

        // ---- stages 1..4: half-sweep k on plane p - k (red, black, red, black) ----
        zs_nb_load<T, N>(n1, slot(0, 2, p - 1), col);
        VT o1 = zs_relax<T, N, CLZ, ST, TAB>(W0[sl(2)], W0[sl(1)], W0[sl(ZS_NC ? 3 : 0)], n1, cur.f1, col, par(p - 1), nbyz(p - 1), g.nx, op, dz);
        if (!ST && !inz(p - 1)) o1 = vz;
        W1[sl(1)] = o1;
        // (a wave of halo rows d >= 4, role 2, needs stage 1 only: its stages 2..4 would feed no needed cell)
        VT o2 = vz, o3 = vz, o4 = vz;
        if (RO < 2) {
            zs_nb_load<T, N>(n2, slot(S::OFF1, 2, p - 2), col);
            o2 = zs_relax<T, N, CLZ, ST, TAB>(W1[sl(3)], W1[sl(2)], W1[sl(ZS_NC ? 0 : 1)], n2, cur.f2, col, 1 ^ par(p - 2), nbyz(p - 2),
                                         g.nx, op, dz);
            if (!ST && !inz(p - 2)) o2 = vz;
            W2[sl(2)] = o2;
            zs_nb_load<T, N>(n3, slot(S::OFF2, 2, p - 3), col);
            o3 = zs_relax<T, N, CLZ, ST, TAB>(W2[sl(4)], W2[sl(3)], W2[sl(ZS_NC ? 1 : 2)], n3, FR[sl(3)], col, par(p - 3), nbyz(p - 3),
                                         g.nx, op, dz);
            if (!ST && !inz(p - 3)) o3 = vz;
            W3[sl(3)] = o3;
            zs_nb_load<T, N>(n4, slot(S::OFF3, NS3, p - 4), col);
            o4 = zs_relax_a<T, N, CLZ, ST, TAB>(W3[sl(5)], W3[sl(4)], W3[sl(ZS_NC ? 2 : 3)], n4, FB[sl(4)], col, 1 ^ par(p - 4),
                                           nbyz(p - 4), g.nx, op, dz, AS[RS & 1]);
            if (!ST && !inz(p - 4)) o4 = vz;
            W4[sl(4)] = o4;
        }

        // ---- LDS writes (slots no stage of this step reads); columns outside the box stay 0 ----
        if (in_xy) {
            vstore<T, N>(slot(0, 2, p) + col.lrow, a0);
            vstore<T, N>(slot(S::OFF1, 2, p - 1) + col.lrow, o1);
            if (RO < 2) {
                vstore<T, N>(slot(S::OFF2, 2, p - 2) + col.lrow, o2);
                vstore<T, N>(slot(S::OFF3, NS3, p - 3) + col.lrow, o3);
                if (RR || FWF) vstore<T, N>(slot(S::OFF4, 2, p - 4) + col.lrow, o4);
            }
        }

        // ---- the smoothed plane p - 4: red final after stage 3, black after stage 4 ----
        // (the chunk test is wave-uniform: steady steps also run the trapezoid's warm-up before the chunk and
        // its drain after it, which store nothing)
        if (RO == 0) {
            const int q = p - 4;
            if (q >= Z0 && q < Z0 + zc && tile_xy) {
                if (!PRE && ERR) {
#pragma unroll
                    for (int e = 0; e < N; ++e) {
                        // (psi - psiOld)^2 in fp64, fused multiply-add into two accumulators (err
                        // matches the oracle's sum to summation order, not bit for bit)
                        const double d0 = (double)W3[sl(4)].v[e] - (double)cur.o0.v[e];
                        const double d1 = (double)o4.v[e] - (double)cur.o1.v[e];
                        err = __builtin_fma(d0, d0, err);
                        err1 = __builtin_fma(d1, d1, err1);
                    }
                }
                T* dp = dst + (int64_t)q * P;
                // PRE: the red cells are not stored.  Its output is read only by POST, whose stage 0
                // loads the black cells (the first post half-sweep replaces the red ones unread).
                if (!(RR || FWF) || kZsPreRed) gstore<T, N, kZsNTS>(dp + goff, W3[sl(4)]);
                gstore<T, N, kZsNTS>(dp + Hh + goff, o4);
            }
        }

        // ---- PRE: residual + restriction of plane p - 5 (tile rows only: role 0) ----
        if (RR && RO == 0) {
            const int q = p - 5;
            const int pq = par(q);
            if (!kZsRask) zs_nb_load<T, N>(nr, slot(S::OFF3, NS3, q), col);  // red of A4 at q
            zs_nb_load<T, N>(nk, slot(S::OFF4, 2, q), col);                  // black of A4 at q
            T xr[2 * N];
            {
                const T* x = xs(q - 1);  // the odd row's residuals of plane q - 1 (even rows read them)
#pragma unroll
                for (int e = 0; e < 2 * N; ++e) xr[e] = x[e];
            }
            // red cells (x parity pq) see black neighbours, black cells (x parity 1 - pq) red ones
            T rred[N], rblk[N], rr[2][N];  // rr: [x parity][e]
            zs_residual<T, N, CLZ, ST, TAB>(W4[sl(6)], W4[sl(5)], W4[sl(ZS_NC ? 3 : 4)], nk, W3[sl(5)], FR[sl(5)], col, pq, nbyz(q), g.nx, op,
                                   dz, rred);
            // the black cells' neighbours are the red cells of the last step's stage 4 (its askew, ZS_RASK)
            if (kZsRask)
                zs_residual_a<T, N, CLZ, ST, TAB>(AS[(RS & 1) ^ 1], W4[sl(5)], FB[sl(5)], col, 1 ^ pq, nbyz(q), g.nx, op, dz,
                                             rblk);
            else
                zs_residual<T, N, CLZ, ST, TAB>(W3[sl(6)], W3[sl(5)], W3[sl(4)], nr, W4[sl(5)], FB[sl(5)], col, 1 ^ pq, nbyz(q),
                                           g.nx, op, dz, rblk);
#pragma unroll
            for (int e = 0; e < N; ++e) {
                rr[0][e] = pq == 0 ? rred[e] : rblk[e];
                rr[1][e] = pq == 0 ? rblk[e] : rred[e];
            }
            const int dq = q - (ST ? (Z0 & ~1) : Z0);
            if (dq >= 0 && dq <= zc && tile_xy)
                zs_restrict_avg<T, N>(rr, xr, acc, dq, zc, even_row, xs(q), R, (zz0 + q - 1) >> 1, gy >> 1, col.gm, cz0, gc);
        }
        // ---- PRE, FWF: residual of plane p - 5 into RX, the x-combination of plane p - 6, the y-combination and the
        // coarse planes of plane p - 7 (fw_eval's order; cells outside the box weigh 0) ----
        if constexpr (FWF) {
            const int q = p - 5;
            const int pq = par(q);
            if (!kZsRask) zs_nb_load<T, N>(nr, slot(S::OFF3, NS3, q), col);
            zs_nb_load<T, N>(nk, slot(S::OFF4, 2, q), col);
            T rred[N], rblk[N];
            zs_residual<T, N, CLZ, ST, TAB>(W4[sl(6)], W4[sl(5)], W4[sl(ZS_NC ? 3 : 4)], nk, W3[sl(5)], FR[sl(5)], col, pq, nbyz(q), g.nx, op,
                                   dz, rred);
            if (kZsRask)
                zs_residual_a<T, N, CLZ, ST, TAB>(AS[(RS & 1) ^ 1], W4[sl(5)], FB[sl(5)], col, 1 ^ pq, nbyz(q), g.nx, op, dz,
                                             rblk);
            else
                zs_residual<T, N, CLZ, ST, TAB>(W3[sl(6)], W3[sl(5)], W3[sl(4)], nr, W4[sl(5)], FB[sl(5)], col, 1 ^ pq, nbyz(q),
                                           g.nx, op, dz, rblk);
            const bool rin = in_xy && (ST || inz(q));  // (the residuals of cells outside the box weigh 0)
            // RX: the group's 2N cells in x order, the low N at t N and the high N at RXH + t N (t = ye G + gx), so
            // that every access is one conflict-free 16-byte vector per lane
            constexpr int RXH = S::RXSLOT / 2;
            const int t = ye * G + gx;
            if (ydist <= 1) {  // (rows within one of the tile: the only ones the x-combination reads)
                VT x[2];  // x order: cell 2 (gm + e) + parity
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    x[(2 * e) / N].v[(2 * e) % N] = rin ? (pq ? rblk[e] : rred[e]) : (T)0;
                    x[(2 * e + 1) / N].v[(2 * e + 1) % N] = rin ? (pq ? rred[e] : rblk[e]) : (T)0;
                }
                T* const rxw = lds + S::OFFRX + (p & 1) * S::RXSLOT + t * N;
                vstore<T, N>(rxw, x[0]);
                vstore<T, N>(rxw + RXH, x[1]);
            }
            const T wfv = (T)3 - clc, w3 = (T)3;
            // the x-combination of plane p - 6 (written to RX one step ago) for the tile's coarse columns, rows within
            // one of the tile: fine cells 2I - 1 .. 2I + 2 of coarse I = gm + e
            const bool tile_x = gx >= S::HXG && gx < G - S::HXG;
            if (tile_x && ydist <= 1) {
                const T* rxr = lds + S::OFFRX + ((p - 1) & 1) * S::RXSLOT;
                T x[2 * N + 2];
                const VT lo = vload_lds_whole<T, N>(rxr + t * N), hi = vload_lds_whole<T, N>(rxr + RXH + t * N);
                x[0] = vload_lds_whole<T, N>(rxr + RXH + (t - 1) * N).v[N - 1];
                x[2 * N + 1] = vload_lds_whole<T, N>(rxr + (t + 1) * N).v[0];
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    x[1 + e] = lo.v[e];
                    x[1 + N + e] = hi.v[e];
                }
                const int cxn = g.nx >> 1;
                VT ax;
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const int I = col.gm + e;
                    ax.v[e] = fw_axis(x[2 * e], x[2 * e + 1], x[2 * e + 2], x[2 * e + 3], I == 0 ? wfv : w3,
                                      I == cxn - 1 ? wfv : w3);
                }
                vstore<T, N>(lds + S::OFFAX + (p & 1) * S::AXSLOT + t * N, ax);
            }
            // the y-combination of plane p - 7 (its x-combinations were written one step ago) for every coarse cell
            // group of the tile (coarse row J: fine rows 2J - 1 .. 2J + 2), then coarse plane K when p - 7 = 2K + 2.
            // The TY / 2 x TX / (2 N) items run in wave FWY (ZsShape: the wave that shares no SIMD when the
            // workgroup has 4 k + 3 waves), each item on the same lane every step (the AY ring is lane-private)
            if (tid >= S::FWY * 64 && tid < S::FWY * 64 + 64) {
                const T* axr = lds + S::OFFAX + ((p - 1) & 1) * S::AXSLOT;
                const int cyn = g.ny >> 1, q2 = p - 7;
                const int dq2 = q2 - 2 - (ST ? (Z0 & ~1) : Z0);  // 2K - z0 - Z0 for the coarse plane K ending at q2
                const bool emit = dq2 >= 0 && dq2 < zc && (dq2 & 1) == 0;
                const int K = (z0 + q2 - 2) >> 1;  // global coarse plane
                const T wk0 = K == 0 ? wfv : w3, wk1 = K == gc.gnz - 1 ? wfv : w3;
                constexpr int CG = TX / (2 * N);  // coarse groups per coarse row
#pragma unroll
                for (int k = 0; k < S::FWYI; ++k) {
                    const int i = tid - S::FWY * 64 + 64 * k;
                    const int jl = i / CG, cg = i % CG;
                    const int J = (Y0 >> 1) + jl, ty = (H + 2 * jl) * G + S::HXG + cg;
                    const VT a0 = vload_lds_whole<T, N>(axr + (ty - G) * N), a1 = vload_lds_whole<T, N>(axr + ty * N),
                             a2 = vload_lds_whole<T, N>(axr + (ty + G) * N), a3 = vload_lds_whole<T, N>(axr + (ty + 2 * G) * N);
                    const T wj0 = J == 0 ? wfv : w3, wj1 = J == cyn - 1 ? wfv : w3;
                    VT ay;
#pragma unroll
                    for (int e = 0; e < N; ++e) ay.v[e] = ((a0.v[e] + wj0 * a1.v[e]) + wj1 * a2.v[e]) + a3.v[e];
                    T* const ayb = lds + S::OFFAY + i * N;
                    vstore<T, N>(ayb + (q2 & 3) * S::AYSLOT, ay);
                    if (emit) {
                        const VT b0 = vload_lds_whole<T, N>(ayb + ((q2 - 3) & 3) * S::AYSLOT),
                                 b1 = vload_lds_whole<T, N>(ayb + ((q2 - 2) & 3) * S::AYSLOT),
                                 b2 = vload_lds_whole<T, N>(ayb + ((q2 - 1) & 3) * S::AYSLOT);
                        // coarse cells I = gm .. gm + N - 1 (gm even): the even ones at m = gm / 2 .. of one colour
                        // half, the odd ones of the other
                        const int gm = X0 / 2 + cg * N;
                        T* rowc = R + (int64_t)(K - cz0) * gc.P + (int64_t)J * gc.hw + (gm >> 1);
                        Vec<T, N / 2> ev, od;
#pragma unroll
                        for (int e = 0; e < N; ++e) {
                            const T az = ((b0.v[e] + wk0 * b1.v[e]) + wk1 * b2.v[e]) + ay.v[e];
                            if (e & 1)
                                od.v[e >> 1] = (T)(1.0 / 512.0) * az;
                            else
                                ev.v[e >> 1] = (T)(1.0 / 512.0) * az;
                        }
                        const int ce = (gm + J + K) & 1;
                        vstore<T, N / 2>(rowc + ce * gc.H, ev);
                        vstore<T, N / 2>(rowc + (ce ^ 1) * gc.H, od);
                    }
                }
            }
        }
        FR[sl(1)] = cur.f1;  // red f of plane p - 1 (replaces p - 5, read above)
        FB[sl(2)] = cur.f2;  // black f of plane p - 2
        lds_barrier();
    };

    const std::false_type GEN;
    const std::true_type STY;
    PF pb[NPF];
#pragma unroll
    for (int k = 0; k < NPF; ++k) pb[k].f1 = pb[k].f2 = vz;  // (the halo rows that skip f loads keep zeros)
    // FACE (cl != 0 levels, whose chunks are short): no step for nothing at the box's z faces.  A chunk at the lower
    // face starts at pg, past the whole groups of steps in which every stage's plane lies below the box (they move
    // zeros: the rings and the LDS slots start as zeros), and the steady range [ps, pe] is not rounded to whole
    // groups: the group that holds ps is generic up to ps - 1 and steady from ps, the one that holds pe is steady up
    // to pe and generic after it.  A 32-plane POST chunk runs 5 generic steps at either face (the steps with a stage
    // on or outside the face plane) where it ran 12 and 8.  cl = 0 levels keep whole groups (the bound tests cost
    // level 0's long steady loop more than its 4 generic steps, see k_zs_split).
    constexpr bool FACE = !CLZ && !ZS_ALL_GENERIC && !FAI;
    int pg = zlo;
    if constexpr (FACE) {
        if (-z0 - zlo >= UNR) pg = zlo + (-z0 - zlo) / UNR * UNR;
    }
    if (!PRE) {  // the coarse planes the first fine plane needs
        const int K = (z0 + (FACE ? pg : zlo)) >> 1;
        for (int k = K - 1; k <= K + 1; ++k) {
            cload(pb[0], k);
            cstore(pb[0], k);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < PFD; ++k) prefetch(GEN, pb[k], (FACE ? pg : zlo) + k);
    // steady steps [ps, pe]: stages inside the box (z0 + p - 5 >= 1, z0 + p < gnz) and the prefetched planes
    // (p + PFD .. p - 4) readable; the chunk's warm-up and drain steps are steady too (their stores are skipped
    // by the uniform chunk test), so a chunk away from the box faces runs no generic step at all (the short
    // chunks of the coarser fused levels were ~45 % generic steps before)
    int ps = FACE ? pg : zlo, pe = p_end;
    if constexpr (!FACE && !FAI) {
        ps = ps > 6 - z0 ? ps : 6 - z0;  // PRE's residual plane p - 5 off the z face (steady diagonals have no z face)
        ps = ps > qlo + 4 ? ps : qlo + 4;
        pe = pe < gnz - (PRE ? 1 : 2) - z0 ? pe : gnz - (PRE ? 1 : 2) - z0;  // POST: Kn inside the coarse box
        pe = pe < qhi - PFD ? pe : qhi - PFD;
        ps += (UNR - (ps - zlo) % UNR) % UNR;  // whole groups of UNR steps in the prologue
        pe -= (pe - ps + 1) % UNR;             // and in the steady part
        // no steady part (the epilogue takes all) without a whole group or with odd z0 / Z0 (static parity)
        // POST with the BQ cache: (z0 + Z0) % 4 == 0 as well (static parity of the coarse plane)
        if (ZS_ALL_GENERIC || pe < ps || ((z0 | Z0) & 1) || (!PRE && LINEAR == 1 && ZS_BQ && ((z0 + Z0) & 3))) ps = pe = zlo - 1;
    } else {
        if (!FAI) {  // FACE: POST's last stage's plane p - 4 off the z face
            const int pz = (PRE ? 6 : 5) - z0;
            ps = ps > pz ? ps : pz;
            pe = pe < gnz - (PRE ? 1 : 2) - z0 ? pe : gnz - (PRE ? 1 : 2) - z0;
        }
        ps = ps > qlo + 4 ? ps : qlo + 4;
        pe = pe < qhi - PFD ? pe : qhi - PFD;
        if (!FACE) {
            ps += (UNR - (ps - zlo) % UNR) % UNR;
            pe -= (pe - ps + 1) % UNR;
        }
        if (pe < ps || ((z0 | Z0) & 1) || (!PRE && LINEAR == 1 && ZS_BQ && ((z0 + Z0) & 3))) {
            ps = FACE ? p_end + 1 : zlo - 1;  // (FACE: the prologue's generic steps take all)
            pe = FACE ? p_end : zlo - 1;
        }
    }
    int p = FACE ? pg : zlo;
    const std::integral_constant<int, -1> RPL;
    // UNR steps from p0 (p0 - zlo a multiple of UNR): ring slot k & 3, buffers k % NPF and (k + PFD) % NPF;
    // steps past plim are skipped (epilogue)
    const std::integral_constant<int, 0> RO0;
    auto group = [&](auto st, auto rp, auto ro, int p0, int plim) __attribute__((always_inline)) {
        zs_unroll<UNR>([&](auto kk) __attribute__((always_inline)) {
            constexpr int k = decltype(kk)::value;
            if (k == 0 || p0 + k <= plim)
                step(st, std::integral_constant<int, (k & 3)>(), rp, ro, pb[k % NPF], pb[(k + PFD) % NPF], p0 + k);
        });
    };
    // FACE: the steps pfirst .. plim of the group from p0
    auto part = [&](auto st, auto rp, auto ro, int p0, int pfirst, int plim) __attribute__((always_inline)) {
        zs_unroll<UNR>([&](auto kk) __attribute__((always_inline)) {
            constexpr int k = decltype(kk)::value;
            if (p0 + k >= pfirst && p0 + k <= plim)
                step(st, std::integral_constant<int, (k & 3)>(), rp, ro, pb[k % NPF], pb[(k + PFD) % NPF], p0 + k);
        });
    };
    if constexpr (FACE) {
        for (; p + UNR <= ps; p += UNR) group(GEN, RPL, RO0, p, p + UNR);
        if (p < ps) part(GEN, RPL, RO0, p, p, ps - 1);  // (p stays: the start of the group that holds ps)
    } else {
        for (; p < ps; p += UNR) group(GEN, RPL, RO0, p, p + UNR);
    }
    auto steady = [&](auto rp, auto ro) __attribute__((always_inline)) {
        if constexpr (!PRE && LINEAR == 1 && ZS_BQ) {
            if (FACE ? ps <= pe : p <= pe) {  // the first steady step (even, K & 1 == 0) reads coarse planes K and K - 1
                const int K = (z0 + p) >> 1;
                bq_fill(rp, BQ[0], K);
                // (FACE: the steady steps may begin at the group's third or fourth step, which read K + 1)
                bq_fill(rp, BQ[1], FACE && ps - p >= 2 ? K + 1 : K - 1);
            }
        }
        for (; p <= pe; p += UNR) {
#ifdef ZS_STAMP // timing experiment (wrong results): POST's wall clock every 16 steps into R (level 1's f)
            if (!PRE && tid == 0 && ((p - zlo) & 15) == 0 && (p - zlo) / 16 < 32) {
                const unsigned long long w = wall_clock64();
                float* out = reinterpret_cast<float*>(R) + 64 * (int)blockIdx.x + 2 * ((p - zlo) / 16);
                out[0] = __uint_as_float((unsigned)(w & 0xffffffffu));
                out[1] = __uint_as_float((unsigned)(w >> 32));
            }
#endif
            // (FACE: every steady step behind its bound tests.  A second copy of the group without them for the whole
            // groups, chosen inside this loop, made the fp32 cl != 0 instantiations spill (POST 168 VGPRs + 34 spilled);
            // as loops of their own, head / whole groups / tail, the 256^3 POST measured 63.3 against 62.3 us)
            if constexpr (FACE)
                part(STY, rp, ro, p, ps, pe);
            else
                group(STY, rp, ro, p, p + UNR);
        }
    };
    if constexpr (S::PS) {  // wave-uniform: one copy of the steady loop per row parity
        if (((H + wcls) & 1) == 0)
            steady(std::integral_constant<int, 0>(), RO0);
        else
            steady(std::integral_constant<int, 1>(), RO0);
    } else {
        steady(RPL, RO0);
    }
    if constexpr (FACE) {  // from pe + 1, in the group that holds it
        for (p = pg + (pe + 1 - pg) / UNR * UNR; p <= p_end; p += UNR) part(GEN, RPL, RO0, p, pe + 1, p_end);
    } else {
        for (; p <= p_end; p += UNR) group(GEN, RPL, RO0, p, p_end);
    }
    if constexpr (ERR && !PRE) block_partial_t<NTL>(err + err1, partials);  // (PRE: ERR is ZSRC, no partials)
}

// ---- what the launchers of k_zs and of its stage-split variants share (host) ----

// Tile order of a launch with more tiles than run at once (FusedTuning::patch_pre / patch_post): consecutive
// tiles of an XCD's band as px x py patches instead of whole tile rows, so that the y neighbours whose halo
// rows a tile reads stream through z at the same time.  Returns px | py << 8, or 0 (tile rows).
inline int zs_patch(int patch, int tiles_x, int tiles_y, unsigned nb)
{
    if (patch == -1) patch = tiles_x * tiles_y >= 4096 ? 4 | (8 << 8) : 0;  // POST's default (FusedTuning)
    const int px = patch & 255, py = patch >> 8;
    if (!patch || tiles_x % px || tiles_y % py || nb <= 512) return 0;
    return patch;
}

// The workgroups of a launch on tile S (one per tile and z-chunk, ntl threads each) and their order (zs_patch with
// the phase's FusedTuning setting); with FusedArgs::info set, the launch's grid goes there (the launcher adds the
// kernel's name).
struct ZsGrid {
    unsigned nb;
    int patch;
};
template <typename S>
ZsGrid zs_grid(const FusedArgs& a, bool pre, int ntl)
{
    ZsGrid gr;
    gr.nb = (unsigned)((a.g.nx / S::TX) * (a.g.ny / S::TY) * (a.g.nz / a.zc));
    gr.patch = zs_patch(pre ? a.tu.patch_pre : a.tu.patch_post, a.g.nx / S::TX, a.g.ny / S::TY, gr.nb);
    if (a.info) a.info->grid = (int64_t)gr.nb * ntl;
    return gr;
}

// ---- k_zs's launcher, the dispatch of a 3D phase and the dynamic-LDS attributes: instantiated per real type by
// mgp_zs.hip (float) and mgp_zs_f64.hip (double), so that neither unit's compile dominates the build ----

template <typename T, bool PRE, int LINEAR, bool ERR, bool CLZ, bool WIDE = false>
static hipError_t zs_launch(const FusedArgs& a, hipStream_t s)
{
    using S = ZsShape<T, PRE, CLZ, WIDE, PRE && LINEAR == 2>;
    const Op<T, 3> op = make_op<T, 3>(a.h, a.cl);
    const ZsGrid gr = zs_grid<S>(a, PRE, S::NTL);
    if (a.info)  // rocprofv3's spelling of the instantiation
        std::snprintf(a.info->name, sizeof a.info->name, "k_zs<%s, %s, %d, %s, %s, %s>", sizeof(T) == 4 ? "float" : "double",
                      tf(PRE), LINEAR, tf(ERR), tf(CLZ), tf(WIDE));
    k_zs<T, PRE, LINEAR, ERR, CLZ, WIDE><<<gr.nb, S::NTL, S::lds_bytes, s>>>((const T*)a.src, (const T*)a.f, (T*)a.dst,
                                                                              (const T*)(a.old ? a.old : a.dst), (T*)a.R,
                                                                              (const T*)a.V, a.partials, a.g, a.gc, op,
                                                                              (T)a.clc, a.zc, a.ghost, gr.patch);
    return hipGetLastError();
}

// POST's wide tile (ZsTile::TXPOST_W): fp32, cl = 0 (or any level with ZS_WIDE_CL: on the 256^3 level of the
// 512^3 box measured +10-16 us per cycle, off), a box it divides, FusedTuning::wide
#ifndef ZS_WIDE_CL
#define ZS_WIDE_CL 0
#endif
inline bool zs_wide(int rb, const Geo& g, bool clz, const FusedTuning& tu)
{
    if (rb != 4 || (!clz && !ZS_WIDE_CL) || !tu.wide) return false;
    return g.nx % ZsTile<float>::TXPOST_W == 0 && g.ny % ZsTile<float>::TYPOST_W == 0;
}

template <typename T, bool CLZ>
static hipError_t fused_dispatch(const FusedArgs& a, hipStream_t s)
{
    const bool err = a.partials != nullptr;
#ifdef ZS_CL_AS_CLZ  // timing experiment only (wrong at the box faces): cl != 0 PRE runs the cl = 0 code
    if (a.pre) return a.linear ? zs_launch<T, true, 1, false, true>(a, s) : zs_launch<T, true, 0, false, true>(a, s);
#endif
    if constexpr (std::is_same<T, float>::value && CLZ) {  // the full weighting fused into PRE (fused_fwf_supported)
        if (a.pre && a.linear == 2)
            return a.src ? zs_launch<T, true, 2, false, CLZ>(a, s) : zs_launch<T, true, 2, true, CLZ>(a, s);
    }
    if (a.pre && a.linear == 2) return hipErrorInvalidValue;
    if constexpr (std::is_same<T, float>::value && CLZ) {
        if (a.pre && !a.linear && a.tu.split) return launch_zs_split(a, s);
    }
    if constexpr (std::is_same<T, float>::value && !CLZ) {  // (a warm guess stays on k_zs: that variant would spill)
        if (a.pre && !a.linear && !a.src && a.tu.split && a.tu.split_cl) return launch_zs_split_cl(a, s);
    }
    if (a.pre && !a.src)  // a fresh zero guess (ERR marks it in PRE)
        return a.linear ? zs_launch<T, true, 1, true, CLZ>(a, s) : zs_launch<T, true, 0, true, CLZ>(a, s);
    if (a.pre) return a.linear ? zs_launch<T, true, 1, false, CLZ>(a, s) : zs_launch<T, true, 0, false, CLZ>(a, s);
    if constexpr (std::is_same<T, float>::value && CLZ) {
        if (zs_wide(4, a.g, true, a.tu)) {
            // (the split POST runs on this tile: zs_split_post_launch's static_assert)
            if (a.linear && a.tu.split_post && (int64_t)a.g.nx * a.g.ny * a.g.nz >= a.tu.split_post_min_cells)
                return launch_zs_split_post(a, s);
            if (a.linear)
                return err ? zs_launch<T, false, 1, true, CLZ, true>(a, s) : zs_launch<T, false, 1, false, CLZ, true>(a, s);
            return err ? zs_launch<T, false, 0, true, CLZ, true>(a, s) : zs_launch<T, false, 0, false, CLZ, true>(a, s);
        }
    }
    if constexpr (std::is_same<T, float>::value && !CLZ && ZS_WIDE_CL) {
        if (!err && zs_wide(4, a.g, false, a.tu))
            return a.linear ? zs_launch<T, false, 1, false, CLZ, true>(a, s) : zs_launch<T, false, 0, false, CLZ, true>(a, s);
    }
    if (a.linear) return err ? zs_launch<T, false, 1, true, CLZ>(a, s) : zs_launch<T, false, 1, false, CLZ>(a, s);
    return err ? zs_launch<T, false, 0, true, CLZ>(a, s) : zs_launch<T, false, 0, false, CLZ>(a, s);
}

template <typename T, bool CLZ>
static hipError_t fused_attr()
{
    const int pre = (int)ZsShape<T, true, CLZ>::lds_bytes, post = (int)ZsShape<T, false, CLZ>::lds_bytes;
    const auto A = hipFuncAttributeMaxDynamicSharedMemorySize;
    if constexpr (std::is_same<T, float>::value && CLZ) {
        const int w = (int)ZsShape<T, true, CLZ, false, true>::lds_bytes;
        hipError_t e = hipFuncSetAttribute((const void*)k_zs<T, true, 2, false, CLZ>, A, w);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, true, 2, true, CLZ>, A, w);
        if (e != hipSuccess) return e;
    }
    if constexpr (std::is_same<T, float>::value && CLZ) {
        const int w = (int)ZsShape<T, false, CLZ, true>::lds_bytes;
        hipError_t e = hipFuncSetAttribute((const void*)k_zs<T, false, 0, false, CLZ, true>, A, w);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, false, 0, true, CLZ, true>, A, w);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, false, 1, false, CLZ, true>, A, w);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, false, 1, true, CLZ, true>, A, w);
        if (e != hipSuccess) return e;
    }
    if constexpr (std::is_same<T, float>::value && !CLZ && ZS_WIDE_CL) {
        const int w = (int)ZsShape<T, false, CLZ, true>::lds_bytes;
        hipError_t e = hipFuncSetAttribute((const void*)k_zs<T, false, 0, false, CLZ, true>, A, w);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, false, 1, false, CLZ, true>, A, w);
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipFuncSetAttribute((const void*)k_zs<T, true, 0, false, CLZ>, A, pre);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, true, 1, false, CLZ>, A, pre);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, true, 0, true, CLZ>, A, pre);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, true, 1, true, CLZ>, A, pre);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, false, 0, false, CLZ>, A, post);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, false, 0, true, CLZ>, A, post);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, false, 1, false, CLZ>, A, post);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs<T, false, 1, true, CLZ>, A, post);
    return e;
}

}  // namespace

}  // namespace mgp
