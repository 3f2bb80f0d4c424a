// mgp_tail.hip — the coarse-level tail: the sub-cycle below one level as a single one-workgroup launch with every
// level in LDS (k_tail: any shapes; k_tail_c: compile-time level shapes), its launcher and dynamic-LDS attributes.
#include "mgp_cell.h"

#include <cstdlib>

namespace mgp {
namespace {

// ---- coarse-level tail ----------------------------------------------------------------------
//
// The levels at and below ~16^3 cost one launch (3-5 us) per piece while their work is a few
// thousand cells.  k_tail runs the whole sub-cycle below level T — the ops of cycle_rec(T, ...)
// that the host recorded into TailSpec::ops — in ONE workgroup with every level resident in LDS
// (same packed layout, ghost planes zero), a __syncthreads() between dependent phases.  The
// per-cell arithmetic is the scalar kernels' (half_item / resrestrict_item / prolong_item), so
// results are bit-identical to the launch-per-piece path.

// 1024 threads = 16 waves on the CU; fp64 gets 512 so the kernel keeps 256 VGPRs without spills
template <typename T>
#ifndef TAIL_THREADS_F32
#define TAIL_THREADS_F32 1024
#endif
constexpr int tail_threads() { return sizeof(T) == 4 ? TAIL_THREADS_F32 : 512; }

template <typename T, int DIM>
struct TailArgs {
    int nlev, nops, jacobi, zero0;  // zero0: level 0's u is a fresh zero guess (not read)
    int fw;                          // full-weighting restriction (TAIL_RR)
    // bit l: the program reads level l's u / f before it writes them (copied in; the others start as 0), and writes
    // level l's f (copied out; u is always copied out)  (tail_io_masks)
    uint32_t in_u, in_f, out_f;
    int64_t off[kTailMaxLevels];     // element offset of the level's LDS region
    int64_t region[kTailMaxLevels];  // elements of one LDS array of the level (ghost planes included)
    T* u[kTailMaxLevels];            // global interior plane 0 of u / f
    T* f[kTailMaxLevels];
    Geo g[kTailMaxLevels];
    Op<T, DIM> op[kTailMaxLevels];
    uint32_t ops[kTailMaxOps];
};

template <typename T, int DIM, int LINEAR>
__global__ __launch_bounds__(tail_threads<T>()) void k_tail(const TailArgs<T, DIM> a)
{
    constexpr int kTailThreads = tail_threads<T>();
    extern __shared__ __align__(16) unsigned char tail_smem[];
    T* const lds = reinterpret_cast<T*>(tail_smem);
    constexpr int G = DIM == 3 ? kGhost3D : 0;
    const int tid = threadIdx.x;
    // level l: u at off, f at off + region, Jacobi target at off + 2 region
#ifndef TAIL_NOCOPYIN  // timing experiment only: results are wrong
    for (int l = 0; l < a.nlev; ++l) {
        const Geo& g = a.g[l];
        T* U = lds + a.off[l];
        T* F = U + a.region[l];
        const int64_t lo = G * g.P, n = g.nz * g.P;
        for (int64_t e = tid; e < a.region[l]; e += kTailThreads) {
            const int64_t ie = e - lo;
            const bool in = ie >= 0 && ie < n;
            U[e] = in && ((a.in_u >> l) & 1) ? a.u[l][ie] : (T)0;
            F[e] = in && ((a.in_f >> l) & 1) ? a.f[l][ie] : (T)0;
            if (a.jacobi) U[e + 2 * a.region[l]] = (T)0;
        }
    }
#endif
    __syncthreads();
#ifdef TAIL_PROF  // timing experiment: shader cycles per op into f of the first level (tools/tail_prof.py)
    __shared__ float tprof[128];
    __shared__ long long tlast;
#endif
    unsigned alt = 0;  // Jacobi: bit l = level l's iterate currently lives in its second array
    auto cur = [&](int l) { return lds + a.off[l] + G * a.g[l].P + (((alt >> l) & 1) ? 2 * a.region[l] : 0); };
    auto rhs = [&](int l) { return lds + a.off[l] + a.region[l] + G * a.g[l].P; };
#ifdef TAIL_NOOPS  // timing experiment only: results are wrong
    for (int pc = 0; pc < 0; ++pc) {
#else
    for (int pc = 0; pc < a.nops; ++pc) {
#endif
#ifdef TAIL_PROF
        if (tid == 0) {
            const long long now = (long long)__builtin_amdgcn_s_memtime();
            if (pc > 0 && pc <= 128) tprof[pc - 1] = (float)(now - tlast);
            tlast = now;
        }
#endif
        const uint32_t w = a.ops[pc];
        const int op = (int)(w & 15), l = (int)((w >> 4) & 15), arg = (int)(w >> 8);
        const Geo g = a.g[l];
        const int64_t half = g.H * g.nz;
        if (op == TAIL_SMOOTH) {
            for (int sw = 0; sw < arg; ++sw) {
                T* U = cur(l);
                const T* F = rhs(l);
                T v;
                if (a.jacobi) {  // both colours from the old iterate into the other array
                    T* D = lds + a.off[l] + G * g.P + (((alt >> l) & 1) ? 0 : 2 * a.region[l]);
                    for (int64_t it = tid; it < 2 * half; it += kTailThreads) {
                        const int c = it >= half;
                        half_item<T, DIM>(U, F, D, g, c, a.op[l], it - c * half, &v);
                    }
                    alt ^= 1u << l;
                    __syncthreads();
                } else {
                    for (int c = 0; c < 2; ++c) {
                        for (int64_t it = tid; it < half; it += kTailThreads) half_item<T, DIM>(U, F, U, g, c, a.op[l], it, &v);
                        __syncthreads();
                    }
                }
            }
        } else if (op == TAIL_RR) {
            const int64_t n = resrestrict_items<T, DIM>(g);
            if (a.fw) {  // full weighting: every fine residual evaluated where a coarse cell reads it
                const Geo gc = a.g[l + 1];
                const T* U = cur(l);
                const T* F = rhs(l);
                const T wf = (T)3 - a.op[l + 1].cl;
                auto get = [&](int i, int j, int64_t k) { return residual_at<T, DIM>(U, F, g, a.op[l], i, j, k); };
                for (int64_t it = tid; it < n; it += kTailThreads) {
                    const int cx = g.nx >> 1, cy = g.ny >> 1;
                    const int I = (int)(it % cx), J = (int)((it / cx) % cy);
                    const int64_t K = it / ((int64_t)cx * cy);
                    rhs(l + 1)[pidx(gc, I, J, K)] = fw_eval<T, DIM>(get, g, gc, wf, I, J, K);
                }
            } else {
                for (int64_t it = tid; it < n; it += kTailThreads)
                    resrestrict_item<T, DIM>(cur(l), rhs(l), rhs(l + 1), g, a.g[l + 1], a.op[l], it);
            }
            __syncthreads();
        } else if (op == TAIL_ZERO) {
            T* U = cur(l);
            for (int64_t e = tid; e < g.nz * g.P; e += kTailThreads) U[e] = (T)0;
            __syncthreads();
        } else if (op == TAIL_PROLONG) {
            for (int64_t it = tid; it < 2 * half; it += kTailThreads) {
                const int c = it >= half;
                prolong_item<T, DIM, LINEAR>(cur(l), cur(l + 1), g, a.g[l + 1], a.op[l + 1].cl, c, it - c * half);
            }
            __syncthreads();
        }
    }
#ifdef TAIL_PROF
    if (tid == 0) {
        const long long now = (long long)__builtin_amdgcn_s_memtime();
        if (a.nops <= 128) tprof[a.nops - 1] = (float)(now - tlast);
        for (int i = 0; i < 128 && i < a.nops; ++i) rhs(0)[i] = (T)tprof[i];
    }
    __syncthreads();
#endif
    for (int l = 0; l < a.nlev; ++l) {
        const T* U = cur(l);
        const T* F = rhs(l);
        const int64_t n = a.g[l].nz * a.g[l].P;
        const bool st_f = (a.out_f >> l) & 1;
        for (int64_t e = tid; e < n; e += kTailThreads) {
            a.u[l][e] = U[e];
            if (st_f) a.f[l][e] = F[e];
        }
    }
}

// ---- coarse tail with compile-time level shapes (k_tail_c) -------------------------------------
//
// The same op program as k_tail for a red/black tail whose first level has one of the compile-time shapes of
// MGP_TC_SHAPES below (the cubic / square tails of cubic / square boxes, and the tails of the slab-shaped boxes: one
// rank's slab of configs[3] / configs[4] ends in 32 x 32 x 4 -> 16 x 16 x 2 -> 8 x 8 x 1, the weak-scaling box
// 512 x 512 x 512 N in 8 x 8 x 8 N ... 1 x 1 x N).  Level l is (TX >> l, TY >> l, TZ >> l), down to the first
// level with an axis of one cell.  Each level lives in LDS as an unpacked (nx+2)(ny+2)(nz+2) array with a zero
// halo (the Dirichlet ghost), so a cell's neighbours are fixed offsets, every loop bound and index is a
// compile-time constant and no box test is needed.  The per-cell arithmetic is half_item's / residual_at +
// resrestrict_item's / prolong_value's, so results are bit-identical to k_tail and to the launch-per-piece path.
template <int DIM, int NX, int NY, int NZ>
struct TcLev {
    static constexpr int W = NX + 2, WY = NY + 2, WZ = NZ + 2, P = DIM == 3 ? W * WY * WZ : W * WY;
    static constexpr int CELLS = DIM == 3 ? NX * NY * NZ : NX * NY;
    static constexpr int SZ = W * WY;  // z stride
    static __device__ __forceinline__ int idx(int i, int j, int k)
    {
        return DIM == 3 ? ((k + 1) * WY + (j + 1)) * W + (i + 1) : (j + 1) * W + (i + 1);
    }
    static __device__ __forceinline__ int nb(int i, int j, int k)  // faces on the box boundary
    {
        return (i == 0) + (i == NX - 1) + (j == 0) + (j == NY - 1) + (DIM == 3 ? (k == 0) + (k == NZ - 1) : 0);
    }
};
template <int T0, int L>
constexpr int tc_dim_at() { return (T0 >> L) > 0 ? (T0 >> L) : 1; }
// level count of a top shape: the levels down to the first one with an axis of one cell
template <int DIM, int TX, int TY, int TZ>
constexpr int tc_levels()
{
    int m = TX < TY ? TX : TY;
    if (DIM == 3 && TZ < m) m = TZ;
    int n = 1;
    for (int t = m; t > 1; t >>= 1) ++n;
    return n;
}
template <int DIM, int TX, int TY, int TZ>
constexpr int tc_off(int l)  // element offset of level l's (u, f) pair
{
    int o = 0;
    for (int q = 0; q < l; ++q) {
        const int wx = (TX >> q > 0 ? TX >> q : 1) + 2, wy = (TY >> q > 0 ? TY >> q : 1) + 2,
                  wz = (TZ >> q > 0 ? TZ >> q : 1) + 2;
        o += 2 * (DIM == 3 ? wx * wy * wz : wx * wy);
    }
    return o;
}
// the full weighting's residual scratch (one array of the first level's layout after the levels): where the levels
// and it fit the LDS with 4 KB to spare for the static part (all fp32 shapes, fp64 16^3)
template <typename T, int DIM, int TX, int TY, int TZ>
constexpr bool tc_fw_scratch()
{
    const int p0 = DIM == 3 ? (TX + 2) * (TY + 2) * (TZ + 2) : (TX + 2) * (TY + 2);
    int n = 1, m = TX < TY ? TX : TY;
    if (DIM == 3 && TZ < m) m = TZ;
    for (int t = m; t > 1; t >>= 1) ++n;
    return (size_t)(tc_off<DIM, TX, TY, TZ>(n) + p0) * sizeof(T) + 4096 <= 160 * 1024;
}
// 16 waves in fp32; fp64 takes 8, so that the kernel keeps 256 VGPRs (at 16 waves it spilled 100-240 VGPRs)
#ifndef TC_THREADS_2D_F32  // (build knob: threads of the 2D fp32 tail)
#define TC_THREADS_2D_F32 1024
#endif
template <typename T, int DIM>
constexpr int tc_threads() { return sizeof(T) == 4 ? (DIM == 2 ? TC_THREADS_2D_F32 : 1024) : 512; }
#ifndef TC_MAXL  // timing experiment: skip the ops of levels >= TC_MAXL (wrong results)
#define TC_MAXL 16
#endif
// Levels of at most this many cells run on wave 0 alone, without workgroup barriers (build knob, 0: every level on the
// workgroup).  Measured slower (round 6, interleaved A/B): 3D 512 / 64 cells +6 / +3 us per 512^3 cycle, 2D 1024 cells
// +8 us, 256 cells neutral; a 16-wave barrier costs less than one wave walking a small level's cells alone.
#ifndef TC_WAVE_CELLS_3D
#define TC_WAVE_CELLS_3D 0
#endif
#ifndef TC_WAVE_CELLS_2D
#define TC_WAVE_CELLS_2D 0
#endif
template <int DIM, int NX, int NY, int NZ>
constexpr bool tc_wave_level()
{
    return TcLev<DIM, NX, NY, NZ>::CELLS <= (DIM == 3 ? TC_WAVE_CELLS_3D : TC_WAVE_CELLS_2D);
}
// The tail's phase boundary: a workgroup barrier, or on a level run by wave 0 alone its own ordering (the LDS accesses
// of one wave are performed in issue order; the wavefront-scope fences keep the compiler from moving them across)
template <bool WV>
__device__ __forceinline__ void tc_sync()
{
    if constexpr (WV) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

template <typename T, int DIM, int NX, int NY, int NZ, int NTH = tc_threads<T, DIM>()>
__device__ __forceinline__ void tc_half(T* U, const T* F, const Op<T, DIM>& op, int c, int tid)
{
    using L = TcLev<DIM, NX, NY, NZ>;
    if constexpr (NX >= 2) {
        constexpr int HN = NX / 2, CNT = L::CELLS / 2;
#pragma unroll
        for (int q0 = 0; q0 < CNT; q0 += NTH) {
            const int q = q0 + tid;
            if (q < CNT) {
                const int i2 = q % HN, j = (q / HN) % NY, k = DIM == 3 ? q / (HN * NY) : 0;
                const int i = 2 * i2 + ((j + k + c) & 1);
                const int x = L::idx(i, j, k);
                T sm = U[x - 1] + U[x + 1];
                sm = sm + U[x - L::W];
                sm = sm + U[x + L::W];
                if (DIM == 3) {
                    sm = sm + U[x - L::SZ];
                    sm = sm + U[x + L::SZ];
                }
                U[x] = op.relax_idx(sm, F[x], L::nb(i, j, k));
            }
        }
    } else {  // one cell per row: cell (0, j, k) has colour (j + k) & 1 (half_item's empty slot is skipped)
        constexpr int CNT = L::CELLS;
        for (int q = tid; q < CNT; q += NTH) {
            const int j = q % NY, k = DIM == 3 ? q / NY : 0;
            if (((j + k) & 1) != c) continue;
            const int x = L::idx(0, j, k);
            T sm = U[x - 1] + U[x + 1];
            sm = sm + U[x - L::W];
            sm = sm + U[x + L::W];
            if (DIM == 3) {
                sm = sm + U[x - L::SZ];
                sm = sm + U[x + L::SZ];
            }
            const T rv = op.relax_idx(sm, F[x], L::nb(0, j, k));
            if constexpr (CNT == 1)  // the one-cell level: under cl = -1 its diagonal is 0 and the cell is relaxed to +0
                U[x] = op.dg[2 * DIM] == (T)0 ? (T)0 : rv;
            else
                U[x] = rv;
        }
    }
}

template <typename T, int DIM, int NX, int NY, int NZ>
__device__ __forceinline__ T tc_res(const T* U, const T* F, const Op<T, DIM>& op, int i, int j, int k)
{
    using L = TcLev<DIM, NX, NY, NZ>;
    const int x = L::idx(i, j, k);
    T sm = U[x - 1] + U[x + 1];
    sm = sm + U[x - L::W];
    sm = sm + U[x + L::W];
    if (DIM == 3) {
        sm = sm + U[x - L::SZ];
        sm = sm + U[x + L::SZ];
    }
    return op.residual_idx(sm, F[x], U[x], L::nb(i, j, k));
}

template <typename T, int DIM, int NX, int NY, int NZ, int NTH = tc_threads<T, DIM>()>
__device__ __forceinline__ void tc_rr(const T* U, const T* F, T* Fc, const Op<T, DIM>& op, int tid)
{
    constexpr int MX = NX / 2, MY = NY / 2, MZ = DIM == 3 ? NZ / 2 : 1;
    using C = TcLev<DIM, MX, MY, MZ>;
    constexpr int CNT = C::CELLS;
    auto res = [&](int i, int j, int k) { return tc_res<T, DIM, NX, NY, NZ>(U, F, op, i, j, k); };
    for (int q = tid; q < CNT; q += NTH) {
        const int I = q % MX, J = (q / MX) % MY, K = DIM == 3 ? q / (MX * MY) : 0;
        const int i = 2 * I, j = 2 * J, k = 2 * K;
        T sm = res(i, j, k) + res(i + 1, j, k);
        sm = sm + res(i, j + 1, k);
        sm = sm + res(i + 1, j + 1, k);
        if (DIM == 3) {
            sm = sm + res(i, j, k + 1);
            sm = sm + res(i + 1, j, k + 1);
            sm = sm + res(i, j + 1, k + 1);
            sm = sm + res(i + 1, j + 1, k + 1);
        }
        Fc[C::idx(I, J, K)] = (DIM == 3 ? (T)0.125 : (T)0.25) * sm;
    }
}

// tc_rr with the full-weighting restriction (fw_eval over the residuals of the 4^DIM fine cells)
template <typename T, int DIM, int NX, int NY, int NZ, int NTH = tc_threads<T, DIM>()>
__device__ __forceinline__ void tc_rr_fw(const T* U, const T* F, T* Fc, const Op<T, DIM>& op, T wf, int tid)
{
    constexpr int MX = NX / 2, MY = NY / 2, MZ = DIM == 3 ? NZ / 2 : 1;
    using C = TcLev<DIM, MX, MY, MZ>;
    constexpr int CNT = C::CELLS;
    Geo g{}, gc{};
    g.nx = NX;
    g.ny = NY;
    g.gnz = DIM == 3 ? NZ : 1;
    gc.nx = MX;
    gc.ny = MY;
    gc.gnz = MZ;
    auto res = [&](int i, int j, int64_t k64) { return tc_res<T, DIM, NX, NY, NZ>(U, F, op, i, j, (int)k64); };
    for (int q = tid; q < CNT; q += NTH) {
        const int I = q % MX, J = (q / MX) % MY, K = DIM == 3 ? q / (MX * MY) : 0;
        Fc[C::idx(I, J, K)] = fw_eval<T, DIM>(res, g, gc, wf, I, J, (int64_t)K);
    }
}

// tc_rr_fw through a residual scratch: r of every cell of the level into RS (the level's unpacked layout) once, then
// the full weighting of each coarse cell from RS (tc_rr_fw evaluates each fine residual for all 8 coarse cells that
// weight it: 64 residuals per coarse cell, the FW tail's extra 27 us per 512^3 cycle)
template <typename T, int DIM, int NX, int NY, int NZ, int NTH = tc_threads<T, DIM>()>
__device__ __forceinline__ void tc_rr_fw_s(const T* U, const T* F, T* Fc, const Op<T, DIM>& op, T wf, int tid, T* RS)
{
    using L = TcLev<DIM, NX, NY, NZ>;
    constexpr int MX = NX / 2, MY = NY / 2, MZ = DIM == 3 ? NZ / 2 : 1;
    using C = TcLev<DIM, MX, MY, MZ>;
    for (int q = tid; q < L::CELLS; q += NTH) {
        const int i = q % NX, j = (q / NX) % NY, k = DIM == 3 ? q / (NX * NY) : 0;
        RS[L::idx(i, j, k)] = tc_res<T, DIM, NX, NY, NZ>(U, F, op, i, j, k);
    }
    tc_sync<(NTH < tc_threads<T, DIM>())>();
    Geo g{}, gc{};
    g.nx = NX;
    g.ny = NY;
    g.gnz = DIM == 3 ? NZ : 1;
    gc.nx = MX;
    gc.ny = MY;
    gc.gnz = MZ;
    auto get = [&](int i, int j, int64_t k) { return RS[L::idx(i, j, (int)k)]; };
    for (int q = tid; q < C::CELLS; q += NTH) {
        const int I = q % MX, J = (q / MX) % MY, K = DIM == 3 ? q / (MX * MY) : 0;
        Fc[C::idx(I, J, K)] = fw_eval<T, DIM>(get, g, gc, wf, I, J, (int64_t)K);
    }
}

template <typename T, int DIM, int NX, int NY, int NZ, int LINEAR, int NTH = tc_threads<T, DIM>()>
__device__ __forceinline__ void tc_prolong(T* U, const T* V, T cl, int tid)
{
    using L = TcLev<DIM, NX, NY, NZ>;
    constexpr int MX = NX / 2, MY = NY / 2, MZ = DIM == 3 ? NZ / 2 : 1;
    using C = TcLev<DIM, MX, MY, MZ>;
    constexpr int CNT = L::CELLS;
#pragma unroll 1
    for (int q0 = 0; q0 < CNT; q0 += NTH) {
        const int q = q0 + tid;
        if (q < CNT) {
            const int i = q % NX, j = (q / NX) % NY, k = DIM == 3 ? q / (NX * NY) : 0;
            const int I = i >> 1, J = j >> 1, K = k >> 1;
            T v;
            if (!LINEAR) {
                v = V[C::idx(I, J, K)];
            } else {
                const T w0 = (T)0.75, w1 = (T)0.25;
                int In = (i & 1) ? I + 1 : I - 1, Jn = (j & 1) ? J + 1 : J - 1, Kn = (k & 1) ? K + 1 : K - 1;
                const bool ox = In < 0 || In >= MX, oy = Jn < 0 || Jn >= MY, oz = DIM == 3 && (Kn < 0 || Kn >= MZ);
                if (ox) In = I;
                if (oy) Jn = J;
                if (oz || DIM == 2) Kn = K;
                auto cv = [&](int a, int b, int d, bool fx, bool fy, bool fz) {  // cval()
                    T s = (T)1;
                    if (fx) s = -cl * s;
                    if (fy) s = -cl * s;
                    if (fz) s = -cl * s;
                    const T val = V[C::idx(a, b, d)];
                    return s == (T)1 ? val : s * val;
                };
                if (DIM == 2) {
                    const T a0 = w0 * cv(I, J, 0, false, false, false) + w1 * cv(In, J, 0, ox, false, false);
                    const T a1 = w0 * cv(I, Jn, 0, false, oy, false) + w1 * cv(In, Jn, 0, ox, oy, false);
                    v = w0 * a0 + w1 * a1;
                } else {
                    const T a00 = w0 * cv(I, J, K, false, false, false) + w1 * cv(In, J, K, ox, false, false);
                    const T a10 = w0 * cv(I, Jn, K, false, oy, false) + w1 * cv(In, Jn, K, ox, oy, false);
                    const T a01 = w0 * cv(I, J, Kn, false, false, oz) + w1 * cv(In, J, Kn, ox, false, oz);
                    const T a11 = w0 * cv(I, Jn, Kn, false, oy, oz) + w1 * cv(In, Jn, Kn, ox, oy, oz);
                    const T b0 = w0 * a00 + w1 * a10;
                    const T b1 = w0 * a01 + w1 * a11;
                    v = w0 * b0 + w1 * b1;
                }
            }
            const int x = L::idx(i, j, k);
            U[x] = U[x] + v;
        }
    }
}

// the packed global offset of LDS element q of a level (its (i, j, k), -1 in the halo)
template <int DIM, int NX, int NY, int NZ>
__device__ __forceinline__ int64_t tc_global(int q)
{
    using L = TcLev<DIM, NX, NY, NZ>;
    constexpr int HW = NX >= 2 ? NX / 2 : 1;
    constexpr int64_t H = (int64_t)HW * NY, P = 2 * H;
    const int i = q % L::W - 1, j = (q / L::W) % L::WY - 1, k = DIM == 3 ? q / (L::W * L::WY) - 1 : 0;
    const bool inside = q < L::P && i >= 0 && i < NX && j >= 0 && j < NY && k >= 0 && k < (DIM == 3 ? NZ : 1);
    return inside ? (int64_t)k * P + ((i + j + k) & 1) * H + (int64_t)j * HW + (i >> 1) : -1;
}

// level l of the tail: copy in (zero halo; a field the program writes before it reads it is not loaded: ld_u / ld_f
// false, zero) or out (f only where the program wrote it: st_f), packed global layout; a thread's loads are all issued
// before its LDS stores (compile-time trip count)
template <typename T, int DIM, int NX, int NY, int NZ>
__device__ __forceinline__ void tc_copy(T* U, T* F, T* gu, T* gf, bool in, bool ld_u, bool ld_f, bool st_f, int tid)
{
    using L = TcLev<DIM, NX, NY, NZ>;
    constexpr int IT = (L::P + tc_threads<T, DIM>() - 1) / tc_threads<T, DIM>();
    T uv[IT], fv[IT];
#pragma unroll
    for (int r = 0; r < IT; ++r) {
        const int q = tid + r * tc_threads<T, DIM>();
        const int64_t gi = tc_global<DIM, NX, NY, NZ>(q);
        if (in) {
            uv[r] = gi >= 0 && ld_u ? gu[gi] : (T)0;
            fv[r] = gi >= 0 && ld_f ? gf[gi] : (T)0;
        } else if (gi >= 0) {
            gu[gi] = U[q];
            if (st_f) gf[gi] = F[q];
        }
    }
    if (in) {
#pragma unroll
        for (int r = 0; r < IT; ++r) {
            const int q = tid + r * tc_threads<T, DIM>();
            if (q < L::P) {
                U[q] = uv[r];
                F[q] = fv[r];
            }
        }
    }
}

// Copy-in in two halves, so that every level's global loads are in flight together (round 4: tc_copy level by
// level waited for one level's loads before issuing the next level's: seven load latencies in a row in 2D)
template <typename T, int DIM, int NX, int NY, int NZ>
struct TcRegs {
    static constexpr int IT = (TcLev<DIM, NX, NY, NZ>::P + tc_threads<T, DIM>() - 1) / tc_threads<T, DIM>();
    T u[IT], f[IT];
};
template <typename T, int DIM, int NX, int NY, int NZ>
__device__ __forceinline__ void tc_load(TcRegs<T, DIM, NX, NY, NZ>& rg, const T* gu, const T* gf, bool ld_u, bool ld_f,
                                        int tid)
{
#pragma unroll
    for (int r = 0; r < TcRegs<T, DIM, NX, NY, NZ>::IT; ++r) {
        const int64_t gi = tc_global<DIM, NX, NY, NZ>(tid + r * tc_threads<T, DIM>());
        rg.u[r] = gi >= 0 && ld_u ? gu[gi] : (T)0;
        rg.f[r] = gi >= 0 && ld_f ? gf[gi] : (T)0;
    }
}
template <typename T, int DIM, int NX, int NY, int NZ>
__device__ __forceinline__ void tc_store(T* U, T* F, const TcRegs<T, DIM, NX, NY, NZ>& rg, int tid)
{
    using L = TcLev<DIM, NX, NY, NZ>;
#pragma unroll
    for (int r = 0; r < TcRegs<T, DIM, NX, NY, NZ>::IT; ++r) {
        const int q = tid + r * tc_threads<T, DIM>();
        if (q < L::P) {
            U[q] = rg.u[r];
            F[q] = rg.f[r];
        }
    }
}

template <typename T, int DIM, int LINEAR, int TX, int TY, int TZ>
__global__ __launch_bounds__((tc_threads<T, DIM>())) void k_tail_c(const TailArgs<T, DIM> a)
{
    constexpr int NL = tc_levels<DIM, TX, TY, TZ>();
    // the full weighting's residual scratch after the levels, where it fits (tc_lds_total)
    constexpr bool FWR = tc_fw_scratch<T, DIM, TX, TY, TZ>();
    constexpr int FWR_OFF = tc_off<DIM, TX, TY, TZ>(NL);
    extern __shared__ __align__(16) unsigned char tc_smem[];
    T* const lds = reinterpret_cast<T*>(tc_smem);
    // the level operators in LDS, read per op (held in registers for all levels they spill)
    __shared__ Op<T, DIM> sop[NL];
    if ((int)threadIdx.x < NL) sop[threadIdx.x] = a.op[threadIdx.x];
#define TC_NX(l) tc_dim_at<TX, (l)>()
#define TC_NY(l) tc_dim_at<TY, (l)>()
#define TC_NZ(l) (DIM == 3 ? tc_dim_at<TZ, (l)>() : 1)
#define TC_SH(l) TC_NX(l), TC_NY(l), TC_NZ(l)
#define TC_U(l) (lds + tc_off<DIM, TX, TY, TZ>(l))
#define TC_F(l) (lds + tc_off<DIM, TX, TY, TZ>(l) + TcLev<DIM, TC_SH(l)>::P)
#define TC_COPY(l, IN)                                                                                      \
    if constexpr ((l) < NL) tc_copy<T, DIM, TC_SH(l)>(TC_U(l), TC_F(l), a.u[l], a.f[l], IN, (a.in_u >> (l)) & 1,     \
                                                      (a.in_f >> (l)) & 1, (a.out_f >> (l)) & 1, threadIdx.x);
#define TC_LOAD(l)                                                                                          \
    TcRegs<T, DIM, TC_SH(l)> rg##l;                                                                         \
    if constexpr ((l) < NL) tc_load<T, DIM, TC_SH(l)>(rg##l, a.u[l], a.f[l], (a.in_u >> (l)) & 1, (a.in_f >> (l)) & 1, \
                                                      threadIdx.x);
#define TC_STORE(l) \
    if constexpr ((l) < NL) tc_store<T, DIM, TC_SH(l)>(TC_U(l), TC_F(l), rg##l, threadIdx.x);
    if constexpr (DIM == 2) {  // (3D: the held values push the kernel past 64 VGPRs into spills; level by level)
        TC_LOAD(0) TC_LOAD(1) TC_LOAD(2) TC_LOAD(3) TC_LOAD(4) TC_LOAD(5) TC_LOAD(6)
        TC_STORE(0) TC_STORE(1) TC_STORE(2) TC_STORE(3) TC_STORE(4) TC_STORE(5) TC_STORE(6)
    } else {
        TC_COPY(0, true) TC_COPY(1, true) TC_COPY(2, true) TC_COPY(3, true) TC_COPY(4, true) TC_COPY(5, true)
        TC_COPY(6, true)
    }
#undef TC_STORE
#undef TC_LOAD
    __syncthreads();
#ifdef TC_PROF  // timing experiment: wall-clock ticks (100 MHz) per op into f of the first level (tools/tail_prof.py)
    __shared__ long long tcp[130];
    if (threadIdx.x == 0) tcp[0] = wall_clock64();
#endif
    bool wave_prev = false;  // the last op ran on wave 0 alone (the same on every wave)
    for (int pc = 0; pc < a.nops; ++pc) {
        const uint32_t w = a.ops[pc];
        const int op = (int)(w & 15), l = (int)((w >> 4) & 15), arg = (int)(w >> 8);
        // an opaque copy of the thread index per op: the index arithmetic of every (level, op) would
        // otherwise be hoisted out of this loop and held in registers for the whole program
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#define TC_CASE(L)                                                                                     \
    case L:                                                                                            \
        if constexpr ((L) < NL && (L) < TC_MAXL) {                                                     \
            using LV = TcLev<DIM, TC_SH(L)>;                                                           \
            /* a small level runs on wave 0 alone (the other waves skip to the next workgroup-wide op) */ \
            constexpr bool WV = tc_wave_level<DIM, TC_SH(L)>() && tc_threads<T, DIM>() > 64;          \
            constexpr int NTH = WV ? 64 : tc_threads<T, DIM>();                                        \
            if constexpr (WV) {                                                                        \
                wave_prev = true;                                                                      \
                if (tid >= 64) break;                                                                  \
            } else {                                                                                   \
                if (wave_prev) __syncthreads();                                                        \
                wave_prev = false;                                                                     \
            }                                                                                          \
            if (op == TAIL_SMOOTH) {                                                                   \
                for (int sw = 0; sw < arg; ++sw) {                                                     \
                    tc_half<T, DIM, TC_SH(L), NTH>(TC_U(L), TC_F(L), sop[L], 0, tid);                  \
                    tc_sync<WV>();                                                                     \
                    if (LV::CELLS >= 2) {                                                              \
                        tc_half<T, DIM, TC_SH(L), NTH>(TC_U(L), TC_F(L), sop[L], 1, tid);              \
                        tc_sync<WV>();                                                                 \
                    }                                                                                  \
                }                                                                                      \
            } else if (op == TAIL_ZERO) {                                                              \
                T* u = TC_U(L);                                                                        \
                constexpr int NXL = TC_NX(L), NYL = TC_NY(L);                                          \
                for (int q = tid; q < LV::CELLS; q += NTH)                                             \
                    u[LV::idx(q % NXL, (q / NXL) % NYL, DIM == 3 ? q / (NXL * NYL) : 0)] = (T)0;       \
                tc_sync<WV>();                                                                         \
            } else if constexpr ((L) + 1 < NL) {                                                       \
                if (op == TAIL_RR) {                                                                   \
                    if (a.fw) {                                                                        \
                        if constexpr (FWR)                                                             \
                            tc_rr_fw_s<T, DIM, TC_SH(L), NTH>(TC_U(L), TC_F(L), TC_F((L) + 1), sop[L],     \
                                                              (T)3 - sop[(L) + 1].cl, tid, lds + FWR_OFF); \
                        else                                                                           \
                            tc_rr_fw<T, DIM, TC_SH(L), NTH>(TC_U(L), TC_F(L), TC_F((L) + 1), sop[L],       \
                                                            (T)3 - sop[(L) + 1].cl, tid);                 \
                    } else                                                                             \
                        tc_rr<T, DIM, TC_SH(L), NTH>(TC_U(L), TC_F(L), TC_F((L) + 1), sop[L], tid);    \
                    /* a fresh guess of the next level (its ZERO op follows) in the same phase: RR writes */ \
                    /* that level's f, ZERO its u                                                        */ \
                    const uint32_t wn = pc + 1 < a.nops ? a.ops[pc + 1] : 0u;                          \
                    if ((int)(wn & 15) == TAIL_ZERO && (int)((wn >> 4) & 15) == (L) + 1) {              \
                        using CV = TcLev<DIM, TC_SH((L) + 1)>;                                         \
                        constexpr int MX = TC_NX((L) + 1), MY = TC_NY((L) + 1);                        \
                        T* uc = TC_U((L) + 1);                                                         \
                        for (int q = tid; q < CV::CELLS; q += NTH)                                     \
                            uc[CV::idx(q % MX, (q / MX) % MY, DIM == 3 ? q / (MX * MY) : 0)] = (T)0;   \
                        ++pc;                                                                          \
                    }                                                                                  \
                    tc_sync<WV>();                                                                     \
                } else if (op == TAIL_PROLONG) {                                                       \
                    tc_prolong<T, DIM, TC_SH(L), LINEAR, NTH>(TC_U(L), TC_U((L) + 1), sop[(L) + 1].cl, tid); \
                    tc_sync<WV>();                                                                     \
                }                                                                                      \
            }                                                                                          \
        }                                                                                              \
        break;
        switch (l) {
            TC_CASE(0)
            TC_CASE(1)
            TC_CASE(2)
            TC_CASE(3)
            TC_CASE(4)
            TC_CASE(5)
            TC_CASE(6)
            default: break;
        }
#undef TC_CASE
#ifdef TC_PROF
        __syncthreads();
        if (threadIdx.x == 0 && pc < 128) tcp[pc + 1] = wall_clock64();
#endif
    }
#ifdef TC_PROF
    if (threadIdx.x == 0) {
        // op q's ticks at cell (q % TX, q / TX, 0) of the first level's f, then 0; op code (op | level << 4) + 1
        // at the cell after the ticks' row block (rows 2 and 3)
        using L0 = TcLev<DIM, TC_SH(0)>;
        T* F0 = TC_F(0);
        const int n = a.nops < 2 * TX ? a.nops : 2 * TX;
        for (int q = 0; q < n; ++q) {
            F0[L0::idx(q % TX, q / TX, 0)] = (T)(tcp[q + 1] - tcp[q]);
            F0[L0::idx(q % TX, 2 + q / TX, 0)] = (T)((a.ops[q] & 255) + 1);
        }
        if (n < 2 * TX) {
            F0[L0::idx(n % TX, n / TX, 0)] = (T)0;
            F0[L0::idx(n % TX, 2 + n / TX, 0)] = (T)0;
        }
    }
    __syncthreads();
#endif
    if (wave_prev) __syncthreads();
    TC_COPY(0, false) TC_COPY(1, false) TC_COPY(2, false) TC_COPY(3, false) TC_COPY(4, false) TC_COPY(5, false)
    TC_COPY(6, false)
#undef TC_COPY
#undef TC_F
#undef TC_U
#undef TC_SH
#undef TC_NZ
#undef TC_NY
#undef TC_NX
}

template <int DIM, int TX, int TY, int TZ>
constexpr size_t tc_lds(int rb)
{
    return (size_t)tc_off<DIM, TX, TY, TZ>(tc_levels<DIM, TX, TY, TZ>()) * rb;
}
// the dynamic LDS of a launch: the levels, and the full weighting's scratch where it fits
template <typename T, int DIM, int TX, int TY, int TZ>
constexpr size_t tc_lds_total()
{
    return tc_lds<DIM, TX, TY, TZ>(sizeof(T)) +
           (tc_fw_scratch<T, DIM, TX, TY, TZ>() ? (size_t)TcLev<DIM, TX, TY, DIM == 3 ? TZ : 1>::P * sizeof(T) : 0);
}

// The compile-time tail shapes (first level nx x ny x nz; nz = 1 in 2D) and their kernels.  k_tail_c runs a
// tail whose first level is one of these (tail_shape); any other red/black tail runs the generic k_tail.
#define MGP_TC_SHAPES(X)   \
    X(3, 16, 16, 16)       \
    X(3, 32, 32, 4)        \
    X(3, 8, 8, 16)         \
    X(3, 8, 8, 32)         \
    X(3, 8, 8, 64)         \
    X(2, 64, 64, 1)

}  // namespace

#ifdef TAIL_PROF
constexpr int kTailStaticLds = 1024;
#else
constexpr int kTailStaticLds = 0;
#endif

template <typename T, int D>
static hipError_t tail_attr()
{
    hipError_t e = hipFuncSetAttribute((const void*)k_tail<T, D, 0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kTailMaxLds - kTailStaticLds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)k_tail<T, D, 1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kTailMaxLds - kTailStaticLds);
    return e;
}

size_t tail_lds_bytes(int rb, int dim, int jacobi, const Geo* g, int nlev)
{
    const int G = dim == 3 ? kGhost3D : 0;
    size_t n = 0;
    for (int l = 0; l < nlev; ++l) n += (size_t)((g[l].nz + 2 * G) * g[l].P) * (jacobi ? 3 : 2);
    return n * (size_t)rb;
}

// k_tail_c applies: red/black, the first level one of MGP_TC_SHAPES and the levels below it the tail's levels
// (one rank's replicated box); returns the shape's index, or -1 (MGP_TAIL_CUBIC=0: always the generic k_tail)
static int tail_shape(const TailSpec& t, int dim)
{
    const char* v = std::getenv("MGP_TAIL_CUBIC");
    if ((v && std::atoi(v) == 0) || t.jacobi) return -1;
    int idx = -1, found = -1;
    auto match = [&](int D, int TX, int TY, int TZ, int NL) {
        ++idx;
        if (found >= 0 || D != dim || t.nlev != NL) return;
        for (int l = 0; l < t.nlev; ++l) {
            const Geo& g = t.g[l];
            const int nx = TX >> l > 0 ? TX >> l : 1, ny = TY >> l > 0 ? TY >> l : 1, nz = TZ >> l > 0 ? TZ >> l : 1;
            if (g.nx != nx || g.ny != ny || g.z0 != 0 || (dim == 3 && (g.nz != nz || g.gnz != nz))) return;
        }
        found = idx;
    };
#define X(D, TX, TY, TZ) match(D, TX, TY, TZ, tc_levels<D, TX, TY, TZ>());
    MGP_TC_SHAPES(X)
#undef X
    return found;
}

// Which fields a tail program reads before writing them (in_u / in_f, bit l = level l: only those are loaded into
// LDS) and which f it writes (out_f: only those are stored back; u is always stored).  A V- or F-cycle tail reads
// level 0's f (and its u unless it is a fresh guess); every level below gets its f from the restriction and, with
// fresh coarse guesses, its u from the zeroing before anything reads them.
static void tail_io_masks(const TailSpec& t, uint32_t& in_u, uint32_t& in_f, uint32_t& out_f)
{
    uint32_t wu = t.zero_first ? 1u : 0u, wf = 0;
    in_u = in_f = 0;
    auto rd = [&](int l) {
        if (!((wu >> l) & 1)) in_u |= 1u << l;
        if (!((wf >> l) & 1)) in_f |= 1u << l;
    };
    for (int i = 0; i < t.nops; ++i) {
        const uint32_t w = t.ops[i];
        const int op = (int)(w & 15), l = (int)((w >> 4) & 15);
        if (op == TAIL_SMOOTH) {
            rd(l);
        } else if (op == TAIL_RR) {
            rd(l);
            wf |= 1u << (l + 1);
        } else if (op == TAIL_ZERO) {
            wu |= 1u << l;
        } else if (op == TAIL_PROLONG) {
            if (!((wu >> (l + 1)) & 1)) in_u |= 1u << (l + 1);
            if (!((wu >> l) & 1)) in_u |= 1u << l;
        }
    }
    out_f = wf;
}

template <typename T, int D>
static hipError_t tail_t(const TailSpec& t, hipStream_t s)
{
    TailArgs<T, D> a{};
    a.nlev = t.nlev;
    a.nops = t.nops;
    a.jacobi = t.jacobi;
    a.zero0 = t.zero_first;
    a.fw = t.fw;
    tail_io_masks(t, a.in_u, a.in_f, a.out_f);
    const int G = D == 3 ? kGhost3D : 0;
    int64_t off = 0;
    for (int l = 0; l < t.nlev; ++l) {
        a.g[l] = t.g[l];
        a.u[l] = (T*)t.u[l];
        a.f[l] = (T*)t.f[l];
        a.op[l] = make_op<T, D>(t.h[l], t.cl[l]);
        a.region[l] = (t.g[l].nz + 2 * G) * t.g[l].P;
        a.off[l] = off;
        off += a.region[l] * (t.jacobi ? 3 : 2);
    }
    for (int i = 0; i < t.nops; ++i) a.ops[i] = t.ops[i];
    const int sh = tail_shape(t, D);
    if (sh >= 0) {
        int idx = -1;
        bool done = false;
#define X(DD, TX, TY, TZ)                                                                                    \
        if constexpr (DD == D) {                                                                             \
            if (++idx == sh && !done) {                                                                      \
                auto kc = t.linear ? k_tail_c<T, D, 1, TX, TY, TZ> : k_tail_c<T, D, 0, TX, TY, TZ>;          \
                kc<<<1, tc_threads<T, D>(), tc_lds_total<T, D, TX, TY, TZ>(), s>>>(a);                               \
                done = true;                                                                                 \
            }                                                                                                \
        } else {                                                                                             \
            ++idx;                                                                                           \
        }
        MGP_TC_SHAPES(X)
#undef X
        return done ? hipGetLastError() : hipErrorInvalidValue;
    }
    const size_t bytes = (size_t)off * sizeof(T);
    auto kern = t.linear ? k_tail<T, D, 1> : k_tail<T, D, 0>;
    kern<<<1, tail_threads<T>(), bytes, s>>>(a);
    return hipGetLastError();
}

template <typename T>
static hipError_t tail_c_attr()
{
    const auto A = hipFuncAttributeMaxDynamicSharedMemorySize;
    hipError_t e = hipSuccess;
#define X(D, TX, TY, TZ)                                                                                 \
    if (e == hipSuccess)                                                                                 \
        e = hipFuncSetAttribute((const void*)k_tail_c<T, D, 0, TX, TY, TZ>, A, (int)tc_lds_total<T, D, TX, TY, TZ>()); \
    if (e == hipSuccess)                                                                                 \
        e = hipFuncSetAttribute((const void*)k_tail_c<T, D, 1, TX, TY, TZ>, A, (int)tc_lds_total<T, D, TX, TY, TZ>());
    MGP_TC_SHAPES(X)
#undef X
    return e;
}

hipError_t launch_tail(int rb, int dim, const TailSpec& t, hipStream_t s)
{
    if (t.nlev < 1 || t.nlev > kTailMaxLevels || t.nops > kTailMaxOps) return hipErrorInvalidValue;
    if (rb == 8) return dim == 3 ? tail_t<double, 3>(t, s) : tail_t<double, 2>(t, s);
    return dim == 3 ? tail_t<float, 3>(t, s) : tail_t<float, 2>(t, s);
}

hipError_t tail_attr(int rb)
{
    hipError_t e = rb == 4 ? tail_attr<float, 2>() : tail_attr<double, 2>();
    if (e == hipSuccess) e = rb == 4 ? tail_attr<float, 3>() : tail_attr<double, 3>();
    if (e == hipSuccess) e = rb == 4 ? tail_c_attr<float>() : tail_c_attr<double>();
    return e;
}

}  // namespace mgp
