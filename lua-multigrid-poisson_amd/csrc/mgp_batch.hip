// mgp_batch.hip — B independent small boxes in one hierarchy (mgp_batch_*, include/mgpoisson.h): every kernel of a
// cycle covers all members in one launch, and each member stops on its own.
//
// No reference counterpart (the reference solves one box): per member the cycle is cpu.lua:70-165 and the outer
// loop cpu.lua:196-216, with the arithmetic of the ordinary context (Op::relax / residual, prolong_eval, the
// reference-order 2^d average, the packed red/black layout of mgp_device.h), so a member's psi equals the ordinary
// context's and the oracle's bit for bit.
//
// Layout: a level holds its members back to back, member m at m * slots reals, each in the packed red/black
// layout of Geo (no ghost planes: a neighbour outside a member's box reads as +0, so no kernel ever reads across
// a member boundary).  The member of a workgroup is blockIdx.x / (workgroups per member): wave-uniform.
//
// Engines: the levels from `T` down (the first level of <= 4096 cells whose sub-hierarchy fits one workgroup's
// LDS) run as ONE launch with one workgroup per member, executing the op program of the coarse sub-cycle (the one
// the ordinary context's tail executes) from LDS; the levels above run one launch per piece (half-sweep, residual
// + restriction, prolongation + correction).  Both engines execute the same per-piece device functions.
//
// mgp_batch_fmg (the full multigrid start per member, mgp_fmg's definition): the levels from T down are one launch of the
// LDS engine as well (k_batch_tail<.., FMG = true>: its op program restricts f, solves the coarsest level and runs every
// cubic prolongation and per-level cycle up to level T), the levels above one launch per piece (k_batch_restrict_field;
// the marching vector P3 of mgp_fmg.hip over all members, or k_batch_fmg_prolong), all captured as one graph.
#include "mgp_fmg_dev.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/mgpoisson.h"

namespace mgp {
namespace {

constexpr int kErrBlocks = 64;        // err / norm partials per member at most
constexpr int64_t kTailCells = 4096;  // the LDS engine starts at the first level of at most this many cells

// One level of one member, as the device sees it
template <typename T, int DIM>
struct BLev {
    Geo g;
    Op<T, DIM> op;
    int64_t slots;  // reals per member = nz * P
};

// A member's packed layout in 32-bit integers: Geo of mgp_device.h with z0 = 0 and P = 2 H (a member has at most
// 2^25 slots), pslot == pidx and slot_of == slot_cell
struct MGeo {
    int nx, ny, nz, hw, lhw, ly, lh, H, P;
};
__device__ __forceinline__ MGeo mgeo(const Geo& g)
{
    MGeo m;
    m.nx = g.nx;
    m.ny = g.ny;
    m.nz = (int)g.nz;
    m.hw = g.hw;
    m.lhw = g.lhw;
    m.ly = g.ly;
    m.lh = g.lhw + g.ly;
    m.H = (int)g.H;
    m.P = 2 * m.H;
    return m;
}
__device__ __forceinline__ int pslot(const MGeo& g, int i, int j, int k)
{
    return k * g.P + ((i + j + k) & 1) * g.H + j * g.hw + (i >> 1);
}
// slot -> cell; false for a slot that holds no cell (nx = 1: i = 1)
__device__ __forceinline__ bool slot_of(int s, const MGeo& g, int& i, int& j, int& k)
{
    const int r = s & (g.P - 1);
    k = s >> (g.lh + 1);
    j = (r >> g.lhw) & (g.ny - 1);
    const int c = (r >> g.lh) & 1;
    i = 2 * (r & (g.hw - 1)) + (c ^ ((j + k) & 1));
    return i < g.nx;
}

// ((xl + xr) + yl) + yr [+ zl + zr] (cpu.lua:44-48) around the cell (i, j, k) at slot p, a neighbour outside the
// member's box reading as +0 (the oracle's zero padding), and the number of box faces of the cell.  Every
// neighbour has the other colour: it sits in the other half of its plane (slot p ^ H is the same row position
// there), x -+ 1 at m - 1 + (i & 1) and m + (i & 1), y -+ 1 a row and z -+ 1 a plane away.
template <typename T, int DIM>
__device__ __forceinline__ T nbsum(const T* u, const MGeo& g, int p, int i, int j, int k, int& nb)
{
    const int ob = p ^ g.H, o = i & 1;
    const T xl = i > 0 ? u[ob - 1 + o] : (T)0;
    const T xr = i < g.nx - 1 ? u[ob + o] : (T)0;
    const T yl = j > 0 ? u[ob - g.hw] : (T)0;
    const T yr = j < g.ny - 1 ? u[ob + g.hw] : (T)0;
    T s = xl + xr;
    s = s + yl;
    s = s + yr;
    nb = (i == 0) + (i == g.nx - 1) + (j == 0) + (j == g.ny - 1);
    if (DIM == 3) {
        const T zl = k > 0 ? u[ob - g.P] : (T)0;
        const T zr = k < g.nz - 1 ? u[ob + g.P] : (T)0;
        s = s + zl;
        s = s + zr;
        nb += (k == 0) + (k == g.nz - 1);
    }
    return s;
}

// The pieces of a cycle on one member: work items tid, tid + nt, ... (a grid's threads of one member, or one
// workgroup's).  Pointers are the member's own fields, in global memory or LDS.

// dst's cells of colour c (0 red, 1 black; -1: every cell, Jacobi with src != dst) = relax(src, f)
template <typename T, int DIM>
__device__ __forceinline__ void sweep_part(const T* src, const T* f, T* dst, const BLev<T, DIM>& L, int c, int tid, int nt)
{
    const MGeo g = mgeo(L.g);
    const int n = c < 0 ? g.nz * g.P : g.nz * g.H;
    for (int q = tid; q < n; q += nt) {
        int s = q;
        if (c >= 0) {
            const int kp = q >> g.lh;
            s = kp * g.P + c * g.H + (q - (kp << g.lh));
        }
        int i, j, k;
        if (!slot_of(s, g, i, j, k)) continue;
        int nb;
        const T sum = nbsum<T, DIM>(src, g, s, i, j, k, nb);
        dst[s] = L.op.relax_z(sum, f[s], nb);
    }
}

// R = the 2^d average (cpu.lua:127-135, x fastest) of r = f - A u (cpu.lua:108-123)
template <typename T, int DIM>
__device__ __forceinline__ void rr_part(const T* u, const T* f, T* R, const BLev<T, DIM>& L, const Geo& gcoarse, int tid,
                                        int nt)
{
    const MGeo g = mgeo(L.g), gc = mgeo(gcoarse);
    const int n = gc.nz * gc.P;
    for (int q = tid; q < n; q += nt) {
        int I, J, K;
        if (!slot_of(q, gc, I, J, K)) continue;
        T s = (T)0;
#pragma unroll
        for (int d = 0; d < (1 << DIM); ++d) {
            const int i = 2 * I + (d & 1), j = 2 * J + ((d >> 1) & 1), k = DIM == 3 ? 2 * K + (d >> 2) : 0;
            const int p = pslot(g, i, j, k);
            int nb;
            const T sum = nbsum<T, DIM>(u, g, p, i, j, k, nb);
            const T r = L.op.residual(sum, f[p], u[p], nb);
            s = d == 0 ? r : s + r;
        }
        R[q] = (DIM == 2 ? (T)0.25 : (T)0.125) * s;
    }
}

// u += P V (cpu.lua:142-158); clc: the coarse level's boundary coefficient
template <typename T, int DIM>
__device__ __forceinline__ void prolong_part(T* u, const T* V, const BLev<T, DIM>& L, const Geo& gcoarse, T clc, int linear,
                                             int tid, int nt)
{
    const MGeo g = mgeo(L.g), gc = mgeo(gcoarse);
    const auto get = [&](int I, int J, int64_t K) { return V[pslot(gc, I, J, (int)K)]; };
    const int n = g.nz * g.P;
    for (int s = tid; s < n; s += nt) {
        int i, j, k;
        if (!slot_of(s, g, i, j, k)) continue;
        const T v = linear ? prolong_eval<T, DIM, 1>(get, gcoarse, clc, i, j, k)
                           : prolong_eval<T, DIM, 0>(get, gcoarse, clc, i, j, k);
        u[s] = u[s] + v;
    }
}

// The two passes of the full multigrid start (mgp_batch_fmg; the definitions are mgp_fmg's in the header).

// R = the 2^d average of the stored field f in reduceResidual's term order (x fastest): a work item per coarse slot
template <typename T, int DIM>
__device__ __forceinline__ void restrict_field_part(const T* f, T* R, const MGeo& g, const MGeo& gc, int tid, int nt)
{
    const int n = gc.nz * gc.P;
    for (int q = tid; q < n; q += nt) {
        int I, J, K;
        if (!slot_of(q, gc, I, J, K)) continue;
        T s = (T)0;
#pragma unroll
        for (int d = 0; d < (1 << DIM); ++d) {
            const T v = f[pslot(g, 2 * I + (d & 1), 2 * J + ((d >> 1) & 1), DIM == 3 ? 2 * K + (d >> 2) : 0)];
            s = d == 0 ? v : s + v;
        }
        R[q] = (DIM == 2 ? (T)0.25 : (T)0.125) * s;
    }
}

// u = P3 V, mc = -(T)c of the coarse level: a work item per fine slot, the expressions of k_fmg_prolong_s (mgp_fmg.hip).
// In 3D the four z terms are computed one after the other and enter the z pass's sum as they come, ((wp z0 + wn z1) +
// wq z2) + wr z3 with every product and sum rounded as cub rounds them: 16 coarse samples are live, not 64, so the LDS
// ascent keeps the cycle's 1024-thread workgroup without spilling.
template <typename T, int DIM>
__device__ __forceinline__ void fmg_prolong_part(T* u, const T* V, const MGeo& g, const MGeo& gc, T mc, int tid, int nt)
{
    const int n = g.nz * g.P;
    for (int s = tid; s < n; s += nt) {
        int i, j, k;
        if (!slot_of(s, g, i, j, k)) continue;
        const int I = i >> 1, J = j >> 1, K = DIM == 3 ? (k >> 1) : 0;
        const int sx = (i & 1) ? 1 : -1, sy = (j & 1) ? 1 : -1, sz = (k & 1) ? 1 : -1;
        const int mz = DIM == 3 ? gc.nz : 1;
        T acc = (T)0;
#pragma unroll 1
        for (int tz = 0; tz < (DIM == 3 ? 4 : 1); ++tz) {
            const int dz = tz == 0 ? 0 : (tz == 1 ? sz : (tz == 2 ? -sz : 2 * sz));
            int nz_ = 0;
            const int Kq = DIM == 3 ? ext_src(K + dz, mz, nz_) : 0;
            T yt[4];
#pragma unroll
            for (int ty = 0; ty < 4; ++ty) {
                const int dy = ty == 0 ? 0 : (ty == 1 ? sy : (ty == 2 ? -sy : 2 * sy));
                int ny_;
                const int Jq = ext_src(J + dy, gc.ny, ny_);
                T xt[4];
#pragma unroll
                for (int tx = 0; tx < 4; ++tx) {
                    const int dx = tx == 0 ? 0 : (tx == 1 ? sx : (tx == 2 ? -sx : 2 * sx));
                    int nx_;
                    const int Iq = ext_src(I + dx, gc.nx, nx_);
                    xt[tx] = ext_scale(V[pslot(gc, Iq, Jq, Kq)], nx_, mc);
                }
                yt[ty] = ext_scale(cub(xt[0], xt[1], xt[2], xt[3]), ny_, mc);
            }
            const T zt = ext_scale(cub(yt[0], yt[1], yt[2], yt[3]), nz_, mc);
            if (DIM == 3) {
                const T w = tz == 0 ? W3<T>::wp : (tz == 1 ? W3<T>::wn : (tz == 2 ? W3<T>::wq : W3<T>::wr));
                const T p = w * zt;
                acc = tz == 0 ? p : acc + p;
            } else {
                acc = zt;
            }
        }
        u[s] = acc;
    }
}

// ---- one launch per piece: workgroups [m * nb, (m + 1) * nb) work on member m -----------------------------------

#define BATCH_MEMBER()                                                          \
    const int m = (int)(blockIdx.x / (unsigned)nb);                             \
    if (!active[m]) return;                                                     \
    const int tid = (int)(blockIdx.x - (unsigned)m * nb) * kBlock + (int)threadIdx.x;    \
    const int nt = nb * kBlock

template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_batch_sweep(const T* src, const T* f, T* dst, BLev<T, DIM> L, int c, int nb,
                                                        const int* __restrict__ active)
{
    BATCH_MEMBER();
    const int64_t o = (int64_t)m * L.slots;
    sweep_part<T, DIM>(src + o, f + o, dst + o, L, c, tid, nt);
}

template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_batch_rr(const T* u, const T* f, T* R, BLev<T, DIM> L, Geo gc, int nb,
                                                     const int* __restrict__ active)
{
    BATCH_MEMBER();
    const int64_t o = (int64_t)m * L.slots;
    rr_part<T, DIM>(u + o, f + o, R + (int64_t)m * (gc.nz * gc.P), L, gc, tid, nt);
}

template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_batch_prolong(T* u, const T* V, BLev<T, DIM> L, Geo gc, T clc, int linear,
                                                          int nb, const int* __restrict__ active)
{
    BATCH_MEMBER();
    prolong_part<T, DIM>(u + (int64_t)m * L.slots, V + (int64_t)m * (gc.nz * gc.P), L, gc, clc, linear, tid, nt);
}

// The full multigrid start's passes per piece (active == nullptr: every member, the ABI's two pieces).  The P3 onto a
// level whose coarse rows hold 16 bytes of reals runs mgp_fmg.hip's marching vector form (launch_fmg_prolong_batch).
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_batch_restrict_field(const T* f, T* R, Geo lg, Geo lgc, int nb,
                                                                 const int* __restrict__ active)
{
    const int m = (int)(blockIdx.x / (unsigned)nb);
    if (active && !active[m]) return;
    const int tid = (int)(blockIdx.x - (unsigned)m * nb) * kBlock + (int)threadIdx.x, nt = nb * kBlock;
    const MGeo g = mgeo(lg), gc = mgeo(lgc);
    restrict_field_part<T, DIM>(f + (int64_t)m * (g.nz * g.P), R + (int64_t)m * (gc.nz * gc.P), g, gc, tid, nt);
}

template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_batch_fmg_prolong(T* u, const T* V, Geo lg, Geo lgc, T mc, int nb,
                                                              const int* __restrict__ active)
{
    const int m = (int)(blockIdx.x / (unsigned)nb);
    if (active && !active[m]) return;
    const int tid = (int)(blockIdx.x - (unsigned)m * nb) * kBlock + (int)threadIdx.x, nt = nb * kBlock;
    const MGeo g = mgeo(lg), gc = mgeo(lgc);
    fmg_prolong_part<T, DIM>(u + (int64_t)m * (g.nz * g.P), V + (int64_t)m * (gc.nz * gc.P), g, gc, mc, tid, nt);
}

// dst = src (src == nullptr: +0) over a member's slots: the psiOld snapshot, a fresh coarse guess, a Jacobi level's
// result back into its u buffer
template <typename T>
__global__ __launch_bounds__(kBlock) void k_batch_copy(const T* src, T* dst, int64_t slots, int nb,
                                                       const int* __restrict__ active)
{
    BATCH_MEMBER();
    const int64_t o = (int64_t)m * slots;
    for (int64_t s = tid; s < slots; s += nt) dst[o + s] = src ? src[o + s] : (T)0;
}

// fp64 sums of one workgroup in a fixed order: per wave (butterfly), then the waves in order
template <int NV>
__device__ __forceinline__ void block_sums(double (&v)[NV], double* out, int stride)
{
    __shared__ double ws[NV][kBlock / 64];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        v[e] = wave_sum(v[e]);
        if ((threadIdx.x & 63) == 0) ws[e][threadIdx.x >> 6] = v[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            double a = ws[e][0];
            for (int w = 1; w < kBlock / 64; ++w) a += ws[e][w];
            out[(int64_t)e * stride] = a;
        }
    }
}

// partials[m * nb + p] = sum over workgroup p's cells of member m of (psi - psiOld)^2 (cpu.lua:203)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_batch_err(const T* u, const T* old, int64_t slots, int nb,
                                                      double* __restrict__ partials, const int* __restrict__ active)
{
    BATCH_MEMBER();
    const int64_t o = (int64_t)m * slots;
    double acc[1] = {0.0};
    for (int64_t s = tid; s < slots; s += nt) {
        const double d = (double)u[o + s] - (double)old[o + s];
        acc[0] += d * d;
    }
    block_sums<1>(acc, partials + blockIdx.x, 0);
}

// mgp_batch_remove_mean, one workgroup per member: out[m] = the fp64 sum of the member's cells (per thread, per wave,
// the waves in order), out[B + m] = that sum / cells
template <typename T>
__global__ __launch_bounds__(kBlock) void k_batch_mean_sum(const T* __restrict__ x, Geo lg, int64_t slots, double cells,
                                                           int B, double* __restrict__ out)
{
    const int m = (int)blockIdx.x;
    const MGeo g = mgeo(lg);
    const T* const xm = x + (int64_t)m * slots;
    double acc[1] = {0.0};
    for (int s = (int)threadIdx.x; s < g.nz * g.P; s += kBlock) {
        int i, j, k;
        if (slot_of(s, g, i, j, k)) acc[0] += (double)xm[s];
    }
    block_sums<1>(acc, out + m, 0);
    if (threadIdx.x == 0) out[B + m] = out[m] / cells;
}

// ... and every cell of member m becomes RN((double)x - mean[m]) (slots that hold no cell stay 0)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_batch_mean_sub(T* __restrict__ x, Geo lg, int64_t slots, int nb,
                                                           const double* __restrict__ mean)
{
    const int m = (int)(blockIdx.x / (unsigned)nb);
    const int tid = (int)(blockIdx.x - (unsigned)m * nb) * kBlock + (int)threadIdx.x, nt = nb * kBlock;
    const MGeo g = mgeo(lg);
    T* const xm = x + (int64_t)m * slots;
    const double mu = mean[m];
    for (int s = tid; s < g.nz * g.P; s += nt) {
        int i, j, k;
        if (slot_of(s, g, i, j, k)) xm[s] = (T)((double)xm[s] - mu);
    }
}

// partials[blockIdx.x] = sum (f - A u)^2, partials[total + blockIdx.x] = sum f^2 over the workgroup's cells
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_batch_resnorm(const T* u, const T* f, BLev<T, DIM> L, int nb,
                                                          double* __restrict__ partials)
{
    const int m = (int)(blockIdx.x / (unsigned)nb);
    const int tid = (int)(blockIdx.x - (unsigned)m * nb) * kBlock + (int)threadIdx.x, nt = nb * kBlock;
    const T* const um = u + (int64_t)m * L.slots;
    const T* const fm = f + (int64_t)m * L.slots;
    const MGeo g = mgeo(L.g);
    double acc[2] = {0.0, 0.0};
    for (int s = tid; s < g.nz * g.P; s += nt) {
        int i, j, k;
        if (!slot_of(s, g, i, j, k)) continue;
        int nbf;
        const T sum = nbsum<T, DIM>(um, g, s, i, j, k, nbf);
        const T r = L.op.residual(sum, fm[s], um[s], nbf);
        acc[0] += (double)r * (double)r;
        acc[1] += (double)fm[s] * (double)fm[s];
    }
    block_sums<2>(acc, partials + blockIdx.x, (int)gridDim.x);
}

// out[m] = the fixed-order sum of member m's nb partials
__global__ __launch_bounds__(kBlock) void k_batch_sum(const double* __restrict__ partials, int nb, int B,
                                                      double* __restrict__ out)
{
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= B) return;
    double a = 0.0;
    for (int p = 0; p < nb; ++p) a += partials[(int64_t)m * nb + p];
    out[m] = a;
}

// Per-member stop state (device memory, so one captured cycle serves mgp_batch_cycles and mgp_batch_solve)
struct BState {
    int* active;       // [B] 1 while the member iterates
    int* iters;        // [B] outer iterations done since the call began
    double* last_err;  // [B] err of the member's last iteration
    int* ctr;          // [0] cycle of the current chunk (the errs row); [1] 1: the stop rule is on (solve)
    double* eps;       // [0] epsilon
    double* errs;      // rows of B errs per cycle of the chunk
    int* nactive;      // host-mapped: active members after the last cycle
};

// The end of an outer iteration (cpu.lua:203-206, 211-214 per member): err = sqrt(sum / N), ++iters, and with the
// stop rule on the member leaves the iteration when err < epsilon or err is not finite
__global__ __launch_bounds__(kBlock) void k_batch_finish(const double* __restrict__ partials, int nb, int B, double ncells,
                                                         BState st)
{
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const int it = st.ctr[0], stop = st.ctr[1];
    const double eps = st.eps[0];
    int mine = 0;
    for (int m = threadIdx.x; m < B; m += kBlock) {
        if (st.active[m]) {
            double a = 0.0;
            for (int p = 0; p < nb; ++p) a += partials[(int64_t)m * nb + p];
            const double e = sqrt(a / ncells);
            st.last_err[m] = e;
            st.iters[m] += 1;
            if (stop && (e < eps || !isfinite(e)))
                st.active[m] = 0;
            else
                ++mine;
        }
        st.errs[(int64_t)it * B + m] = st.last_err[m];
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        *st.nactive = cnt;
        st.ctr[0] = it + 1;
    }
}

// every member active, no iterations done; stop: the stop rule of mgp_batch_solve with epsilon eps
__global__ __launch_bounds__(kBlock) void k_batch_arm(int B, int stop, double eps, BState st)
{
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m < B) {
        st.active[m] = 1;
        st.iters[m] = 0;
        st.last_err[m] = __builtin_nan("");
    }
    if (m == 0) {
        st.ctr[0] = 0;
        st.ctr[1] = stop;
        st.eps[0] = eps;
        *st.nactive = B;
    }
}

// f = -1e6 at the centre cell of every member, psi = -f (cpu.lua:180-193); the fields were zeroed before
template <typename T>
__global__ __launch_bounds__(kBlock) void k_batch_point_charge(T* u, T* f, Geo g, int64_t slots, int B, int ci, int cj,
                                                               int64_t ck)
{
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= B) return;
    const int64_t p = (int64_t)m * slots + pidx(g, ci, cj, ck);
    const T q = (T)(-1e6 / 1.0);
    f[p] = q;
    u[p] = -q;
}

// lexicographic (x fastest; member mm of the caller's buffer) <-> packed (member m0 + mm)
template <typename T, bool TO_PACKED>
__global__ __launch_bounds__(kBlock) void k_batch_pack(T* lex, T* packed, Geo g, int64_t slots, int64_t cells, int m0,
                                                       int nb)
{
    const int mm = (int)(blockIdx.x / (unsigned)nb);
    const int64_t tid = (int64_t)(blockIdx.x - (unsigned)mm * nb) * kBlock + threadIdx.x, nt = (int64_t)nb * kBlock;
    for (int64_t s = tid; s < slots; s += nt) {
        int i, j;
        int64_t k;
        if (!slot_cell(s, g, i, j, k)) continue;
        T* const a = lex + (int64_t)mm * cells + i + (int64_t)g.nx * (j + (int64_t)g.ny * k);
        T* const b = packed + (int64_t)(m0 + mm) * slots + s;
        if (TO_PACKED)
            *b = *a;
        else
            *a = *b;
    }
}

// ---- the LDS engine: one workgroup per member runs the coarse sub-cycle's op program --------------------------

template <typename T, int DIM>
struct BTail {
    int nlev, jacobi, linear, warm;
    int nops[2];                     // V / F program
    BLev<T, DIM> lev[kTailMaxLevels];
    int64_t off[kTailMaxLevels];     // the level's LDS offset in reals: u, then f, then (Jacobi) the target buffer
    T* u[kTailMaxLevels];            // global fields of all members (member stride = slots)
    T* f[kTailMaxLevels];
    uint32_t ops[2][kTailMaxOps];    // TailOp | level << 4 | arg << 8, levels relative to the first
    const uint32_t* fprog;           // the LDS ascent's program (mgp_batch_fmg; a device array of its own length)
    int nfprog;
};

// zero_first: the first level's u is a fresh zero guess (never read from memory)
// FMG: the LDS ascent of mgp_batch_fmg in place of a sub-cycle: the program sp->fprog (TAIL_FMG_RESTRICT down from the
// first level's f, the coarsest level zeroed and solved, then per level TAIL_FMG_PROLONG, TAIL_ZERO of the level below
// and the cycles' own ops).  Only the first level's f is loaded: every u is written before it is read (slots that hold
// no cell start as 0).  fcycle and zero_first are not read.  It runs with the cycle's workgroup size except in 3D fp64,
// where the residual + restriction already fills a 1024-thread workgroup's 128 registers (the cycle's instantiation
// spills there) and the ascent's further ops would spill more: at most 512 threads (256 registers), no scratch.
template <typename T, int DIM>
constexpr int tail_max_threads(bool fmg)
{
    return fmg && DIM == 3 && sizeof(T) == 8 ? 512 : 1024;
}
template <typename T, int DIM, bool FMG>
__global__ __launch_bounds__((tail_max_threads<T, DIM>(FMG))) void k_batch_tail(const BTail<T, DIM>* __restrict__ sp, int fcycle, int zero_first,
                                                     const int* __restrict__ active)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int m = blockIdx.x;
    if (!active[m]) return;
    T* const lds = reinterpret_cast<T*>(lds_raw);
    const BTail<T, DIM>& t = *sp;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    for (int l = 0; l < t.nlev; ++l) {
        const int64_t n = t.lev[l].slots;
        T* const lu = lds + t.off[l];
        if constexpr (FMG) {
            for (int64_t s = tid; s < n; s += nt) lu[s] = (T)0;
            if (t.jacobi)
                for (int64_t s = tid; s < n; s += nt) lu[2 * n + s] = (T)0;
        } else {
            const bool zero = l == 0 ? zero_first != 0 : !t.warm;
            const T* const gu = t.u[l] + (int64_t)m * n;
            for (int64_t s = tid; s < n; s += nt) lu[s] = zero ? (T)0 : gu[s];
        }
        if (l == 0) {
            const T* const gf = t.f[0] + (int64_t)m * n;
            for (int64_t s = tid; s < n; s += nt) lu[n + s] = gf[s];
        }
    }
    __syncthreads();
    unsigned in_t = 0;  // bit l: level l's current u is in its Jacobi target buffer
    const int nops = FMG ? t.nfprog : t.nops[fcycle];
    for (int p = 0; p < nops; ++p) {
        const uint32_t w = FMG ? t.fprog[p] : t.ops[fcycle][p];
        const int op = (int)(w & 15u), l = (int)((w >> 4) & 15u), arg = (int)(w >> 8);
        const BLev<T, DIM>& L = t.lev[l];
        const int64_t n = L.slots;
        T* const base = lds + t.off[l];
        T* const f = base + n;
        T* u = ((in_t >> l) & 1u) ? base + 2 * n : base;
        if (op == TAIL_SMOOTH) {
            for (int sw = 0; sw < arg; ++sw) {
                if (t.jacobi) {
                    T* const o = ((in_t >> l) & 1u) ? base : base + 2 * n;
                    sweep_part<T, DIM>(u, f, o, L, -1, tid, nt);
                    __syncthreads();
                    u = o;
                    in_t ^= 1u << l;
                } else {
                    sweep_part<T, DIM>(u, f, u, L, 0, tid, nt);
                    __syncthreads();
                    sweep_part<T, DIM>(u, f, u, L, 1, tid, nt);
                    __syncthreads();
                }
            }
        } else if (op == TAIL_RR) {
            rr_part<T, DIM>(u, f, lds + t.off[l + 1] + t.lev[l + 1].slots, L, t.lev[l + 1].g, tid, nt);
            __syncthreads();
        } else if (op == TAIL_ZERO) {
            for (int64_t s = tid; s < n; s += nt) u[s] = (T)0;
            __syncthreads();
        } else if (op == TAIL_PROLONG) {
            const int64_t nc = t.lev[l + 1].slots;
            const T* const V = lds + t.off[l + 1] + (((in_t >> (l + 1)) & 1u) ? 2 * nc : 0);
            prolong_part<T, DIM>(u, V, L, t.lev[l + 1].g, t.lev[l + 1].op.cl, t.linear, tid, nt);
            __syncthreads();
        } else if (FMG && op == TAIL_FMG_RESTRICT) {
            restrict_field_part<T, DIM>(f, lds + t.off[l + 1] + t.lev[l + 1].slots, mgeo(L.g), mgeo(t.lev[l + 1].g), tid, nt);
            __syncthreads();
        } else if (FMG && op == TAIL_FMG_PROLONG) {
            const int64_t nc = t.lev[l + 1].slots;
            const T* const V = lds + t.off[l + 1] + (((in_t >> (l + 1)) & 1u) ? 2 * nc : 0);
            fmg_prolong_part<T, DIM>(u, V, mgeo(L.g), mgeo(t.lev[l + 1].g), -t.lev[l + 1].op.cl, tid, nt);
            __syncthreads();
        }
    }
    // every level's u (level 0: the sub-cycle's result; below: Vs, the warm guess of the next cycle) and the
    // restricted residuals Rs
    for (int l = 0; l < t.nlev; ++l) {
        const int64_t n = t.lev[l].slots;
        const T* const base = lds + t.off[l];
        const T* const lu = ((in_t >> l) & 1u) ? base + 2 * n : base;
        T* const gu = t.u[l] + (int64_t)m * n;
        for (int64_t s = tid; s < n; s += nt) gu[s] = lu[s];
        if (l > 0) {
            T* const gf = t.f[l] + (int64_t)m * n;
            for (int64_t s = tid; s < n; s += nt) gf[s] = base[n + s];
        }
    }
}

thread_local std::string g_batch_error;

int ilog2(int64_t v)
{
    int l = 0;
    while ((int64_t(1) << l) < v) ++l;
    return l;
}

Geo member_geo(int64_t nx, int64_t ny, int64_t nz)
{
    Geo g;
    g.nx = (int)nx;
    g.ny = (int)ny;
    g.lx = ilog2(nx);
    g.ly = ilog2(ny);
    g.hw = nx >= 2 ? (int)(nx / 2) : 1;
    g.lhw = ilog2(g.hw);
    g.nz = nz;
    g.H = (int64_t)g.hw * g.ny;
    g.P = 2 * g.H;
    g.z0 = 0;
    g.gnz = nz;
    return g;
}


struct BHostLevel {
    Geo g;
    int64_t slots = 0, cells = 0;
    double h = 0, cl = 0;
    char *u = nullptr, *f = nullptr, *t = nullptr;  // all members; t: the Jacobi target (per-piece levels)
    int cur = 0;                                    // 1: the current u is in t (within a cycle)
};

}  // namespace
}  // namespace mgp

using mgp::BHostLevel;
using mgp::BState;
using mgp::Geo;
using mgp::g_batch_error;
using mgp::kBlock;

struct mgp_batch {
    mgp_opts o{};
    int B = 0, rb = 0, dim = 0;
    std::vector<BHostLevel> lev;
    int T = -1;  // first level of the LDS engine (-1: none)
    std::vector<uint32_t> ops[2];
    size_t tail_lds = 0;
    int tail_threads = 256;
    void* d_tail = nullptr;
    char* old = nullptr;  // psiOld of every member (err_mode 1)
    BState st{};
    int* h_nactive = nullptr;
    double* d_part = nullptr;  // err partials B * nbe; the norms' 2 * B * nbe
    double* d_norm = nullptr;  // 2 * B
    int nbe = 1;
    int64_t chunk = 1;  // cycles per errs buffer
    hipStream_t s = nullptr;
    bool use_graph = true;
    hipGraphExec_t exec = nullptr;
    int64_t launches = 0, last_launches = 0;
    // mgp_batch_fmg: the LDS ascent's program and the captured ascent, each for the last cycles_per_level used
    uint32_t* d_fprog = nullptr;
    int fprog_cycles = 0;         // 0: none built
    bool fprog_piece = false;     // the program is over kFmgMaxOps: the tail levels' ascent runs per piece
    hipGraphExec_t fmg_exec = nullptr;
    int fmg_exec_cycles = 0;
    int64_t fmg_launches = 0;
    bool old_stale = false;       // psiOld describes an iterate that is gone (until the next outer iteration)
    mutable std::string err;

    int fail(int code, const char* fmt, ...) const
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

#define BHIP(b, expr)                                                                                              \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess)                                                                                      \
            return (b)->fail(MGP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define BTRY(expr)                     \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != MGP_OK) return rc_; \
    } while (0)

namespace {

// Options a batch refuses (before any device call), then the ordinary context's own validation; rows as mgp_plan
int batch_validate(const mgp_opts* o, int32_t batch, std::vector<int64_t>& rows, int& nlev, std::string& err)
{
    if (!o) {
        err = "null mgp_opts";
        return MGP_ERR_ARG;
    }
    if (o->struct_size != (int32_t)sizeof(mgp_opts)) {
        err = "mgp_opts.struct_size mismatch (header/library version skew): fill the struct with this library's "
              "mgp_opts_default";
        return MGP_ERR_ARG;
    }
    if (batch < 1) {
        err = "batch must be >= 1";
        return MGP_ERR_ARG;
    }
    if (o->world != 1) {
        err = "world must be 1: a batch lives on one GPU";
        return MGP_ERR_ARG;
    }
    if (o->smoother == MGP_GS_LEX) {
        err = "smoother MGP_GS_LEX is not batched (Jacobi or red/black Gauss-Seidel)";
        return MGP_ERR_ARG;
    }
    if (o->arith != MGP_ARITH_REAL) {
        err = "arith must be MGP_ARITH_REAL: cpu-raw.lua's double arithmetic (MGP_ARITH_DOUBLE) is not batched";
        return MGP_ERR_ARG;
    }
    if (o->restriction != MGP_RESTRICT_AVERAGE) {
        err = "restriction MGP_RESTRICT_FULL_WEIGHTING is not batched (MGP_RESTRICT_AVERAGE only)";
        return MGP_ERR_ARG;
    }
    rows.assign(8 * 48, 0);
    nlev = mgp_plan(o, rows.data(), 48);
    if (nlev < 0) {
        const char* m = mgp_last_error(nullptr);
        err = m ? m : "invalid options";
        return nlev;
    }
    const int64_t cells = rows[0] * rows[1] * rows[2];
    if (cells > (int64_t(1) << 24)) {
        err = "n: a member of more than 2^24 cells is not batched (one such box fills the GPU: use mgp_create)";
        return MGP_ERR_ARG;
    }
    if ((int64_t)batch * cells >= (int64_t(1) << 31)) {
        err = "batch * cells of a member (n) must be < 2^31";
        return MGP_ERR_ARG;
    }
    return MGP_OK;
}

// The ops of the cycle from level l down for the LDS engine, levels relative to T (the ordinary tail's program)
void tail_gen(const mgp_batch* b, int T, int l, bool fcycle, std::vector<uint32_t>& ops)
{
    auto emit = [&](int op, int lv, int arg) {
        ops.push_back((uint32_t)op | ((uint32_t)(lv - T) << 4) | ((uint32_t)arg << 8));
    };
    const int last = (int)b->lev.size() - 1;
    if (l == last) {
        emit(mgp::TAIL_SMOOTH, l, b->lev[l].cells == 1 ? 1 : b->o.coarse_sweeps);
        return;
    }
    emit(mgp::TAIL_SMOOTH, l, b->o.nu1);
    emit(mgp::TAIL_RR, l, 0);
    if (b->o.coarse_init == MGP_COARSE_FRESH) emit(mgp::TAIL_ZERO, l + 1, 0);
    if (fcycle) tail_gen(b, T, l + 1, true, ops);
    tail_gen(b, T, l + 1, false, ops);
    emit(mgp::TAIL_PROLONG, l, 0);
    emit(mgp::TAIL_SMOOTH, l, b->o.nu2);
}

size_t tail_bytes(const mgp_batch* b, int T)
{
    int64_t reals = 0;
    for (size_t l = T; l < b->lev.size(); ++l) reals += b->lev[l].slots * (b->o.smoother == MGP_JACOBI ? 3 : 2);
    return (size_t)reals * b->rb;
}

// The first level of <= kTailCells cells whose sub-hierarchy fits one workgroup's LDS and the op budget
// (MGP_TAIL=0: none, every level one launch per piece)
void plan_tail(mgp_batch* b)
{
    b->T = -1;
    const char* v = std::getenv("MGP_TAIL");
    if (v && std::atoi(v) == 0) return;
    const int n = (int)b->lev.size();
    for (int T = 0; T < n; ++T) {
        if (b->lev[T].cells > mgp::kTailCells || n - T > mgp::kTailMaxLevels) continue;
        if (tail_bytes(b, T) > mgp::kTailMaxLds) continue;
        std::vector<uint32_t> pv, pf;
        tail_gen(b, T, T, false, pv);
        tail_gen(b, T, T, true, pf);
        if ((int)pv.size() > mgp::kTailMaxOps || (int)pf.size() > mgp::kTailMaxOps) continue;
        if (std::max(b->o.nu1, std::max(b->o.nu2, b->o.coarse_sweeps)) >= (1 << 24)) continue;  // (an op's arg has 24 bits)
        b->T = T;
        b->ops[0] = pv;
        b->ops[1] = pf;
        b->tail_lds = tail_bytes(b, T);
        b->tail_threads = b->lev[T].slots >= 2048 ? 1024 : 256;
        return;
    }
}

void host_plan(mgp_batch* b, const mgp_opts& o, int32_t batch, const std::vector<int64_t>& rows, int nlev)
{
    b->o = o;
    if (o.dim == 2) b->o.n[2] = 1;
    b->B = batch;
    b->rb = o.real_bytes;
    b->dim = o.dim;
    for (int l = 0; l < nlev; ++l) {
        BHostLevel L;
        const int64_t* r = rows.data() + 8 * l;
        L.g = mgp::member_geo(r[0], r[1], o.dim == 3 ? r[2] : 1);
        L.cells = r[0] * r[1] * (o.dim == 3 ? r[2] : 1);
        L.slots = L.g.nz * L.g.P;
        L.h = std::ldexp(1.0, l) / (double)rows[0];  // cpu.lua:197-198, doubled per level
        L.cl = mgp::coarse_coef(o.coarse_bc, l);
        b->lev.push_back(L);
    }
    plan_tail(b);
    b->nbe = (int)std::min<int64_t>(mgp::kErrBlocks, (b->lev[0].slots + kBlock - 1) / kBlock);
    b->chunk = std::max<int64_t>(1, (int64_t(1) << 20) / batch);
}

template <typename T, int DIM>
mgp::BLev<T, DIM> dev_level(const BHostLevel& L)
{
    mgp::BLev<T, DIM> d;
    d.g = L.g;
    d.op = mgp::make_op<T, DIM>(L.h, L.cl);
    d.slots = L.slots;
    return d;
}

// fn(T{}, std::integral_constant<int, DIM>{}) for the batch's real type and dimension
template <typename F>
int dispatch(const mgp_batch* b, F&& fn)
{
    using D2 = std::integral_constant<int, 2>;
    using D3 = std::integral_constant<int, 3>;
    if (b->rb == 4) return b->dim == 2 ? fn(float{}, D2{}) : fn(float{}, D3{});
    return b->dim == 2 ? fn(double{}, D2{}) : fn(double{}, D3{});
}

// workgroups per member for a thread per item
int piece_blocks(int64_t items) { return (int)std::max<int64_t>(1, (items + kBlock - 1) / kBlock); }

#define BLAUNCH(b, kernel, grid, block, lds, ...)                    \
    do {                                                             \
        kernel<<<dim3((unsigned)(grid)), dim3(block), lds, (b)->s>>>(__VA_ARGS__); \
        BHIP(b, hipGetLastError());                                  \
        ++(b)->launches;                                             \
    } while (0)

template <typename T, int DIM>
struct Cycle {
    mgp_batch* b;
    const int* active() const { return b->st.active; }
    T* U(int l) const { return (T*)(b->lev[l].cur ? b->lev[l].t : b->lev[l].u); }
    T* F(int l) const { return (T*)b->lev[l].f; }

    int smooth(int l, int sweeps)
    {
        BHostLevel& L = b->lev[l];
        const auto dl = dev_level<T, DIM>(L);
        for (int sw = 0; sw < sweeps; ++sw) {
            if (b->o.smoother == MGP_JACOBI) {
                const int nb = piece_blocks(L.slots);
                T* const src = U(l);
                L.cur ^= 1;
                BLAUNCH(b, (mgp::k_batch_sweep<T, DIM>), (int64_t)b->B * nb, kBlock, 0, src, F(l), U(l), dl, -1, nb, active());
            } else {
                const int nb = piece_blocks(L.g.nz * L.g.H);
                for (int c = 0; c < 2; ++c)
                    BLAUNCH(b, (mgp::k_batch_sweep<T, DIM>), (int64_t)b->B * nb, kBlock, 0, U(l), F(l), U(l), dl, c, nb, active());
            }
        }
        return MGP_OK;
    }
    int copy(const T* src, T* dst, int64_t slots)
    {
        const int nb = piece_blocks(slots);
        BLAUNCH(b, (mgp::k_batch_copy<T>), (int64_t)b->B * nb, kBlock, 0, src, dst, slots, nb, active());
        return MGP_OK;
    }
    // cpu.lua:70-165 from level l; zero: level l's guess is a fresh zero (cpu.lua:138)
    int rec(int l, bool fcycle, bool zero)
    {
        const int last = (int)b->lev.size() - 1;
        BHostLevel& L = b->lev[l];
        if (l == b->T) {
            BLAUNCH(b, (mgp::k_batch_tail<T, DIM, false>), b->B, b->tail_threads, b->tail_lds,
                    (const mgp::BTail<T, DIM>*)b->d_tail, fcycle ? 1 : 0, zero ? 1 : 0, active());
            return MGP_OK;
        }
        if (zero) {
            L.cur = 0;
            BTRY(copy(nullptr, U(l), L.slots));
        }
        if (l == last) return smooth(l, L.cells == 1 ? 1 : b->o.coarse_sweeps);
        BHostLevel& C = b->lev[l + 1];
        BTRY(smooth(l, b->o.nu1));
        {
            const int nb = piece_blocks(C.slots);
            BLAUNCH(b, (mgp::k_batch_rr<T, DIM>), (int64_t)b->B * nb, kBlock, 0, U(l), F(l), F(l + 1), (dev_level<T, DIM>(L)), C.g,
                    nb, active());
        }
        const bool fresh = b->o.coarse_init == MGP_COARSE_FRESH;
        if (fcycle) {
            BTRY(rec(l + 1, true, fresh));
            BTRY(rec(l + 1, false, false));
        } else {
            BTRY(rec(l + 1, false, fresh));
        }
        {
            const int nb = piece_blocks(L.slots);
            const T clc = mgp::make_op<T, DIM>(C.h, C.cl).cl;
            BLAUNCH(b, (mgp::k_batch_prolong<T, DIM>), (int64_t)b->B * nb, kBlock, 0, U(l), U(l + 1), (dev_level<T, DIM>(L)), C.g,
                    clc, b->o.prolong == MGP_PROLONG_LINEAR ? 1 : 0, nb, active());
        }
        return smooth(l, b->o.nu2);
    }
    // an odd number of Jacobi sweeps leaves a level's result in its target buffer: back into u
    int fold()
    {
        for (auto& L : b->lev)
            if (L.cur) {
                BTRY(copy((const T*)L.t, (T*)L.u, L.slots));
                L.cur = 0;
            }
        return MGP_OK;
    }
    // f of level l + 1 = R f of level l; act: the members it runs on (nullptr: all)
    int fmg_restrict(int l, const int* act)
    {
        const BHostLevel& L = b->lev[l];
        const BHostLevel& C = b->lev[l + 1];
        const int nb = piece_blocks(C.slots);
        BLAUNCH(b, (mgp::k_batch_restrict_field<T, DIM>), (int64_t)b->B * nb, kBlock, 0, F(l), F(l + 1), L.g, C.g, nb, act);
        return MGP_OK;
    }
    // the current u of level l = P3 (the current u of level l + 1): the marching vector form where a coarse row holds
    // 16 bytes of reals, the scalar part function below that
    int fmg_p3(int l, const int* act)
    {
        const BHostLevel& L = b->lev[l];
        const BHostLevel& C = b->lev[l + 1];
        if ((int64_t)C.g.nx * b->rb >= 16) {
            BHIP(b, mgp::launch_fmg_prolong_batch(b->rb, DIM, U(l), U(l + 1), L.g, C.g, C.cl, b->B, L.slots, C.slots, act, b->s));
            ++b->launches;
        } else {
            const int nb = piece_blocks(L.slots);
            BLAUNCH(b, (mgp::k_batch_fmg_prolong<T, DIM>), (int64_t)b->B * nb, kBlock, 0, U(l), U(l + 1), L.g, C.g, -(T)C.cl, nb,
                    act);
        }
        return MGP_OK;
    }
    int zero_level(int l)
    {
        BHostLevel& L = b->lev[l];
        L.cur = 0;
        return copy(nullptr, U(l), L.slots);
    }
    // Steps 1-4 of mgp_fmg on every armed member.  The levels from T down are ONE launch (the LDS ascent: the
    // restrictions from T, the coarse solve, every P3 and per-level cycle up to level T); with no LDS engine, or a
    // program over kFmgMaxOps, they run per piece like the levels above.
    int fmg_ascent(int cycles)
    {
        const int last = (int)b->lev.size() - 1, T0 = b->T;
        const bool fcycle = b->o.cycle == MGP_CYCLE_F;
        const bool lds = T0 >= 0 && !b->fprog_piece;
        for (int l = 0; l < (lds ? T0 : last); ++l) BTRY(fmg_restrict(l, active()));
        int from;  // the first level a per-piece P3 writes
        if (lds) {
            BLAUNCH(b, (mgp::k_batch_tail<T, DIM, true>), b->B, std::min(b->tail_threads, mgp::tail_max_threads<T, DIM>(true)),
                    b->tail_lds,
                    (const mgp::BTail<T, DIM>*)b->d_tail, 0, 0, active());
            from = T0 - 1;
        } else {
            BTRY(zero_level(last));
            BTRY(smooth(last, b->lev[last].cells == 1 ? 1 : b->o.coarse_sweeps));
            from = last - 1;
        }
        for (int l = from; l >= 0; --l) {
            BTRY(fmg_p3(l, active()));
            BTRY(zero_level(l + 1));
            if (l == 0) break;
            for (int k = 0; k < cycles; ++k) BTRY(rec(l, fcycle, false));
            if (!lds && T0 >= 0) BTRY(fold());  // (the LDS engine's cycle reads its levels' u buffers)
        }
        return fold();
    }
    // One outer iteration of every active member (cpu.lua:196-206)
    int outer()
    {
        BHostLevel& L0 = b->lev[0];
        if (b->o.err_mode) BTRY(copy((const T*)L0.u, (T*)b->old, L0.slots));
        BTRY(rec(0, b->o.cycle == MGP_CYCLE_F, false));
        BTRY(fold());
        if (b->o.err_mode) {
            BLAUNCH(b, (mgp::k_batch_err<T>), (int64_t)b->B * b->nbe, kBlock, 0, (const T*)L0.u, (const T*)b->old, L0.slots, b->nbe,
                    b->d_part, active());
            BLAUNCH(b, mgp::k_batch_finish, 1, kBlock, 0, b->d_part, b->nbe, b->B, (double)L0.cells, b->st);
        }
        return MGP_OK;
    }
};

int enqueue_outer(mgp_batch* b)
{
    return dispatch(b, [&](auto t, auto d) {
        Cycle<decltype(t), decltype(d)::value> c{b};
        return c.outer();
    });
}

// k outer iterations on the stream: replays of the one captured cycle (a single linear chain), or eager launches
int enqueue_cycles(mgp_batch* b, int k)
{
    if (b->use_graph && !b->exec) {
        BHIP(b, hipStreamBeginCapture(b->s, hipStreamCaptureModeThreadLocal));
        b->launches = 0;
        const int rc = enqueue_outer(b);
        hipGraph_t graph = nullptr;
        const hipError_t ec = hipStreamEndCapture(b->s, &graph);
        if (rc != MGP_OK) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        BHIP(b, ec);
        const hipError_t ei = hipGraphInstantiate(&b->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        BHIP(b, ei);
        b->last_launches = b->launches;
    }
    for (int i = 0; i < k; ++i) {
        if (b->exec) {
            BHIP(b, hipGraphLaunch(b->exec, b->s));
        } else {
            b->launches = 0;
            BTRY(enqueue_outer(b));
            b->last_launches = b->launches;
        }
    }
    return MGP_OK;
}

// The LDS ascent's program for `cycles` cycles per level, levels relative to T; generation stops once it is over `cap`
void fmg_gen(const mgp_batch* b, int cycles, size_t cap, std::vector<uint32_t>& ops)
{
    const int T = b->T, last = (int)b->lev.size() - 1;
    const bool fcycle = b->o.cycle == MGP_CYCLE_F;
    auto emit = [&](int op, int lv) { ops.push_back((uint32_t)op | ((uint32_t)(lv - T) << 4)); };
    for (int l = T; l < last; ++l) emit(mgp::TAIL_FMG_RESTRICT, l);
    emit(mgp::TAIL_ZERO, last);
    tail_gen(b, T, last, false, ops);
    for (int l = last - 1; l >= T; --l) {
        emit(mgp::TAIL_FMG_PROLONG, l);
        emit(mgp::TAIL_ZERO, l + 1);
        for (int k = 0; k < cycles && l >= 1; ++k) {
            tail_gen(b, T, l, fcycle, ops);
            if (ops.size() > cap) return;
        }
    }
}

// A program longer than this runs the tail levels' ascent per piece (cycles_per_level <= 2 stays far below it on every
// tail plan_tail admits: at most 1100 ops for 8 levels and F-cycles)
constexpr size_t kFmgMaxOps = 4096;

// What the ascent needs before it is enqueued (never inside a capture): the program on the device, or, when it runs
// the tail levels per piece, their Jacobi target buffers
int fmg_prepare(mgp_batch* b, int cycles)
{
    if (b->T < 0) return MGP_OK;
    if (b->fprog_cycles != cycles) {
        std::vector<uint32_t> ops;
        fmg_gen(b, cycles, kFmgMaxOps, ops);
        BHIP(b, hipStreamSynchronize(b->s));
        b->fprog_cycles = 0;
        b->fprog_piece = ops.size() > kFmgMaxOps;
        if (!b->fprog_piece) {
            if (b->d_fprog) (void)hipFree(b->d_fprog);
            b->d_fprog = nullptr;
            if (hipMalloc((void**)&b->d_fprog, ops.size() * sizeof(uint32_t)) != hipSuccess) {
                (void)hipGetLastError();
                return b->fail(MGP_ERR_OOM, "hipMalloc failed for the ascent's program (%zu ops)", ops.size());
            }
            BHIP(b, hipMemcpy(b->d_fprog, ops.data(), ops.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            struct {
                const uint32_t* fprog;
                int nfprog;
            } ref{b->d_fprog, (int)ops.size()};  // BTail's last two members, uploaded together
            BTRY(dispatch(b, [&](auto t, auto d) {
                using BT = mgp::BTail<decltype(t), decltype(d)::value>;
                static_assert(offsetof(BT, nfprog) == offsetof(BT, fprog) + sizeof(ref.fprog), "fprog, nfprog are adjacent");
                BHIP(b, hipMemcpy((char*)b->d_tail + offsetof(BT, fprog), &ref, sizeof(ref.fprog) + sizeof(ref.nfprog),
                                  hipMemcpyHostToDevice));
                return (int)MGP_OK;
            }));
        }
        b->fprog_cycles = cycles;
    }
    if (b->fprog_piece && b->o.smoother == MGP_JACOBI)
        for (size_t l = b->T; l < b->lev.size(); ++l) {
            BHostLevel& L = b->lev[l];
            if (L.t) continue;
            const size_t bytes = (size_t)b->B * L.slots * b->rb;
            if (hipMalloc((void**)&L.t, bytes) != hipSuccess) {
                L.t = nullptr;
                (void)hipGetLastError();
                return b->fail(MGP_ERR_OOM, "hipMalloc failed for the Jacobi buffer of level %d", (int)l);
            }
            BHIP(b, hipMemset(L.t, 0, bytes));
        }
    return MGP_OK;
}

// (a pass that fails part-way leaves the Jacobi levels' host-side buffer toggles where it stopped: back to u)
int enqueue_ascent_once(mgp_batch* b, int cycles)
{
    const int rc = dispatch(b, [&](auto t, auto d) {
        Cycle<decltype(t), decltype(d)::value> c{b};
        return c.fmg_ascent(cycles);
    });
    if (rc != MGP_OK)
        for (auto& L : b->lev) L.cur = 0;
    return rc;
}

// The ascent on the stream: a replay of its captured graph (one linear chain, kept for the last cycles_per_level), or
// eager launches
int enqueue_ascent(mgp_batch* b, int cycles)
{
    BTRY(fmg_prepare(b, cycles));
    if (b->use_graph && (!b->fmg_exec || b->fmg_exec_cycles != cycles)) {
        if (b->fmg_exec) {
            BHIP(b, hipStreamSynchronize(b->s));
            (void)hipGraphExecDestroy(b->fmg_exec);
            b->fmg_exec = nullptr;
        }
        BHIP(b, hipStreamBeginCapture(b->s, hipStreamCaptureModeThreadLocal));
        b->launches = 0;
        const int rc = enqueue_ascent_once(b, cycles);
        hipGraph_t graph = nullptr;
        const hipError_t ec = hipStreamEndCapture(b->s, &graph);
        if (rc != MGP_OK) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        BHIP(b, ec);
        const hipError_t ei = hipGraphInstantiate(&b->fmg_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        BHIP(b, ei);
        b->fmg_exec_cycles = cycles;
        b->fmg_launches = b->launches;
    }
    if (b->fmg_exec) {
        BHIP(b, hipGraphLaunch(b->fmg_exec, b->s));
    } else {
        b->launches = 0;
        BTRY(enqueue_ascent_once(b, cycles));
        b->fmg_launches = b->launches;
    }
    return MGP_OK;
}

int arm(mgp_batch* b, int stop, double eps)
{
    mgp::k_batch_arm<<<dim3((unsigned)((b->B + kBlock - 1) / kBlock)), dim3(kBlock), 0, b->s>>>(b->B, stop, eps, b->st);
    BHIP(b, hipGetLastError());
    return MGP_OK;
}

void batch_free(mgp_batch* b)
{
    if (!b) return;
    if (b->exec) (void)hipGraphExecDestroy(b->exec);
    if (b->fmg_exec) (void)hipGraphExecDestroy(b->fmg_exec);
    for (auto& L : b->lev) {
        if (L.u) (void)hipFree(L.u);
        if (L.f) (void)hipFree(L.f);
        if (L.t) (void)hipFree(L.t);
    }
    for (void* p : {(void*)b->old, (void*)b->d_tail, (void*)b->st.active, (void*)b->st.iters, (void*)b->st.last_err,
                    (void*)b->st.ctr, (void*)b->st.eps, (void*)b->st.errs, (void*)b->d_part, (void*)b->d_norm, (void*)b->d_fprog})
        if (p) (void)hipFree(p);
    if (b->h_nactive) (void)hipHostFree(b->h_nactive);
    if (b->s) (void)hipStreamDestroy(b->s);
    delete b;
}

template <typename T, int DIM>
int upload_tail(mgp_batch* b)
{
    auto* t = new mgp::BTail<T, DIM>();
    const int T0 = b->T;
    t->nlev = (int)b->lev.size() - T0;
    t->jacobi = b->o.smoother == MGP_JACOBI;
    t->linear = b->o.prolong == MGP_PROLONG_LINEAR;
    t->warm = b->o.coarse_init == MGP_COARSE_WARM;
    int64_t off = 0;
    for (int i = 0; i < t->nlev; ++i) {
        const BHostLevel& L = b->lev[T0 + i];
        t->lev[i] = dev_level<T, DIM>(L);
        t->off[i] = off;
        off += L.slots * (t->jacobi ? 3 : 2);
        t->u[i] = (T*)L.u;
        t->f[i] = (T*)L.f;
    }
    for (int p = 0; p < 2; ++p) {
        t->nops[p] = (int)b->ops[p].size();
        std::copy(b->ops[p].begin(), b->ops[p].end(), t->ops[p]);
    }
    hipError_t e = hipMalloc(&b->d_tail, sizeof(*t));
    if (e == hipSuccess) e = hipMemcpy(b->d_tail, t, sizeof(*t), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)mgp::k_batch_tail<T, DIM, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)mgp::kTailMaxLds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)mgp::k_batch_tail<T, DIM, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)mgp::kTailMaxLds);
    delete t;
    if (e == hipErrorOutOfMemory) return b->fail(MGP_ERR_OOM, "hipMalloc failed for the coarse program");
    BHIP(b, e);
    return MGP_OK;
}

int field_ptr(const mgp_batch* b, int member, int level, int which, int64_t count, bool set, char** base, int* m0, int* nm)
{
    if (level < 0 || level >= (int)b->lev.size()) return b->fail(MGP_ERR_ARG, "level %d out of range", level);
    if (member < -1 || member >= b->B) return b->fail(MGP_ERR_ARG, "member %d out of range (batch %d)", member, b->B);
    const BHostLevel& L = b->lev[level];
    *m0 = member < 0 ? 0 : member;
    *nm = member < 0 ? b->B : 1;
    if (count != (int64_t)*nm * L.cells)
        return b->fail(MGP_ERR_ARG, "count %lld != %lld (members x the level's cells)", (long long)count,
                       (long long)((int64_t)*nm * L.cells));
    if (which == MGP_FIELD_U)
        *base = L.u;
    else if (which == MGP_FIELD_F)
        *base = L.f;
    else if (which == MGP_FIELD_PSI_OLD && level == 0 && !set) {
        if (!b->o.err_mode) return b->fail(MGP_ERR_STATE, "MGP_FIELD_PSI_OLD needs err_mode 1");
        if (b->old_stale)
            return b->fail(MGP_ERR_STATE, "MGP_FIELD_PSI_OLD: psi was replaced by the full multigrid start; psiOld is "
                                          "valid again after the next outer iteration");
        *base = b->old;
    } else
        return b->fail(MGP_ERR_ARG, "field %d is not %s on a batch", which, set ? "writable" : "readable");
    return MGP_OK;
}

// caller buffer (host or device, lexicographic per member) <-> the packed members
int field_io(mgp_batch* b, int member, int level, int which, void* buf, int64_t count, int mem, bool set)
{
    if (!b) return MGP_ERR_ARG;
    if (!buf) return b->fail(MGP_ERR_ARG, "null buffer");
    if (mem != MGP_MEM_HOST && mem != MGP_MEM_DEVICE) return b->fail(MGP_ERR_ARG, "mem must be MGP_MEM_HOST or MGP_MEM_DEVICE");
    char* base;
    int m0, nm;
    BTRY(field_ptr(b, member, level, which, count, set, &base, &m0, &nm));
    const BHostLevel& L = b->lev[level];
    const size_t bytes = (size_t)count * b->rb;
    void* stage = nullptr;
    if (mem == MGP_MEM_HOST) {
        if (hipMalloc(&stage, bytes) != hipSuccess) return b->fail(MGP_ERR_OOM, "hipMalloc failed for the staging buffer");
        if (set) {
            const hipError_t e = hipMemcpyAsync(stage, buf, bytes, hipMemcpyHostToDevice, b->s);
            if (e != hipSuccess) {
                (void)hipFree(stage);
                BHIP(b, e);
            }
        }
    }
    void* lex = stage ? stage : buf;
    const int nb = piece_blocks(L.slots);
    const unsigned grid = (unsigned)((int64_t)nm * nb);
    hipError_t e;
    if (b->rb == 4) {
        if (set)
            mgp::k_batch_pack<float, true><<<dim3(grid), dim3(kBlock), 0, b->s>>>((float*)lex, (float*)base, L.g, L.slots, L.cells, m0, nb);
        else
            mgp::k_batch_pack<float, false><<<dim3(grid), dim3(kBlock), 0, b->s>>>((float*)lex, (float*)base, L.g, L.slots, L.cells, m0, nb);
    } else {
        if (set)
            mgp::k_batch_pack<double, true><<<dim3(grid), dim3(kBlock), 0, b->s>>>((double*)lex, (double*)base, L.g, L.slots, L.cells, m0, nb);
        else
            mgp::k_batch_pack<double, false><<<dim3(grid), dim3(kBlock), 0, b->s>>>((double*)lex, (double*)base, L.g, L.slots, L.cells, m0, nb);
    }
    e = hipGetLastError();
    if (e == hipSuccess && stage && !set) e = hipMemcpyAsync(buf, stage, bytes, hipMemcpyDeviceToHost, b->s);
    if (e == hipSuccess) e = hipStreamSynchronize(b->s);
    if (stage) (void)hipFree(stage);
    BHIP(b, e);
    return MGP_OK;
}

// k outer iterations of the armed members and the one synchronisation at the end (one more per full errs buffer);
// sync = false (errs == nullptr): the caller enqueues more and synchronises itself
int cycles_armed(mgp_batch* b, int32_t k, double* errs, bool sync = true)
{
    if (k > 0) b->old_stale = false;
    for (int64_t done = 0; done < k;) {
        const int n = (int)std::min<int64_t>(b->chunk, k - done);
        BHIP(b, hipMemsetAsync(b->st.ctr, 0, sizeof(int), b->s));
        BTRY(enqueue_cycles(b, n));
        if (errs && b->o.err_mode)
            BHIP(b, hipMemcpyAsync(errs + done * b->B, b->st.errs, sizeof(double) * (size_t)n * b->B, hipMemcpyDeviceToHost,
                                   b->s));
        if (done + n < k) BHIP(b, hipStreamSynchronize(b->s));  // (the errs buffer is reused by the next chunk)
        done += n;
    }
    if (!sync) return MGP_OK;
    BHIP(b, hipStreamSynchronize(b->s));
    if (errs && !b->o.err_mode)
        for (int64_t i = 0; i < (int64_t)k * b->B; ++i) errs[i] = NAN;
    return MGP_OK;
}

// d_norm[m] = sum (f - A u)^2, d_norm[B + m] = sum f^2 of member m on level 0 (mgp_batch_residual_norm's passes)
int resnorm_enqueue(mgp_batch* b)
{
    const BHostLevel& L = b->lev[0];
    const int nb = b->nbe;
    const int64_t total = (int64_t)b->B * nb;
    BTRY(dispatch(b, [&](auto t, auto d) {
        using T = decltype(t);
        constexpr int DIM = decltype(d)::value;
        mgp::k_batch_resnorm<T, DIM><<<dim3((unsigned)total), dim3(kBlock), 0, b->s>>>((const T*)L.u, (const T*)L.f,
                                                                                     dev_level<T, DIM>(L), nb, b->d_part);
        BHIP(b, hipGetLastError());
        return (int)MGP_OK;
    }));
    const unsigned g = (unsigned)((b->B + kBlock - 1) / kBlock);
    mgp::k_batch_sum<<<dim3(g), dim3(kBlock), 0, b->s>>>(b->d_part, nb, b->B, b->d_norm);
    BHIP(b, hipGetLastError());
    mgp::k_batch_sum<<<dim3(g), dim3(kBlock), 0, b->s>>>(b->d_part + total, nb, b->B, b->d_norm + b->B);
    BHIP(b, hipGetLastError());
    return MGP_OK;
}

// every member's cells of a level's field lose the member's own mean; d_norm[B + m] = the mean (mgp_batch_remove_mean's
// passes)
int mean_enqueue(mgp_batch* b, const BHostLevel& L, char* base)
{
    const int nb = piece_blocks(L.slots);
    const unsigned grid = (unsigned)((int64_t)b->B * nb);
    if (b->rb == 4) {
        mgp::k_batch_mean_sum<float><<<dim3((unsigned)b->B), dim3(kBlock), 0, b->s>>>((const float*)base, L.g, L.slots,
                                                                                     (double)L.cells, b->B, b->d_norm);
        mgp::k_batch_mean_sub<float><<<dim3(grid), dim3(kBlock), 0, b->s>>>((float*)base, L.g, L.slots, nb, b->d_norm + b->B);
    } else {
        mgp::k_batch_mean_sum<double><<<dim3((unsigned)b->B), dim3(kBlock), 0, b->s>>>((const double*)base, L.g, L.slots,
                                                                                      (double)L.cells, b->B, b->d_norm);
        mgp::k_batch_mean_sub<double><<<dim3(grid), dim3(kBlock), 0, b->s>>>((double*)base, L.g, L.slots, nb, b->d_norm + b->B);
    }
    BHIP(b, hipGetLastError());
    return MGP_OK;
}

// ---- MAC-grid projection of the members (mgp_project.hip's k_div_b / k_grad_b; the header has the definitions) ----

// The caller's face arrays of nm members as device pointers for one call: device memory as it is, host memory through
// buffers allocated here (uploaded when the call reads the faces) and freed when the call returns
struct BatchFaces {
    mgp_batch* b;
    void* host[3] = {nullptr, nullptr, nullptr};
    char* dev[3] = {nullptr, nullptr, nullptr};
    size_t bytes[3] = {0, 0, 0};
    int axes = 0;
    bool own = false;
    explicit BatchFaces(mgp_batch* bb) : b(bb) {}
    ~BatchFaces()
    {
        if (own)
            for (char* p : dev)
                if (p) (void)hipFree(p);
    }
    int open(void* vx, void* vy, void* vz, int mem, int nm, bool upload, const char* what)
    {
        const Geo& g = b->lev[0].g;
        const size_t nx = (size_t)g.nx, ny = (size_t)g.ny, nz = (size_t)g.nz, per = (size_t)nm * b->rb;
        axes = b->dim;
        bytes[0] = (nx + 1) * ny * nz * per;
        bytes[1] = nx * (ny + 1) * nz * per;
        bytes[2] = axes == 3 ? nx * ny * (nz + 1) * per : 0;
        host[0] = vx, host[1] = vy, host[2] = axes == 3 ? vz : nullptr;
        if (mem == MGP_MEM_DEVICE) {
            for (int a = 0; a < axes; ++a) dev[a] = (char*)host[a];
            return MGP_OK;
        }
        own = true;
        for (int a = 0; a < axes; ++a)
            if (hipMalloc((void**)&dev[a], bytes[a]) != hipSuccess) {
                dev[a] = nullptr;
                (void)hipGetLastError();
                return b->fail(MGP_ERR_OOM, "%s: no room for the device copies of the face arrays", what);
            }
        if (upload)
            for (int a = 0; a < axes; ++a) BHIP(b, hipMemcpyAsync(dev[a], host[a], bytes[a], hipMemcpyHostToDevice, b->s));
        return MGP_OK;
    }
    int download()
    {
        if (!own) return MGP_OK;
        for (int a = 0; a < axes; ++a) BHIP(b, hipMemcpyAsync(host[a], dev[a], bytes[a], hipMemcpyDeviceToHost, b->s));
        return MGP_OK;
    }
};

int face_args(const mgp_batch* b, const char* what, int member, const void* vx, const void* vy, const void* vz, int mem)
{
    if (!vx || !vy || (b->dim == 3 && !vz))
        return b->fail(MGP_ERR_ARG, "%s: NULL face array (vx, vy%s)", what, b->dim == 3 ? ", vz" : "; vz is ignored in 2D");
    if (mem != MGP_MEM_HOST && mem != MGP_MEM_DEVICE) return b->fail(MGP_ERR_ARG, "%s: unknown mem %d", what, mem);
    if (member < -1 || member >= b->B)
        return b->fail(MGP_ERR_ARG, "%s: member %d out of range (batch %d)", what, member, b->B);
    return MGP_OK;
}

// level 0's packed field `base` from member m0 on
char* member_base(const mgp_batch* b, char* base, int m0) { return base + (size_t)m0 * b->lev[0].slots * b->rb; }

// f of members [m0, m0 + nm) = D v
int divergence_enqueue(mgp_batch* b, const BatchFaces& v, int m0, int nm)
{
    const BHostLevel& L = b->lev[0];
    BHIP(b, mgp::launch_divergence_batch(b->rb, b->dim, v.dev[0], v.dev[1], v.dev[2], member_base(b, L.f, m0), L.g, nm, b->s));
    return MGP_OK;
}

// faces = G psi or faces -= G psi of members [m0, m0 + nm)
int gradient_enqueue(mgp_batch* b, int op, const BatchFaces& v, int m0, int nm)
{
    const BHostLevel& L = b->lev[0];
    BHIP(b, mgp::launch_gradient_batch(b->rb, b->dim, op == MGP_GRAD_SUBTRACT, member_base(b, L.u, m0), v.dev[0], v.dev[1],
                                       v.dev[2], L.g, L.cl, nm, b->s));
    return MGP_OK;
}

}  // namespace

extern "C" {

int mgp_batch_plan(const mgp_opts* o, int32_t batch, int64_t* rows, int max_levels)
{
    std::vector<int64_t> r;
    int nlev = 0;
    const int rc = batch_validate(o, batch, r, nlev, g_batch_error);
    if (rc != MGP_OK) return rc;
    mgp_batch b;
    host_plan(&b, *o, batch, r, nlev);
    for (int l = 0; l < nlev && l < max_levels && rows; ++l) {
        int64_t* d = rows + 8 * l;
        const BHostLevel& L = b.lev[l];
        d[0] = L.g.nx;
        d[1] = L.g.ny;
        d[2] = L.g.nz;
        d[3] = L.g.nz;
        d[4] = 0;
        d[5] = 0;
        d[6] = b.T >= 0 && l >= b.T ? 1 : 0;
        d[7] = 0;
    }
    return nlev;
}

int mgp_batch_create(mgp_batch** out, const mgp_opts* o, int32_t batch)
{
    if (!out) {
        g_batch_error = "mgp_batch_create: null argument";
        return MGP_ERR_ARG;
    }
    *out = nullptr;
    std::vector<int64_t> rows;
    int nlev = 0;
    const int rc = batch_validate(o, batch, rows, nlev, g_batch_error);
    if (rc != MGP_OK) return rc;
    mgp_batch* b = new mgp_batch();
    host_plan(b, *o, batch, rows, nlev);
    auto bail = [&](int code) {
        g_batch_error = b->err;
        batch_free(b);
        return code;
    };
    int ndev = 0;
    hipError_t he = hipGetDeviceCount(&ndev);
    if (he != hipSuccess || ndev == 0) {
        b->err = std::string("no HIP device available: ") + hipGetErrorString(he);
        return bail(MGP_ERR_HIP);
    }
    if (o->device >= 0) {
        if (o->device >= ndev) {
            b->err = "device ordinal out of range";
            return bail(MGP_ERR_ARG);
        }
        he = hipSetDevice(o->device);
        if (he != hipSuccess) {
            b->err = std::string("hipSetDevice: ") + hipGetErrorString(he);
            return bail(MGP_ERR_HIP);
        }
    }
    he = hipStreamCreateWithFlags(&b->s, hipStreamNonBlocking);
    if (he != hipSuccess) {
        b->err = std::string("hipStreamCreate: ") + hipGetErrorString(he);
        return bail(MGP_ERR_HIP);
    }
    bool oom = false;
    auto alloc0 = [&](void** p, size_t bytes) {
        if (oom) return;
        if (hipMalloc(p, bytes) != hipSuccess) {
            *p = nullptr;
            oom = true;
            return;
        }
        if (hipMemsetAsync(*p, 0, bytes, b->s) != hipSuccess) oom = true;
    };
    const size_t B = (size_t)batch;
    for (int l = 0; l < nlev; ++l) {
        BHostLevel& L = b->lev[l];
        const size_t bytes = B * (size_t)L.slots * b->rb;
        alloc0((void**)&L.u, bytes);
        alloc0((void**)&L.f, bytes);
        if (o->smoother == MGP_JACOBI && (b->T < 0 || l < b->T)) alloc0((void**)&L.t, bytes);
    }
    if (o->err_mode) alloc0((void**)&b->old, B * (size_t)b->lev[0].slots * b->rb);
    alloc0((void**)&b->st.active, B * sizeof(int));
    alloc0((void**)&b->st.iters, B * sizeof(int));
    alloc0((void**)&b->st.last_err, B * sizeof(double));
    alloc0((void**)&b->st.ctr, 2 * sizeof(int));
    alloc0((void**)&b->st.eps, sizeof(double));
    alloc0((void**)&b->st.errs, (size_t)b->chunk * B * sizeof(double));
    alloc0((void**)&b->d_part, 2 * B * (size_t)b->nbe * sizeof(double));
    alloc0((void**)&b->d_norm, 2 * B * sizeof(double));
    if (oom) {
        b->err = "hipMalloc failed for a batch of " + std::to_string(batch) + " members";
        (void)hipGetLastError();
        return bail(MGP_ERR_OOM);
    }
    he = hipHostMalloc((void**)&b->h_nactive, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent);
    if (he == hipSuccess) he = hipHostGetDevicePointer((void**)&b->st.nactive, b->h_nactive, 0);
    if (he != hipSuccess) {
        b->err = std::string("hipHostMalloc (mapped): ") + hipGetErrorString(he);
        return bail(MGP_ERR_HIP);
    }
    *b->h_nactive = batch;
    if (b->T >= 0) {
        const int rt = dispatch(b, [&](auto t, auto d) { return upload_tail<decltype(t), decltype(d)::value>(b); });
        if (rt != MGP_OK) return bail(rt);
    }
    {
        const char* v = std::getenv("MGP_GRAPH");
        b->use_graph = !(v && std::atoi(v) == 0);
    }
    if (arm(b, 0, 0.0) != MGP_OK) return bail(MGP_ERR_HIP);
    he = hipStreamSynchronize(b->s);
    if (he != hipSuccess) {
        b->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(he);
        return bail(MGP_ERR_HIP);
    }
    *out = b;
    return MGP_OK;
}

void mgp_batch_destroy(mgp_batch* b)
{
    if (b && b->s) (void)hipStreamSynchronize(b->s);
    batch_free(b);
}

const char* mgp_batch_last_error(const mgp_batch* b) { return b ? b->err.c_str() : g_batch_error.c_str(); }

int mgp_batch_size(const mgp_batch* b) { return b ? b->B : MGP_ERR_ARG; }

int mgp_batch_init_point_charge(mgp_batch* b)
{
    if (!b) return MGP_ERR_ARG;
    const BHostLevel& L = b->lev[0];
    const size_t bytes = (size_t)b->B * L.slots * b->rb;
    BHIP(b, hipMemsetAsync(L.u, 0, bytes, b->s));
    BHIP(b, hipMemsetAsync(L.f, 0, bytes, b->s));
    const unsigned grid = (unsigned)((b->B + kBlock - 1) / kBlock);
    const int64_t ck = b->dim == 3 ? L.g.nz / 2 : 0;
    if (b->rb == 4)
        mgp::k_batch_point_charge<float><<<dim3(grid), dim3(kBlock), 0, b->s>>>((float*)L.u, (float*)L.f, L.g, L.slots, b->B,
                                                                              L.g.nx / 2, L.g.ny / 2, ck);
    else
        mgp::k_batch_point_charge<double><<<dim3(grid), dim3(kBlock), 0, b->s>>>((double*)L.u, (double*)L.f, L.g, L.slots, b->B,
                                                                               L.g.nx / 2, L.g.ny / 2, ck);
    BHIP(b, hipGetLastError());
    BHIP(b, hipStreamSynchronize(b->s));
    return MGP_OK;
}

int mgp_batch_set_field(mgp_batch* b, int member, int level, int which, const void* src, int64_t count, int mem)
{
    return field_io(b, member, level, which, const_cast<void*>(src), count, mem, true);
}

int mgp_batch_get_field(const mgp_batch* b, int member, int level, int which, void* dst, int64_t count, int mem)
{
    return field_io(const_cast<mgp_batch*>(b), member, level, which, dst, count, mem, false);
}

int mgp_batch_cycles(mgp_batch* b, int32_t k, double* errs)
{
    if (!b) return MGP_ERR_ARG;
    if (k < 0) return b->fail(MGP_ERR_ARG, "k must be >= 0");
    BTRY(arm(b, 0, 0.0));
    return cycles_armed(b, k, errs);
}

int mgp_batch_solve(mgp_batch* b, double epsilon, int32_t maxiter, int32_t* iters, double* last_err)
{
    if (!b) return MGP_ERR_ARG;
    if (!b->o.err_mode) return b->fail(MGP_ERR_STATE, "mgp_batch_solve needs err_mode 1 (the stop rule reads the err)");
    if (maxiter < 0) return b->fail(MGP_ERR_ARG, "maxiter must be >= 0");
    constexpr int kSolveChunk = 4;  // cycles enqueued between two looks at the number of active members
    BTRY(arm(b, 1, epsilon));
    if (maxiter > 0) b->old_stale = false;
    for (int done = 0; done < maxiter;) {
        const int n = (int)std::min<int64_t>(std::min<int64_t>(kSolveChunk, b->chunk), maxiter - done);
        BHIP(b, hipMemsetAsync(b->st.ctr, 0, sizeof(int), b->s));
        BTRY(enqueue_cycles(b, n));
        BHIP(b, hipStreamSynchronize(b->s));
        done += n;
        if (*(volatile int*)b->h_nactive == 0) break;
    }
    if (iters) BHIP(b, hipMemcpyAsync(iters, b->st.iters, sizeof(int32_t) * b->B, hipMemcpyDeviceToHost, b->s));
    if (last_err) BHIP(b, hipMemcpyAsync(last_err, b->st.last_err, sizeof(double) * b->B, hipMemcpyDeviceToHost, b->s));
    BHIP(b, hipStreamSynchronize(b->s));
    return MGP_OK;
}

int mgp_batch_residual_norm(mgp_batch* b, double* rnorm, double* fnorm)
{
    if (!b) return MGP_ERR_ARG;
    BTRY(resnorm_enqueue(b));
    std::vector<double> h(2 * (size_t)b->B);
    BHIP(b, hipMemcpyAsync(h.data(), b->d_norm, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b->s));
    BHIP(b, hipStreamSynchronize(b->s));
    for (int m = 0; m < b->B; ++m) {
        if (rnorm) rnorm[m] = std::sqrt(h[m]);
        if (fnorm) fnorm[m] = std::sqrt(h[b->B + m]);
    }
    return MGP_OK;
}

int mgp_batch_remove_mean(mgp_batch* b, int level, int which, double* means)
{
    if (!b) return MGP_ERR_ARG;
    if (level < 0 || level >= (int)b->lev.size()) return b->fail(MGP_ERR_ARG, "level %d out of range", level);
    if (which != MGP_FIELD_U && which != MGP_FIELD_F)
        return b->fail(MGP_ERR_ARG, "mgp_batch_remove_mean: which must be MGP_FIELD_U or MGP_FIELD_F");
    const BHostLevel& L = b->lev[level];
    BTRY(mean_enqueue(b, L, which == MGP_FIELD_U ? L.u : L.f));
    std::vector<double> h((size_t)b->B);
    BHIP(b, hipMemcpyAsync(h.data(), b->d_norm + b->B, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b->s));
    BHIP(b, hipStreamSynchronize(b->s));
    if (means) std::copy(h.begin(), h.end(), means);
    return MGP_OK;
}

int mgp_batch_fmg_restrict_rhs(mgp_batch* b, int level)
{
    if (!b) return MGP_ERR_ARG;
    if (level < 0 || level + 1 >= (int)b->lev.size()) return b->fail(MGP_ERR_ARG, "mgp_batch_fmg_restrict_rhs: bad level %d", level);
    BTRY(dispatch(b, [&](auto t, auto d) {
        Cycle<decltype(t), decltype(d)::value> c{b};
        return c.fmg_restrict(level, nullptr);
    }));
    BHIP(b, hipStreamSynchronize(b->s));
    return MGP_OK;
}

int mgp_batch_fmg_prolong(mgp_batch* b, int level)
{
    if (!b) return MGP_ERR_ARG;
    if (level < 0 || level + 1 >= (int)b->lev.size()) return b->fail(MGP_ERR_ARG, "mgp_batch_fmg_prolong: bad level %d", level);
    BTRY(dispatch(b, [&](auto t, auto d) {
        Cycle<decltype(t), decltype(d)::value> c{b};
        return c.fmg_p3(level, nullptr);
    }));
    if (level == 0) b->old_stale = true;  // psiOld describes an iterate that is gone
    BHIP(b, hipStreamSynchronize(b->s));
    return MGP_OK;
}

int mgp_batch_fmg(mgp_batch* b, int32_t cycles_per_level, int32_t final_cycles, double* errs)
{
    if (!b) return MGP_ERR_ARG;
    if (cycles_per_level < 1 || final_cycles < 0)
        return b->fail(MGP_ERR_ARG, "mgp_batch_fmg: cycles_per_level >= 1 and final_cycles >= 0");
    BTRY(arm(b, 0, 0.0));
    b->old_stale = true;  // (before the first launch: an ascent that fails part-way has replaced psi already)
    BTRY(enqueue_ascent(b, cycles_per_level));
    return cycles_armed(b, final_cycles, errs);
}

int mgp_batch_fmg_launches(const mgp_batch* b, int64_t* ascent)
{
    if (!b || !ascent) return MGP_ERR_ARG;
    *ascent = b->fmg_launches;
    return MGP_OK;
}

int mgp_batch_divergence(mgp_batch* b, int member, const void* vx, const void* vy, const void* vz, int mem)
{
    if (!b) return MGP_ERR_ARG;
    BTRY(face_args(b, "mgp_batch_divergence", member, vx, vy, vz, mem));
    const int m0 = member < 0 ? 0 : member, nm = member < 0 ? b->B : 1;
    BatchFaces v(b);
    BTRY(v.open(const_cast<void*>(vx), const_cast<void*>(vy), const_cast<void*>(vz), mem, nm, true, "mgp_batch_divergence"));
    BTRY(divergence_enqueue(b, v, m0, nm));
    BHIP(b, hipStreamSynchronize(b->s));
    return MGP_OK;
}

int mgp_batch_gradient(mgp_batch* b, int member, int op, void* vx, void* vy, void* vz, int mem)
{
    if (!b) return MGP_ERR_ARG;
    if (op != MGP_GRAD_STORE && op != MGP_GRAD_SUBTRACT) return b->fail(MGP_ERR_ARG, "mgp_batch_gradient: unknown op %d", op);
    BTRY(face_args(b, "mgp_batch_gradient", member, vx, vy, vz, mem));
    const int m0 = member < 0 ? 0 : member, nm = member < 0 ? b->B : 1;
    BatchFaces v(b);
    BTRY(v.open(vx, vy, vz, mem, nm, op == MGP_GRAD_SUBTRACT, "mgp_batch_gradient"));
    BTRY(gradient_enqueue(b, op, v, m0, nm));
    BTRY(v.download());
    BHIP(b, hipStreamSynchronize(b->s));
    return MGP_OK;
}

int mgp_batch_project(mgp_batch* b, void* vx, void* vy, void* vz, int mem, int32_t fmg_cycles, int32_t cycles,
                      double* div_before, double* div_after)
{
    if (!b) return MGP_ERR_ARG;
    if (fmg_cycles < 0 || cycles < 0) return b->fail(MGP_ERR_ARG, "mgp_batch_project: fmg_cycles >= 0 and cycles >= 0");
    BTRY(face_args(b, "mgp_batch_project", -1, vx, vy, vz, mem));
    BatchFaces v(b);
    BTRY(v.open(vx, vy, vz, mem, b->B, true, "mgp_batch_project"));
    const BHostLevel& L = b->lev[0];
    BTRY(divergence_enqueue(b, v, 0, b->B));
    if (b->o.coarse_bc == MGP_BC_NEUMANN) BTRY(mean_enqueue(b, L, L.f));  // mgp_batch_remove_mean(0, F) without its read-back
    BTRY(arm(b, 0, 0.0));
    if (fmg_cycles >= 1) {  // mgp_batch_fmg's path
        b->old_stale = true;
        BTRY(enqueue_ascent(b, fmg_cycles));
    }
    BTRY(cycles_armed(b, cycles, nullptr, false));
    BTRY(gradient_enqueue(b, MGP_GRAD_SUBTRACT, v, 0, b->B));
    BTRY(v.download());
    std::vector<double> h;
    if (div_before || div_after) {
        BTRY(resnorm_enqueue(b));
        h.resize(2 * (size_t)b->B);
        BHIP(b, hipMemcpyAsync(h.data(), b->d_norm, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b->s));
    }
    BHIP(b, hipStreamSynchronize(b->s));
    for (int m = 0; m < b->B && !h.empty(); ++m) {
        if (div_before) div_before[m] = std::sqrt(h[b->B + m]);
        if (div_after) div_after[m] = std::sqrt(h[m]);
    }
    return MGP_OK;
}

int mgp_batch_launches(const mgp_batch* b, int64_t* per_cycle)
{
    if (!b || !per_cycle) return MGP_ERR_ARG;
    *per_cycle = b->last_launches;
    return MGP_OK;
}

}  // extern "C"
