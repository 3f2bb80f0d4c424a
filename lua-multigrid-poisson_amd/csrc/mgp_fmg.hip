// mgp_fmg.hip — the two device passes of the full multigrid start (mgp_fmg, mgp_fmg_restrict_rhs, mgp_fmg_prolong):
//
//  k_restrict_field   f of level l + 1 = the 2^d average of f of level l, in reduceResidual's term order
//                     R = 1/8 (((((((f000 + f100) + f010) + f110) + f001) + f101) + f011) + f111)   (x fastest; 2D: the
//                     first four terms, times 1/4).  The full weighting of a stored field is launch_fw_restrict.
//  k_fmg_prolong      u of level l = P3 (u of level l + 1): every fine cell is REPLACED by the separable cubic
//                     interpolation of the coarse level, one pass per active axis in the order x, y, z, each pass on
//                     the result of the pass before.
//
// P3 along one axis.  The coarse line A[0 .. m) is extended by two ghosts per side, mc = -(T)c_{l+1}:
//     E[-1] = mc E[0], E[-2] = mc E[1], E[m] = mc E[m-1], E[m+1] = mc E[m-2]
//     (m = 1: E[-1] = E[1] = mc A[0], E[-2] = E[2] = mc (mc A[0]));
// each ghost is one multiplication, always performed (mc = -0 included).  The ghost lines of the y and z passes are mc
// times the already x- (x, y-) interpolated in-box line.  The children of coarse cell I:
//     child 2I     = ((wp E[I] + wn E[I-1]) + wq E[I+1]) + wr E[I-2]
//     child 2I + 1 = ((wp E[I] + wn E[I+1]) + wq E[I-1]) + wr E[I+2]
// wp = 105/128, wn = 35/128, wq = -7/128, wr = -5/128 (the cubic Lagrange weights at -+1/4 of a coarse cell; exact in
// binary).  Every operation is rounded in the real type T (no contraction: -ffp-contract=off).
//
// Layout.  Vector form (coarse nx >= 16 bytes of reals): a thread owns the fine cells above N consecutive coarse cells
// of a column of coarse rows: in 3D (J, K0 .. K0 + zc - 1), in 2D (J0 .. J0 + yc - 1).  It marches along the column
// with the five x, y-interpolated coarse planes K - 2 .. K + 2 (2D: the five x-interpolated rows) in registers: every
// step x-interpolates the five coarse rows J - 2 .. J + 2 of ONE new coarse plane, y-interpolates them into the two
// fine rows, and stores the 2 x 2 fine rows (j pair, k pair) above coarse row (J, K), N cells of each colour in each:
// one 16-byte store per fine row and colour half.  A ghost plane (row) is the in-box one it mirrors, interpolated and
// scaled.  The march length is chosen on the host so that the level still fills the machine (march_len; 1 = a thread
// per coarse row) and does not change a bit of the result.  Coarse reads come through L1 / L2 (the coarse level is
// 1/8 of the fine one); no LDS.  Scalar form: a thread per fine slot (any sizes: coarse nx below the vector width,
// one- and two-cell coarse axes).  Both evaluate exactly the expressions above.
//
// A batch (mgp_batch.hip) runs the vector form on all its members in one launch: k_fmg_prolong_b / k_fmg_prolong_2d_b are
// the same march (fmg_march / fmg_march_2d) with a member stride for u and V and a number of workgroups per member;
// the small helpers of P3 (W3, cub, ext_src, ext_scale) are in mgp_fmg_dev.h for both translation units.
//
// One rank's whole box only (g.z0 = 0, every plane local): the cubic stencil needs a second coarse ghost plane that a
// slab level does not carry.
#include "mgp_fmg_dev.h"

namespace mgp {
namespace {

// ---- scalar form: a thread per fine slot ------------------------------------------------------------------

template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_fmg_prolong_s(T* __restrict__ u, const T* __restrict__ V, Geo g, Geo gc,
                                                          T mc)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= g.P * g.nz) return;
    int i, j;
    int64_t k;
    if (!slot_cell(s, g, i, j, k)) return;
    const int I = i >> 1, J = j >> 1, K = DIM == 3 ? (int)(k >> 1) : 0;
    const int sx = (i & 1) ? 1 : -1, sy = (j & 1) ? 1 : -1, sz = (k & 1) ? 1 : -1;
    const int mz = DIM == 3 ? (int)gc.nz : 1;
    T zt[4];
#pragma unroll
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
                xt[tx] = ext_scale(V[pidx(gc, Iq, Jq, Kq)], nx_, mc);
            }
            yt[ty] = ext_scale(cub(xt[0], xt[1], xt[2], xt[3]), ny_, mc);
        }
        zt[tz] = ext_scale(cub(yt[0], yt[1], yt[2], yt[3]), nz_, mc);
    }
    u[s] = DIM == 3 ? cub(zt[0], zt[1], zt[2], zt[3]) : zt[0];
}

// ---- vector form -------------------------------------------------------------------------------------------

// The x pass of coarse row (Jr, Kr), both in the box, above coarse cells I0 .. I0 + N - 1: xe[e] / xo[e] = the even /
// odd child of coarse cell I0 + e.  Samples I0 - 2 .. I0 + N + 1: N / 2 + 2 from each colour half.
template <typename T, int N>
__device__ __forceinline__ void x_pass(const T* __restrict__ V, const Geo& gc, int Jr, int Kr, int I0, T mc,
                                       T (&xe)[N], T (&xo)[N])
{
    const int pc = (Jr + Kr) & 1;  // colour of even x in this row
    const int64_t row = (int64_t)Kr * gc.P + (int64_t)Jr * gc.hw;
    const T* hp = V + row + pc * gc.H;        // I0 - 2, I0, ..., I0 + N
    const T* hq = V + row + (pc ^ 1) * gc.H;  // I0 - 1, I0 + 1, ..., I0 + N + 1
    const int cm = I0 >> 1;
    const bool lo = I0 == 0, hi = I0 + N == gc.nx;
    T c[N + 4];  // c[e] = E[I0 - 2 + e]
#pragma unroll
    for (int e = 0; e < N; ++e) c[e + 2] = ((e & 1) ? hq : hp)[cm + (e >> 1)];
    if (lo) {
        c[1] = mc * c[2];
        c[0] = mc * c[3];
    } else {
        c[0] = hp[cm - 1];
        c[1] = hq[cm - 1];
    }
    if (hi) {
        c[N + 2] = mc * c[N + 1];
        c[N + 3] = mc * c[N];
    } else {
        c[N + 2] = hp[cm + N / 2];
        c[N + 3] = hq[cm + N / 2];
    }
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int p = e + 2;
        xe[e] = cub(c[p], c[p - 1], c[p + 1], c[p - 2]);
        xo[e] = cub(c[p], c[p + 1], c[p - 1], c[p + 2]);
    }
}

// The x and y passes of coarse plane Kr (in the box) above coarse cells I0 .. of coarse row J: y[dy][o][e] = fine row
// 2J + dy, x parity o, above coarse cell I0 + e
template <typename T, int N>
__device__ __forceinline__ void xy_pass(const T* __restrict__ V, const Geo& gc, int J, int Kr, int I0, T mc,
                                        T (&y)[2][2][N])
{
    T x[5][2][N];  // rows J - 2 .. J + 2
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        int nm;
        const int Jr = ext_src(J - 2 + r, gc.ny, nm);
        x_pass<T, N>(V, gc, Jr, Kr, I0, mc, x[r][0], x[r][1]);
        if (nm) {
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int e = 0; e < N; ++e) x[r][o][e] = ext_scale(x[r][o][e], nm, mc);
        }
    }
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int e = 0; e < N; ++e) {
            y[0][o][e] = cub(x[2][o][e], x[1][o][e], x[3][o][e], x[0][o][e]);
            y[1][o][e] = cub(x[2][o][e], x[3][o][e], x[1][o][e], x[4][o][e]);
        }
}

// the fine row (j, k) above coarse cells I0 ..: N cells of each colour, one 16-byte store each
template <typename T, int N>
__device__ __forceinline__ void store_row(T* __restrict__ u, const Geo& g, int j, int64_t k, int I0, const T (&v)[2][N])
{
    const int p = (int)((j + k) & 1);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        Vec<T, N> out;
#pragma unroll
        for (int e = 0; e < N; ++e) out.v[e] = v[c ^ p][e];
        vstore<T, N>(u + k * g.P + c * g.H + (int64_t)j * g.hw + I0, out);
    }
}

// One coarse plane's x and y passes, as the z pass sees it: plane q of the extended column (q in [-2, mz + 1])
template <typename T, int N>
__device__ __forceinline__ void z_sample(const T* __restrict__ V, const Geo& gc, int J, int q, int mz, int I0, T mc,
                                         T (&w)[2][2][N])
{
    int nm;
    const int Kr = ext_src(q, mz, nm);
    xy_pass<T, N>(V, gc, J, Kr, I0, mc, w);
    if (nm) {
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int e = 0; e < N; ++e) w[dy][o][e] = ext_scale(w[dy][o][e], nm, mc);
    }
}

// 3D: the thread marches through `zc` coarse planes of its column (J, I0 ..) with the x, y-interpolated planes
// K - 2 .. K + 2 in registers: every step computes one new plane (a ghost plane from the in-box plane it mirrors) and
// stores the 2 x 2 fine rows above coarse row (J, K).  zc = 1 is a thread per coarse row.
// (lb: the workgroup's index within its box; < 0: the grid is one box, XCD-remapped)
template <typename T>
__device__ __forceinline__ void fmg_march(T* __restrict__ u, const T* __restrict__ V, Geo g, Geo gc, T mc, int zc, int lb)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int lgpr = gc.lx - LN;  // log2 groups of N per coarse row
    const int b = lb < 0 ? xcd_remap(blockIdx.x, gridDim.x) : lb;
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    const int grp = (int)(it & ((1 << lgpr) - 1));
    const int J = (int)((it >> lgpr) & (gc.ny - 1));
    const int64_t chunk = it >> (lgpr + gc.ly);
    const int mz = (int)gc.nz;
    if (chunk * zc >= mz) return;
    const int K0 = (int)chunk * zc;
    const int I0 = grp * N;
    T w[5][2][2][N];  // planes K - 2 .. K + 2
#pragma unroll
    for (int t = 1; t < 5; ++t) z_sample<T, N>(V, gc, J, K0 - 3 + t, mz, I0, mc, w[t]);
    for (int K = K0; K < K0 + zc; ++K) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int o = 0; o < 2; ++o)
#pragma unroll
                    for (int e = 0; e < N; ++e) w[t][dy][o][e] = w[t + 1][dy][o][e];
        z_sample<T, N>(V, gc, J, K + 2, mz, I0, mc, w[4]);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            T ze[2][N], zo[2][N];
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    ze[o][e] = cub(w[2][dy][o][e], w[1][dy][o][e], w[3][dy][o][e], w[0][dy][o][e]);
                    zo[o][e] = cub(w[2][dy][o][e], w[3][dy][o][e], w[1][dy][o][e], w[4][dy][o][e]);
                }
            store_row<T, N>(u, g, 2 * J + dy, 2 * (int64_t)K, I0, ze);
            store_row<T, N>(u, g, 2 * J + dy, 2 * (int64_t)K + 1, I0, zo);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_fmg_prolong(T* __restrict__ u, const T* __restrict__ V, Geo g, Geo gc, T mc,
                                                        int zc)
{
    fmg_march<T>(u, V, g, gc, mc, zc, -1);
}

// The same march on every member of a batch (mgp_batch.hip): workgroups [m * nb, (m + 1) * nb) work on member m, whose
// u / V start us / vs reals after member m - 1's; active == nullptr: every member
template <typename T>
__global__ __launch_bounds__(kBlock) void k_fmg_prolong_b(T* __restrict__ u, const T* __restrict__ V, Geo g, Geo gc,
                                                          T mc, int zc, int64_t us, int64_t vs, int nb,
                                                          const int* __restrict__ active)
{
    const int m = (int)(blockIdx.x / (unsigned)nb);
    if (active && !active[m]) return;
    fmg_march<T>(u + m * us, V + m * vs, g, gc, mc, zc, (int)(blockIdx.x - (unsigned)m * nb));
}

// 2D: the same march through `yc` coarse rows with the x-interpolated rows J - 2 .. J + 2 in registers
template <typename T>
__device__ __forceinline__ void fmg_march_2d(T* __restrict__ u, const T* __restrict__ V, Geo g, Geo gc, T mc, int yc,
                                             int lb)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int lgpr = gc.lx - LN;
    const int b = lb < 0 ? xcd_remap(blockIdx.x, gridDim.x) : lb;
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    const int grp = (int)(it & ((1 << lgpr) - 1));
    const int64_t chunk = it >> lgpr;
    if (chunk * yc >= gc.ny) return;
    const int J0 = (int)chunk * yc;
    const int I0 = grp * N;
    T x[5][2][N];  // rows J - 2 .. J + 2
    auto sample = [&](int q, T (&r)[2][N]) {
        int nm;
        const int Jr = ext_src(q, gc.ny, nm);
        x_pass<T, N>(V, gc, Jr, 0, I0, mc, r[0], r[1]);
        if (nm) {
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int e = 0; e < N; ++e) r[o][e] = ext_scale(r[o][e], nm, mc);
        }
    };
#pragma unroll
    for (int t = 1; t < 5; ++t) sample(J0 - 3 + t, x[t]);
    for (int J = J0; J < J0 + yc; ++J) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int e = 0; e < N; ++e) x[t][o][e] = x[t + 1][o][e];
        sample(J + 2, x[4]);
        T ye[2][N], yo[2][N];
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int e = 0; e < N; ++e) {
                ye[o][e] = cub(x[2][o][e], x[1][o][e], x[3][o][e], x[0][o][e]);
                yo[o][e] = cub(x[2][o][e], x[3][o][e], x[1][o][e], x[4][o][e]);
            }
        store_row<T, N>(u, g, 2 * J, 0, I0, ye);
        store_row<T, N>(u, g, 2 * J + 1, 0, I0, yo);
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_fmg_prolong_2d(T* __restrict__ u, const T* __restrict__ V, Geo g, Geo gc,
                                                           T mc, int yc)
{
    fmg_march_2d<T>(u, V, g, gc, mc, yc, -1);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_fmg_prolong_2d_b(T* __restrict__ u, const T* __restrict__ V, Geo g, Geo gc,
                                                             T mc, int yc, int64_t us, int64_t vs, int nb,
                                                             const int* __restrict__ active)
{
    const int m = (int)(blockIdx.x / (unsigned)nb);
    if (active && !active[m]) return;
    fmg_march_2d<T>(u + m * us, V + m * vs, g, gc, mc, yc, (int)(blockIdx.x - (unsigned)m * nb));
}

// ---- the 2^d average of a field ------------------------------------------------------------------------------

// Scalar form: a thread per coarse cell (any sizes)
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_restrict_field_s(const T* __restrict__ f, T* __restrict__ R, Geo g, Geo gc)
{
    const int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int cx = g.nx >> 1, cy = g.ny >> 1;
    const int64_t ncz = DIM == 3 ? (g.nz >> 1) : 1;
    if (it >= (int64_t)cx * cy * ncz) return;
    const int I = (int)(it & (cx - 1));
    const int J = (int)((it >> (g.lx - 1)) & (cy - 1));
    const int64_t K = it >> (g.lx - 1 + g.ly - 1);
    const int i = 2 * I, j = 2 * J;
    const int64_t k = DIM == 3 ? 2 * K : 0;
    T s = f[pidx(g, i, j, k)] + f[pidx(g, i + 1, j, k)];
    s = s + f[pidx(g, i, j + 1, k)];
    s = s + f[pidx(g, i + 1, j + 1, k)];
    if (DIM == 3) {
        s = s + f[pidx(g, i, j, k + 1)];
        s = s + f[pidx(g, i + 1, j, k + 1)];
        s = s + f[pidx(g, i, j + 1, k + 1)];
        s = s + f[pidx(g, i + 1, j + 1, k + 1)];
    }
    R[pidx(gc, I, J, K)] = (DIM == 3 ? (T)0.125 : (T)0.25) * s;
}

// Vector form (coarse nx >= N): a thread owns N consecutive coarse cells of one coarse row; their children are, in
// each of the 2 (4) fine rows, the N cells m = I0 .. of both colours: one 16-byte load each.
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_restrict_field(const T* __restrict__ f, T* __restrict__ R, Geo g, Geo gc)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int cy = g.ny >> 1;
    const int lgpr = (g.lx - 1) - LN;
    const int64_t ncz = DIM == 3 ? (g.nz >> 1) : 1;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    const int grp = (int)(it & ((1 << lgpr) - 1));
    const int J = (int)((it >> lgpr) & (cy - 1));
    const int64_t K = it >> (lgpr + g.ly - 1);
    if (K >= ncz) return;
    const int I0 = grp * N;
    T acc[N];
#pragma unroll
    for (int dz = 0; dz < (DIM == 3 ? 2 : 1); ++dz) {
        const int64_t k = DIM == 3 ? 2 * K + dz : 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int j = 2 * J + dy;
            const int p = (int)((j + k) & 1);  // colour of the row's even x
            const T* row = f + k * g.P + (int64_t)j * g.hw + I0;
            const Vec<T, N> ev = vload<T, N>(row + p * g.H);
            const Vec<T, N> od = vload<T, N>(row + (p ^ 1) * g.H);
#pragma unroll
            for (int e = 0; e < N; ++e) {
                if (dz == 0 && dy == 0) {
                    acc[e] = ev.v[e] + od.v[e];
                } else {
                    acc[e] = acc[e] + ev.v[e];
                    acc[e] = acc[e] + od.v[e];
                }
            }
        }
    }
    // coarse cells I0 + e: colour (I0 + e + J + K) & 1, packed position (I0 + e) >> 1: N / 2 consecutive per half
    const int pc = (int)((J + K) & 1);
    const int64_t rowc = K * gc.P + (int64_t)J * gc.hw + (I0 >> 1);
    Vec<T, N / 2> he, ho;
#pragma unroll
    for (int e = 0; e < N; ++e) ((e & 1) ? ho : he).v[e >> 1] = (DIM == 3 ? (T)0.125 : (T)0.25) * acc[e];
    vstore<T, N / 2>(R + rowc + pc * gc.H, he);
    vstore<T, N / 2>(R + rowc + (pc ^ 1) * gc.H, ho);
}

// Coarse lines per thread of the marching kernels: as long as a level still fills the machine with threads, at most
// 16 (the four lines a thread computes before its first store are 4 / len of its work)
#ifndef FMG_MARCH_THREADS  // build-time constant (a host-side check of the kernels compiles with a small one)
#define FMG_MARCH_THREADS (1 << 17)
#endif
inline int march_len(int64_t cols, int m)
{
    int c = m < 16 ? m : 16;
    while (c > 1 && cols * (m / c) < (int64_t)FMG_MARCH_THREADS) c >>= 1;
    return c;
}

template <typename T, int D>
hipError_t fmg_prolong_t(void* u, const void* V, Geo g, Geo gc, double clc, hipStream_t s)
{
    constexpr int n = VN<T>::n;
    const T mc = -(T)clc;
    if (gc.nx >= n) {
        const int64_t groups = gc.nx / n;
        if (D == 3) {
            const int zc = march_len(groups * gc.ny, (int)gc.nz);
            k_fmg_prolong<T><<<nblk(groups * gc.ny * (gc.nz / zc)), kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, mc, zc);
        } else {
            const int yc = march_len(groups, gc.ny);
            k_fmg_prolong_2d<T><<<nblk(groups * (gc.ny / yc)), kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, mc, yc);
        }
    } else {
        k_fmg_prolong_s<T, D><<<nblk(g.P * g.nz), kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, mc);
    }
    return hipGetLastError();
}

// The vector form on B members: the march length from B x the member's columns, so that the batch fills the machine
// as one box of its size would
template <typename T, int D>
hipError_t fmg_prolong_batch_t(void* u, const void* V, Geo g, Geo gc, double clc, int B, int64_t us, int64_t vs,
                               const int* active, hipStream_t s)
{
    constexpr int n = VN<T>::n;
    const T mc = -(T)clc;
    const int64_t groups = gc.nx / n;
    if (D == 3) {
        const int zc = march_len((int64_t)B * groups * gc.ny, (int)gc.nz);
        const int nb = (int)nblk(groups * gc.ny * (gc.nz / zc));
        k_fmg_prolong_b<T><<<(unsigned)((int64_t)B * nb), kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, mc, zc, us, vs, nb, active);
    } else {
        const int yc = march_len((int64_t)B * groups, gc.ny);
        const int nb = (int)nblk(groups * (gc.ny / yc));
        k_fmg_prolong_2d_b<T><<<(unsigned)((int64_t)B * nb), kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, mc, yc, us, vs, nb,
                                                                            active);
    }
    return hipGetLastError();
}

template <typename T, int D>
hipError_t restrict_field_t(const void* f, void* R, Geo g, Geo gc, hipStream_t s)
{
    constexpr int n = VN<T>::n;
    const int cx = g.nx / 2;
    const int64_t rows = (int64_t)(g.ny / 2) * (D == 3 ? g.nz / 2 : 1);
    if (cx >= n)
        k_restrict_field<T, D><<<nblk((cx / n) * rows), kBlock, 0, s>>>((const T*)f, (T*)R, g, gc);
    else
        k_restrict_field_s<T, D><<<nblk(cx * rows), kBlock, 0, s>>>((const T*)f, (T*)R, g, gc);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fmg_prolong(int rb, int dim, void* u, const void* V, Geo g, Geo gc, double clc, hipStream_t s)
{
    if ((rb != 4 && rb != 8) || g.z0 != 0 || gc.z0 != 0 || g.nz != g.gnz || gc.nz != gc.gnz || g.nx != 2 * gc.nx ||
        g.ny != 2 * gc.ny || g.nz != (dim == 3 ? 2 : 1) * gc.nz)
        return hipErrorInvalidValue;
    if (rb == 8) return dim == 3 ? fmg_prolong_t<double, 3>(u, V, g, gc, clc, s) : fmg_prolong_t<double, 2>(u, V, g, gc, clc, s);
    return dim == 3 ? fmg_prolong_t<float, 3>(u, V, g, gc, clc, s) : fmg_prolong_t<float, 2>(u, V, g, gc, clc, s);
}

hipError_t launch_fmg_prolong_batch(int rb, int dim, void* u, const void* V, Geo g, Geo gc, double clc, int B, int64_t us,
                                    int64_t vs, const int* active, hipStream_t s)
{
    if ((rb != 4 && rb != 8) || B < 1 || gc.nx * rb < 16 || g.z0 != 0 || gc.z0 != 0 || g.nz != g.gnz || gc.nz != gc.gnz ||
        g.P != 2 * g.H || gc.P != 2 * gc.H || g.nx != 2 * gc.nx || g.ny != 2 * gc.ny || g.nz != (dim == 3 ? 2 : 1) * gc.nz ||
        us < g.P * g.nz || vs < gc.P * gc.nz || (us * rb) % 16 != 0)
        return hipErrorInvalidValue;
    if (rb == 8)
        return dim == 3 ? fmg_prolong_batch_t<double, 3>(u, V, g, gc, clc, B, us, vs, active, s)
                        : fmg_prolong_batch_t<double, 2>(u, V, g, gc, clc, B, us, vs, active, s);
    return dim == 3 ? fmg_prolong_batch_t<float, 3>(u, V, g, gc, clc, B, us, vs, active, s)
                    : fmg_prolong_batch_t<float, 2>(u, V, g, gc, clc, B, us, vs, active, s);
}

hipError_t launch_restrict_field(int rb, int dim, const void* f, void* R, Geo g, Geo gc, hipStream_t s)
{
    if ((rb != 4 && rb != 8) || g.z0 != 0 || gc.z0 != 0 || g.nz != g.gnz || g.nx != 2 * gc.nx || g.ny != 2 * gc.ny ||
        g.nz != (dim == 3 ? 2 : 1) * gc.nz)
        return hipErrorInvalidValue;
    if (rb == 8) return dim == 3 ? restrict_field_t<double, 3>(f, R, g, gc, s) : restrict_field_t<double, 2>(f, R, g, gc, s);
    return dim == 3 ? restrict_field_t<float, 3>(f, R, g, gc, s) : restrict_field_t<float, 2>(f, R, g, gc, s);
}

}  // namespace mgp
