// mgp_vc.hip — the variable-coefficient operator A_beta u = div(beta grad u) with face coefficients beta
// (mgp_set_coefficients; include/mgpoisson.h has the definition).  While a context has coefficients every level of its
// cycle runs one launch per piece on these kernels:
//   k_vc_check                   every raw input value finite and > 0 (one pass, one flag bit per axis)
//   k_vc_pack / k_vc_coarsen     level 0's faces from the caller's lexicographic arrays / a coarse level's faces from
//                                the level above (the mean of the 2^(d-1) fine faces that tile a coarse face)
//   k_vc_unpack                  a level's faces back into the lexicographic layout (mgp_get_coefficients)
//   k_half_vc / k_half_vc_s      one colour's half-sweep, 16-byte vector form / a thread per slot (k_half's and
//                                k_half_s's thread-to-cell mappings and err partials)
//   k_resrestrict_vc(_s)         residual + 2^d average into the coarse f: a thread per coarse cell, or (where
//                                MGP_RR_SCALAR_CELLS is given, from that many coarse cells up) N coarse cells of a row
//   k_residual_vc / k_resnorm_vc r = f - A_beta u at every slot / its fp64 norms (k_resnorm_s's sum scheme)
//   k_grad_vc                    faces = beta G psi (or faces -= beta G psi), a thread per slot
//
// Layout of a level's coefficients: per axis one array in the level's red/black packed layout that holds at each cell's
// slot the coefficient of the cell's LOWER face on that axis.  The upper face of a cell is the lower face of its upper
// neighbour, which has the other colour and sits exactly where the half-sweep reads that neighbour's u: at m + (i & 1)
// of the other half for x, one row up for y, one plane up for z.  So a half-sweep reads beta with the 16-byte accesses
// it uses for u and f, every face once.  The faces on the upper walls have no owning cell: x = nx goes to the side
// array wx[k][j], y = ny to wy[k][i & 1][i >> 1] (a row's cells of one x parity are contiguous, as in a half), and
// z = nz to the packed array's upper ghost plane (the slot of the cell that would lie above).
// Every expression in T, each operation rounded (the unit is built without contraction).
#include "mgp_cell.h"

#include <algorithm>

namespace mgp {
namespace {

template <typename T>
struct VcT {
    T* bx;
    T* by;
    T* bz;
    T* wx;
    T* wy;
};

template <typename T>
VcT<T> vc_view(const VcCoef& v)
{
    return {(T*)v.b[0], (T*)v.b[1], (T*)v.b[2], (T*)v.wx, (T*)v.wy};
}

// where the face (i, j, k) of `axis` lives (i <= nx on axis 0, j <= ny on axis 1, k <= nz on axis 2)
template <typename T>
__device__ __forceinline__ T* vc_face(const VcT<T>& v, const Geo& g, int axis, int i, int j, int64_t k)
{
    if (axis == 0) return i < g.nx ? v.bx + pidx(g, i, j, k) : v.wx + k * g.ny + j;
    if (axis == 1) return j < g.ny ? v.by + pidx(g, i, j, k) : v.wy + (k * 2 + (i & 1)) * g.hw + (i >> 1);
    return v.bz + pidx(g, i, j, k);
}

// lexicographic face index q of `axis` -> (i, j, k); false past the array's end
__device__ __forceinline__ bool vc_lex(int64_t q, const Geo& g, int dim, int axis, int& i, int& j, int64_t& k)
{
    const int64_t fx = g.nx + (axis == 0), fy = g.ny + (axis == 1), fz = dim == 3 ? g.nz + (axis == 2) : 1;
    if (q >= fx * fy * fz) return false;
    i = (int)(q % fx);
    j = (int)((q / fx) % fy);
    k = q / (fx * fy);
    return true;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_vc_check(const T* __restrict__ p, int64_t n, int* __restrict__ bad, int bit)
{
    bool ok = true;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (int64_t)gridDim.x * kBlock) {
        const T x = p[q];
        ok = ok && x > (T)0 && x < (T)INFINITY;
    }
    if (__any(!ok) && (threadIdx.x & 63) == 0) atomicOr(bad, bit);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_vc_pack(const T* __restrict__ lex, VcT<T> v, Geo g, int dim, int axis)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int i, j;
    int64_t k;
    if (vc_lex(q, g, dim, axis, i, j, k)) *vc_face(v, g, axis, i, j, k) = lex[q];
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_vc_unpack(VcT<T> v, T* __restrict__ lex, Geo g, int dim, int axis)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int i, j;
    int64_t k;
    if (vc_lex(q, g, dim, axis, i, j, k)) lex[q] = *vc_face(v, g, axis, i, j, k);
}

// coarse face (I, J, K) of `axis` = the mean of the fine faces (2I, 2J, 2K) + the tangential offsets, the lower
// tangential axis fastest
template <typename T>
__global__ __launch_bounds__(kBlock) void k_vc_coarsen(VcT<T> vf, Geo g, VcT<T> vc, Geo gc, int dim, int axis)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int I, J;
    int64_t K;
    if (!vc_lex(q, gc, dim, axis, I, J, K)) return;
    const int t0 = axis == 0 ? 1 : 0;                // the lower tangential axis
    const int t1 = axis == 2 ? 1 : 2;                // the upper one (3D)
    const int i = 2 * I, j = 2 * J;
    const int64_t k = dim == 3 ? 2 * K : 0;
    auto fine = [&](int a, int b) {
        const int di = (t0 == 0 ? a : 0), dj = (t0 == 1 ? a : 0) + (t1 == 1 ? b : 0), dk = (t1 == 2 ? b : 0);
        return *vc_face(vf, g, axis, i + di, j + dj, k + dk);
    };
    T s = fine(0, 0) + fine(1, 0);
    if (dim == 3) {
        s = s + fine(0, 1);
        s = s + fine(1, 1);
        s = s * (T)0.25;
    } else {
        s = s * (T)0.5;
    }
    *vc_face(vc, gc, axis, I, J, K) = s;
}

// ---- the operator at one cell (scalar loads; any level size, nx = 1 included) -------------------------------------
// own / oth: the packed offsets of cell (i, j, k) and of the same slot in the other half.  s and dg as the header
// defines them; dividing by hSq = multiplying by inv_hSq exactly (a power of two, no underflow: beta > 0, h <= 1).
template <typename T, int DIM>
__device__ __forceinline__ void vc_stencil(const T* u, const VcT<T>& v, const Geo& g, T cl, T inv_hSq, int i, int j,
                                           int64_t k, int64_t own, int64_t oth, T& s, T& dg)
{
    const int o = i & 1;
    const bool wxl = i == 0, wxr = i == g.nx - 1, wyl = j == 0, wyr = j == g.ny - 1;
    const T bxl = v.bx[own];
    const T bxr = wxr ? v.wx[k * g.ny + j] : v.bx[oth + o];
    const T byl = v.by[own];
    const T byr = wyr ? v.wy[(k * 2 + o) * g.hw + (i >> 1)] : v.by[oth + g.hw];
    const T xl = wxl ? (T)0 : u[oth - 1 + o];
    const T xr = wxr ? (T)0 : u[oth + o];
    const T yl = wyl ? (T)0 : u[oth - g.hw];
    const T yr = wyr ? (T)0 : u[oth + g.hw];
    s = bxl * xl + bxr * xr;
    s = s + byl * yl;
    s = s + byr * yr;
    T S = bxl + bxr;
    S = S + byl;
    S = S + byr;
    T W = (wxl ? bxl : (T)0) + (wxr ? bxr : (T)0);
    W = W + (wyl ? byl : (T)0);
    W = W + (wyr ? byr : (T)0);
    if (DIM == 3) {
        const int64_t gk = g.z0 + k;
        const bool wzl = gk == 0, wzr = gk == g.gnz - 1;
        const T bzl = v.bz[own];
        const T bzr = v.bz[oth + g.P];  // (the top wall's faces: the upper ghost plane)
        s = s + bzl * u[oth - g.P];     // (u's ghost planes at the box faces hold +0)
        s = s + bzr * u[oth + g.P];
        S = S + bzl;
        S = S + bzr;
        W = W + (wzl ? bzl : (T)0);
        W = W + (wzr ? bzr : (T)0);
    }
    dg = ((-S) - cl * W) * inv_hSq;
}

template <typename T>
__device__ __forceinline__ T vc_relax(T s, T fc, T dg, T inv_hSq)
{
    const T a = fc - s * inv_hSq;
    return dg == (T)0 ? (T)0 : a / dg;
}

template <typename T>
__device__ __forceinline__ T vc_residual(T s, T fc, T uc, T dg, T inv_hSq)
{
    const T askew = s * inv_hSq;
    const T a_u = askew + dg * uc;
    return fc - a_u;
}

template <typename T, int DIM>
__device__ __forceinline__ T vc_residual_at(const T* __restrict__ u, const T* __restrict__ f, const VcT<T>& v,
                                            const Geo& g, T cl, T inv_hSq, int i, int j, int64_t k)
{
    const int64_t c = pidx(g, i, j, k);
    const int64_t oth = c + ((c - k * g.P) >= g.H ? -g.H : g.H);
    T s, dg;
    vc_stencil<T, DIM>(u, v, g, cl, inv_hSq, i, j, k, c, oth, s, dg);
    return vc_residual(s, f[c], u[c], dg, inv_hSq);
}

// ---- half-sweep ----------------------------------------------------------------------------------------------------

// One item of the vector forms (rows of at least 16 bytes per colour, nx >= 2): the N consecutive cells of colour
// `color` at half positions m0 .. m0 + N - 1 of row j, plane k, relaxed (RES = false) or their residuals (RES = true).
// Per axis the own half's vector holds the lower faces and the other half's vector, at the address of the upper
// neighbours' u, the upper faces.  Every load is issued before the arithmetic.
template <typename T, int DIM, bool RES>
__device__ __forceinline__ Vec<T, VN<T>::n> vc_item(const T* __restrict__ u, const T* __restrict__ f, const Geo& g,
                                                    int color, const VcT<T>& v, T cl, T inv_hSq, int m0, int j,
                                                    int64_t k, int64_t& own_out)
{
    constexpr int N = VN<T>::n;
    const int64_t gk = g.z0 + k;
    const int o = color ^ (int)((j + gk) & 1);
    const int64_t own = k * g.P + color * g.H + (int64_t)j * g.hw + m0;
    const int64_t oth = k * g.P + (color ^ 1) * g.H + (int64_t)j * g.hw + m0;
    const bool last = m0 + N == g.hw, top = j == g.ny - 1;
    const Vec<T, N> cen = vload<T, N>(u + oth);
    T edge, bedge = (T)0;
    if (o == 0) {
        edge = m0 > 0 ? u[oth - 1] : (T)0;
    } else {
        edge = last ? (T)0 : u[oth + N];
        bedge = last ? v.wx[k * g.ny + j] : v.bx[oth + N];
    }
    const Vec<T, N> yl = j > 0 ? vload<T, N>(u + oth - g.hw) : vzero<T, N>();
    const Vec<T, N> yr = top ? vzero<T, N>() : vload<T, N>(u + oth + g.hw);
    Vec<T, N> zl, zr, bzo, bzn, uc;
    if (DIM == 3) {
        zl = vload<T, N>(u + oth - g.P);
        zr = vload<T, N>(u + oth + g.P);
        bzo = vload<T, N>(v.bz + own);
        bzn = vload<T, N>(v.bz + oth + g.P);
    }
    if (RES) uc = vload<T, N>(u + own);
    const Vec<T, N> fv = vload<T, N>(f + own);
    const Vec<T, N> bxo = vload<T, N>(v.bx + own);
    const Vec<T, N> bxn = vload<T, N>(v.bx + oth);
    const Vec<T, N> byo = vload<T, N>(v.by + own);
    const Vec<T, N> byn = top ? vload<T, N>(v.wy + (k * 2 + o) * g.hw + m0) : vload<T, N>(v.by + oth + g.hw);
    const bool wyl = j == 0, wzl = DIM == 3 && gk == 0, wzr = DIM == 3 && gk == g.gnz - 1;
    // a wall face in this item: S_wall is +0 otherwise, and (-S) - cl (+-0) = -S
    const bool wall = cl != (T)0 && (wyl || top || wzl || wzr || m0 == 0 || last);
    Vec<T, N> out;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int i = 2 * (m0 + e) + o;
        const T xl = o == 0 ? (e == 0 ? edge : cen.v[e - 1]) : cen.v[e];
        const T xr = o == 0 ? cen.v[e] : (e == N - 1 ? edge : cen.v[e + 1]);
        const T bxl = bxo.v[e];
        const T bxr = o == 0 ? bxn.v[e] : (e == N - 1 ? bedge : bxn.v[e + 1]);
        T s = bxl * xl + bxr * xr;
        s = s + byo.v[e] * yl.v[e];
        s = s + byn.v[e] * yr.v[e];
        T S = bxl + bxr;
        S = S + byo.v[e];
        S = S + byn.v[e];
        if (DIM == 3) {
            s = s + bzo.v[e] * zl.v[e];
            s = s + bzn.v[e] * zr.v[e];
            S = S + bzo.v[e];
            S = S + bzn.v[e];
        }
        T d = -S;
        if (wall) {
            T W = (i == 0 ? bxl : (T)0) + (i == g.nx - 1 ? bxr : (T)0);
            W = W + (wyl ? byo.v[e] : (T)0);
            W = W + (top ? byn.v[e] : (T)0);
            if (DIM == 3) {
                W = W + (wzl ? bzo.v[e] : (T)0);
                W = W + (wzr ? bzn.v[e] : (T)0);
            }
            d = d - cl * W;
        }
        out.v[e] = RES ? vc_residual(s, fv.v[e], uc.v[e], d * inv_hSq, inv_hSq) : vc_relax(s, fv.v[e], d * inv_hSq, inv_hSq);
    }
    own_out = own;
    return out;
}

// Vector half-sweep: k_half's item, a thread owns N consecutive cells of colour `color` in one row
template <typename T, int DIM, bool ERR>
__global__ __launch_bounds__(kBlock) void k_half_vc(const T* __restrict__ other, const T* __restrict__ f,
                                                    T* __restrict__ dst, const T* __restrict__ old,
                                                    double* __restrict__ partials, Geo g, int color, VcT<T> v, T cl,
                                                    T inv_hSq)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    double acc = 0.0;
    const int lgpr = g.lhw - LN;
    if ((it >> (lgpr + g.ly)) < g.nz) {
        const int m0 = (int)(it & ((1 << lgpr) - 1)) * N;
        const int j = (int)((it >> lgpr) & (g.ny - 1));
        const int64_t k = it >> (lgpr + g.ly);
        int64_t own;
        const Vec<T, N> out = vc_item<T, DIM, false>(other, f, g, color, v, cl, inv_hSq, m0, j, k, own);
        vstore<T, N>(dst + own, out);
        if (ERR) {
            const Vec<T, N> w = vload<T, N>(old + own);
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const double d = (double)out.v[e] - (double)w.v[e];
                acc += d * d;
            }
        }
    }
    if (ERR) block_partial<T>(acc, partials);
}

// Scalar form (shorter rows, nx = 1, the one-cell level): half_item's slot
template <typename T, int DIM, bool ERR>
__global__ __launch_bounds__(kBlock) void k_half_vc_s(const T* other, const T* __restrict__ f, T* dst,
                                                      const T* __restrict__ old, double* __restrict__ partials, Geo g,
                                                      int color, VcT<T> v, T cl, T inv_hSq)
{
    const int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double acc = 0.0;
    if (it < g.H * g.nz) {
        const int m = (int)(it & (g.hw - 1));
        const int j = (int)((it >> g.lhw) & (g.ny - 1));
        const int64_t k = it >> (g.lhw + g.ly);
        const int o = color ^ (int)((j + g.z0 + k) & 1);
        const int i = 2 * m + o;
        if (i < g.nx) {
            const int64_t own = k * g.P + color * g.H + (int64_t)j * g.hw + m;
            const int64_t oth = k * g.P + (color ^ 1) * g.H + (int64_t)j * g.hw + m;
            T s, dg;
            vc_stencil<T, DIM>(other, v, g, cl, inv_hSq, i, j, k, own, oth, s, dg);
            const T r = vc_relax(s, f[own], dg, inv_hSq);
            dst[own] = r;
            if (ERR) {
                const double d = (double)r - (double)old[own];
                acc += d * d;
            }
        }
    }
    if (ERR) block_partial<T>(acc, partials);
}

// ---- residual: restricted, as a field, as norms --------------------------------------------------------------------

// resrestrict_item with A_beta: the 2^d children's residuals in reduceResidual's order
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_resrestrict_vc_s(const T* __restrict__ u, const T* __restrict__ f,
                                                             T* __restrict__ R, Geo g, Geo gc, VcT<T> v, T cl, T inv_hSq)
{
    const int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (it >= resrestrict_items<T, DIM>(g)) return;
    const int cx = g.nx >> 1, cy = g.ny >> 1;
    const int lcx = g.lx - 1, lcy = g.ly - 1;
    const int I = (int)(it & (cx - 1));
    const int J = (int)((it >> lcx) & (cy - 1));
    const int64_t K = it >> (lcx + lcy);
    const int i = 2 * I, j = 2 * J;
    const int64_t k = DIM == 3 ? 2 * K : 0;
    auto r = [&](int a, int b, int64_t c) { return vc_residual_at<T, DIM>(u, f, v, g, cl, inv_hSq, a, b, c); };
    T s = r(i, j, k) + r(i + 1, j, k);
    s = s + r(i, j + 1, k);
    s = s + r(i + 1, j + 1, k);
    if (DIM == 3) {
        s = s + r(i, j, k + 1);
        s = s + r(i + 1, j, k + 1);
        s = s + r(i, j + 1, k + 1);
        s = s + r(i + 1, j + 1, k + 1);
        R[pidx(gc, I, J, K)] = (T)0.125 * s;
    } else {
        R[pidx(gc, I, J, 0)] = (T)0.25 * s;
    }
}

// Vector form: k_resrestrict's item, a thread owns N consecutive coarse cells I0 .. I0 + N - 1 of one coarse row; their
// children are, in every fine row, the N cells m = I0 .. of BOTH colours, each colour one vc_item (16-byte loads; rows
// shared between the items of a thread come from cache).  The same sum order as the scalar form.
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_resrestrict_vc(const T* __restrict__ u, const T* __restrict__ f,
                                                           T* __restrict__ R, Geo g, Geo gc, VcT<T> v, T cl, T inv_hSq)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int cy = g.ny >> 1;
    const int lgpr = (g.lx - 1) - LN;  // log2 groups of N per coarse row
    const int64_t ncz = DIM == 3 ? (g.nz >> 1) : 1;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    const int m0 = (int)(it & ((1 << lgpr) - 1)) * N;
    const int J = (int)((it >> lgpr) & (cy - 1));
    const int64_t K = it >> (lgpr + g.ly - 1);
    if (K >= ncz) return;
    T acc[N];
#pragma unroll
    for (int dz = 0; dz < (DIM == 3 ? 2 : 1); ++dz) {
        const int64_t k = DIM == 3 ? 2 * K + dz : 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int j = 2 * J + dy;
            const int p = (int)((j + g.z0 + k) & 1);
            int64_t own;
            // the colour whose cells have even x in this row first: r(i, j, k) + r(i + 1, j, k)
            const Vec<T, N> r0 = vc_item<T, DIM, true>(u, f, g, p, v, cl, inv_hSq, m0, j, k, own);
            const Vec<T, N> r1 = vc_item<T, DIM, true>(u, f, g, p ^ 1, v, cl, inv_hSq, m0, j, k, own);
#pragma unroll
            for (int e = 0; e < N; ++e) {
                if (dz == 0 && dy == 0) {
                    acc[e] = r0.v[e] + r1.v[e];
                } else {
                    acc[e] = acc[e] + r0.v[e];
                    acc[e] = acc[e] + r1.v[e];
                }
            }
        }
    }
    const int pc = (int)((J + gc.z0 + K) & 1);
    const int64_t rowc = K * gc.P + (int64_t)J * gc.hw;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int I = m0 + e;
        R[rowc + ((I + pc) & 1) * gc.H + (I >> 1)] = (DIM == 3 ? (T)0.125 : (T)0.25) * acc[e];
    }
}

template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_residual_vc(const T* __restrict__ u, const T* __restrict__ f,
                                                        T* __restrict__ r, Geo g, VcT<T> v, T cl, T inv_hSq)
{
    const int64_t n = g.P * g.nz;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        int i, j;
        int64_t k;
        r[s] = slot_cell(s, g, i, j, k) ? vc_residual_at<T, DIM>(u, f, v, g, cl, inv_hSq, i, j, k) : (T)0;
    }
}

// k_resnorm_s's scheme: fp64 per wave, per workgroup, then launch_sum_partials' fixed order
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_resnorm_vc(const T* __restrict__ u, const T* __restrict__ f, Geo g,
                                                       VcT<T> v, T cl, T inv_hSq, double* __restrict__ partials,
                                                       int fofs)
{
    const int64_t n = g.P * g.nz;
    double rr = 0.0, ff = 0.0;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        int i, j;
        int64_t k;
        if (slot_cell(s, g, i, j, k)) {
            const T r = vc_residual_at<T, DIM>(u, f, v, g, cl, inv_hSq, i, j, k);
            rr += (double)r * (double)r;
            ff += (double)f[s] * (double)f[s];
        }
    }
    rr = wave_sum(rr);
    ff = wave_sum(ff);
    __shared__ double ws[2][kBlock / 64];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        ws[0][w] = rr;
        ws[1][w] = ff;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int q = 0; q < kBlock / 64; ++q) {
            a += ws[0][q];
            b += ws[1][q];
        }
        partials[blockIdx.x] = a;
        partials[fofs + blockIdx.x] = b;
    }
}

// ---- gradient with coefficients: grad_slot's faces (mgp_project.hip), each times its beta ---------------------------

template <typename T, bool SUBTRACT>
__device__ __forceinline__ void vc_face_out(T* __restrict__ p, T beta, T gv)
{
    const T bg = beta * gv;
    *p = SUBTRACT ? *p - bg : bg;
}

template <typename T, int DIM, bool SUBTRACT>
__global__ __launch_bounds__(kBlock) void k_grad_vc(const T* __restrict__ u, T* __restrict__ vx, T* __restrict__ vy,
                                                    T* __restrict__ vz, Geo g, VcT<T> v, T ih, T mc)
{
    const int64_t nx = g.nx, ny = g.ny;
    const int64_t n = 2 * g.H * g.nz;
    for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n; c += (int64_t)gridDim.x * kBlock) {
        const int64_t o = level_slot(c, g.lhw + g.ly + 1, g.P);
        int i, j;
        int64_t k;
        if (!slot_cell(o, g, i, j, k)) continue;
        const T e = u[o], gh = mc * e;
        {
            T* x = vx + (k * ny + j) * (nx + 1) + i;
            const T lo = i > 0 ? u[pidx(g, i - 1, j, k)] : gh;
            vc_face_out<T, SUBTRACT>(x, v.bx[o], (e - lo) * ih);
            if (i == g.nx - 1) vc_face_out<T, SUBTRACT>(x + 1, v.wx[k * g.ny + j], (gh - e) * ih);
        }
        {
            T* y = vy + (k * (ny + 1) + j) * nx + i;
            const T lo = j > 0 ? u[pidx(g, i, j - 1, k)] : gh;
            vc_face_out<T, SUBTRACT>(y, v.by[o], (e - lo) * ih);
            if (j == g.ny - 1) vc_face_out<T, SUBTRACT>(y + nx, *vc_face(v, g, 1, i, g.ny, k), (gh - e) * ih);
        }
        if (DIM == 3) {
            T* z = vz + (k * ny + j) * nx + i;
            const T lo = k > 0 ? u[pidx(g, i, j, k - 1)] : gh;
            vc_face_out<T, SUBTRACT>(z, v.bz[o], (e - lo) * ih);
            if (k == g.nz - 1) vc_face_out<T, SUBTRACT>(z + nx * ny, *vc_face(v, g, 2, i, j, g.nz), (gh - e) * ih);
        }
    }
}

template <typename T>
T inv_hsq(double h)
{
    const T hh = (T)h;
    return (T)1 / (hh * hh);  // exact: h is a power of two (make_op)
}

int64_t vc_faces(const Geo& g, int dim, int axis)
{
    return (int64_t)(g.nx + (axis == 0)) * (g.ny + (axis == 1)) * (dim == 3 ? g.nz + (axis == 2) : 1);
}

bool vc_vector(int rb, const Geo& g) { return g.hw >= 16 / rb && g.nx >= 2; }

template <typename T, int D>
void half_vc_t(unsigned nb, int color, const void* other, const void* f, void* dst, const void* old, double* partials,
               const Geo& g, double h, double cl, const VcCoef& vc, hipStream_t s)
{
    const VcT<T> v = vc_view<T>(vc);
    const T *o_ = (const T*)other, *f_ = (const T*)f, *w_ = (const T*)old;
    const T c = (T)cl, ih = inv_hsq<T>(h);
    if (vc_vector(sizeof(T), g)) {
        if (old) k_half_vc<T, D, true><<<nb, kBlock, 0, s>>>(o_, f_, (T*)dst, w_, partials, g, color, v, c, ih);
        else k_half_vc<T, D, false><<<nb, kBlock, 0, s>>>(o_, f_, (T*)dst, w_, partials, g, color, v, c, ih);
    } else {
        if (old) k_half_vc_s<T, D, true><<<nb, kBlock, 0, s>>>(o_, f_, (T*)dst, w_, partials, g, color, v, c, ih);
        else k_half_vc_s<T, D, false><<<nb, kBlock, 0, s>>>(o_, f_, (T*)dst, w_, partials, g, color, v, c, ih);
    }
}

}  // namespace

#define MGP_VC_DIM(dim, BODY)      \
    do {                           \
        if (dim == 3) {            \
            constexpr int D = 3;   \
            BODY;                  \
        } else {                   \
            constexpr int D = 2;   \
            BODY;                  \
        }                          \
    } while (0)

hipError_t launch_vc_check(int rb, const void* p, int64_t n, int* bad, int bit, hipStream_t s)
{
    const unsigned nb = std::min(nblk_gs(n), 4096u);
    MGP_REAL(rb, (k_vc_check<T><<<nb, kBlock, 0, s>>>((const T*)p, n, bad, bit)));
    return hipGetLastError();
}

hipError_t launch_vc_pack(int rb, int dim, int axis, const void* lex, VcCoef vc, Geo g, hipStream_t s)
{
    const unsigned nb = nblk(vc_faces(g, dim, axis));
    MGP_REAL(rb, (k_vc_pack<T><<<nb, kBlock, 0, s>>>((const T*)lex, vc_view<T>(vc), g, dim, axis)));
    return hipGetLastError();
}

hipError_t launch_vc_unpack(int rb, int dim, int axis, VcCoef vc, void* lex, Geo g, hipStream_t s)
{
    const unsigned nb = nblk(vc_faces(g, dim, axis));
    MGP_REAL(rb, (k_vc_unpack<T><<<nb, kBlock, 0, s>>>(vc_view<T>(vc), (T*)lex, g, dim, axis)));
    return hipGetLastError();
}

hipError_t launch_vc_coarsen(int rb, int dim, int axis, VcCoef fine, Geo g, VcCoef coarse, Geo gc, hipStream_t s)
{
    const unsigned nb = nblk(vc_faces(gc, dim, axis));
    MGP_REAL(rb, (k_vc_coarsen<T><<<nb, kBlock, 0, s>>>(vc_view<T>(fine), g, vc_view<T>(coarse), gc, dim, axis)));
    return hipGetLastError();
}

int half_blocks_vc(int rb, Geo g)
{
    return (int)nblk(vc_vector(rb, g) ? (g.H / (16 / rb)) * g.nz : g.H * g.nz);
}

hipError_t launch_half_sweep_vc(int rb, int dim, int color, const void* other, const void* f, void* dst, const void* old,
                                double* partials, Geo g, double h, double cl, VcCoef vc, hipStream_t s)
{
    const unsigned nb = (unsigned)half_blocks_vc(rb, g);
    MGP_REAL(rb, MGP_VC_DIM(dim, (half_vc_t<T, D>(nb, color, other, f, dst, old, partials, g, h, cl, vc, s))));
    return hipGetLastError();
}

hipError_t launch_residual_restrict_vc(int rb, int dim, const void* u, const void* f, void* R, Geo g, Geo gc, double h,
                                       double cl, VcCoef vc, const PieceTuning& pt, hipStream_t s)
{
    const int n = 16 / rb, cx = g.nx / 2;
    const int64_t rows = (int64_t)(g.ny / 2) * (dim == 3 ? g.nz / 2 : 1);
    // A thread per coarse cell by default on every level: at 512^3 -> 256^3 (fp32) the cycle measured 5.55 ms with it
    // and 5.70 ms with the 16-byte form, whose items re-read the rows they share.  The 16-byte form runs where
    // MGP_RR_SCALAR_CELLS is given and the level has at least that many coarse cells (rows of at least 16 bytes).
    if (pt.rr_scalar_env && cx >= n && cx * rows >= pt.rr_scalar_cells) {
        MGP_REAL(rb, MGP_VC_DIM(dim, (k_resrestrict_vc<T, D><<<nblk((cx / n) * rows), kBlock, 0, s>>>(
                                         (const T*)u, (const T*)f, (T*)R, g, gc, vc_view<T>(vc), (T)cl, inv_hsq<T>(h)))));
        return hipGetLastError();
    }
    MGP_REAL(rb, MGP_VC_DIM(dim, (k_resrestrict_vc_s<T, D><<<nblk(cx * rows), kBlock, 0, s>>>(
                                     (const T*)u, (const T*)f, (T*)R, g, gc, vc_view<T>(vc), (T)cl, inv_hsq<T>(h)))));
    return hipGetLastError();
}

hipError_t launch_residual_field_vc(int rb, int dim, const void* u, const void* f, void* r, Geo g, double h, double cl,
                                    VcCoef vc, hipStream_t s)
{
    const unsigned nb = nblk_gs(g.P * g.nz);
    MGP_REAL(rb, MGP_VC_DIM(dim, (k_residual_vc<T, D><<<nb, kBlock, 0, s>>>((const T*)u, (const T*)f, (T*)r, g,
                                                                            vc_view<T>(vc), (T)cl, inv_hsq<T>(h)))));
    return hipGetLastError();
}

int resnorm_blocks_vc(Geo g) { return (int)std::min(nblk_gs(g.P * g.nz), 4096u); }

hipError_t launch_residual_norm_vc(int rb, int dim, const void* u, const void* f, Geo g, double h, double cl, VcCoef vc,
                                   double* partials, double* out, hipStream_t s)
{
    const int nb = resnorm_blocks_vc(g);
    const int fofs = nb + sum_scratch(nb);
    MGP_REAL(rb, MGP_VC_DIM(dim, (k_resnorm_vc<T, D><<<nb, kBlock, 0, s>>>((const T*)u, (const T*)f, g, vc_view<T>(vc),
                                                                           (T)cl, inv_hsq<T>(h), partials, fofs))));
    (void)launch_sum_partials(partials, nb, out, s);
    (void)launch_sum_partials(partials + fofs, nb, out + 1, s);
    return hipGetLastError();
}

hipError_t launch_gradient_vc(int rb, int dim, bool subtract, const void* u, void* vx, void* vy, void* vz, Geo g,
                              double cl, VcCoef vc, hipStream_t s)
{
    const unsigned nb = nblk_gs(2 * g.H * g.nz);
    if (subtract)
        MGP_REAL(rb, MGP_VC_DIM(dim, (k_grad_vc<T, D, true><<<nb, kBlock, 0, s>>>((const T*)u, (T*)vx, (T*)vy, (T*)vz, g,
                                                                                  vc_view<T>(vc), (T)g.nx, -(T)cl))));
    else
        MGP_REAL(rb, MGP_VC_DIM(dim, (k_grad_vc<T, D, false><<<nb, kBlock, 0, s>>>((const T*)u, (T*)vx, (T*)vy, (T*)vz, g,
                                                                                   vc_view<T>(vc), (T)g.nx, -(T)cl))));
    return hipGetLastError();
}

}  // namespace mgp
