// mgp_cell.h — the scalar per-cell arithmetic of the cycle's pieces, which the tiled and tail engines restate "in its
// order": one slot of a half-sweep (half_item), the residual of a cell (residual_at), the residual + restriction of a
// coarse cell (resrestrict_item), the full weighting (fw_eval) and the prolongation (prolong_value, prolong_item).
// Used by mgp_kernels.hip (one launch per piece), mgp_blk.hip (tiled phases) and mgp_tail.hip (coarse tail).
// Everything is internal to each translation unit (anonymous namespace).
#pragma once
#include "mgp_device.h"

namespace mgp {
namespace {

// One colour-c slot of a half-sweep (scalar; any level size, nx = 1 included).  Returns the
// packed index written, or -1 for the empty slot of an nx = 1 row; *v = the new value.
// C: the type the expression is evaluated in (C = double with T = float: cpu-raw.lua's real = 'float',
// LuaJIT doubles rounded once at the store, cpu-raw.lua:34-44); with C = T every cast is the identity.
template <typename T, int DIM, typename C = T>
__device__ __forceinline__ int64_t half_item(const T* other, const T* __restrict__ f, T* dst, const Geo& g,
                                             int color, const Op<C, DIM>& op, int64_t it, T* v)
{
    const int m = (int)(it & (g.hw - 1));
    const int j = (int)((it >> g.lhw) & (g.ny - 1));
    const int64_t k = it >> (g.lhw + g.ly);
    const int64_t gk = g.z0 + k;
    const int o = color ^ (int)((j + gk) & 1);
    const int i = 2 * m + o;
    if (i >= g.nx) return -1;
    const int64_t own = k * g.P + color * g.H + (int64_t)j * g.hw + m;
    const int64_t oth = k * g.P + (color ^ 1) * g.H + (int64_t)j * g.hw + m;
    const C xl = i > 0 ? (C)other[oth - 1 + o] : (C)0;
    const C xr = i < g.nx - 1 ? (C)other[oth + o] : (C)0;
    C s = xl + xr;
    s = s + (j > 0 ? (C)other[oth - g.hw] : (C)0);
    s = s + (j < g.ny - 1 ? (C)other[oth + g.hw] : (C)0);
    if (DIM == 3) {
        s = s + (C)other[oth - g.P];
        s = s + (C)other[oth + g.P];
    }
    const int nb = (i == 0) + (i == g.nx - 1) + (j == 0) + (j == g.ny - 1) +
                   (DIM == 3 ? (gk == 0) + (gk == g.gnz - 1) : 0);
    *v = (T)op.relax_z(s, (C)f[own], nb);
    dst[own] = *v;
    return own;
}

// Residual of one fine cell from packed u (generic, scalar loads), evaluated in C (half_item's C).
template <typename T, int DIM, typename C = T>
__device__ __forceinline__ C residual_at(const T* __restrict__ u, const T* __restrict__ f, const Geo& g,
                                         const Op<C, DIM>& op, int i, int j, int64_t k)
{
    const int64_t c = pidx(g, i, j, k);
    const int o = i & 1;
    // neighbours: other colour, same row at m-1+o / m+o; rows j+-1 and planes k+-1 at m
    const int64_t oth = c + ((c - k * g.P) >= g.H ? -g.H : g.H);
    const C xl = i > 0 ? (C)u[oth - 1 + o] : (C)0;
    const C xr = i < g.nx - 1 ? (C)u[oth + o] : (C)0;
    C s = xl + xr;
    s = s + (j > 0 ? (C)u[oth - g.hw] : (C)0);
    s = s + (j < g.ny - 1 ? (C)u[oth + g.hw] : (C)0);
    const int64_t gk = g.z0 + k;
    if (DIM == 3) {
        s = s + (C)u[oth - g.P];
        s = s + (C)u[oth + g.P];
    }
    const int nb = (i == 0) + (i == g.nx - 1) + (j == 0) + (j == g.ny - 1) + (DIM == 3 ? (gk == 0) + (gk == g.gnz - 1) : 0);
    return op.residual(s, (C)f[c], (C)u[c], nb);
}

// One coarse cell of the fused residual + restriction (scalar; any sizes).  C = double (cpu-raw.lua's float):
// each child residual is rounded to the real type first (calcResidual stores it in rs[L], cpu-raw.lua:211),
// then summed and scaled in double and rounded once (reduceResidual, cpu-raw.lua:59-63).
template <typename T, int DIM, typename C = T>
__device__ __forceinline__ void resrestrict_item(const T* u, const T* f, T* R, const Geo& g, const Geo& gc,
                                                 const Op<C, DIM>& op, int64_t it)
{
    const int cx = g.nx >> 1, cy = g.ny >> 1;
    const int lcx = g.lx - 1, lcy = g.ly - 1;
    const int I = (int)(it & (cx - 1));
    const int J = (int)((it >> lcx) & (cy - 1));
    const int64_t K = it >> (lcx + lcy);
    const int i = 2 * I, j = 2 * J;
    const int64_t k = DIM == 3 ? 2 * K : 0;
    auto r = [&](int a, int b, int64_t c) { return (C)(T)residual_at<T, DIM, C>(u, f, g, op, a, b, c); };
    C s = r(i, j, k) + r(i + 1, j, k);
    s = s + r(i, j + 1, k);
    s = s + r(i + 1, j + 1, k);
    if (DIM == 3) {
        s = s + r(i, j, k + 1);
        s = s + r(i + 1, j, k + 1);
        s = s + r(i, j + 1, k + 1);
        s = s + r(i + 1, j + 1, k + 1);
        R[pidx(gc, I, J, K)] = (T)((C)0.125 * s);
    } else {
        R[pidx(gc, I, J, 0)] = (T)((C)0.25 * s);
    }
}

template <typename T, int DIM>
__device__ __forceinline__ int64_t resrestrict_items(const Geo& g)
{
    return (int64_t)(g.nx >> 1) * (g.ny >> 1) * (DIM == 3 ? (g.nz >> 1) : 1);
}

// Coarse cell (I, J, local plane K) from fine residuals get(i, j, k) (k local; called only for cells
// inside the box).  gc.z0 = g.z0 / 2 (the coarse plane of this rank's fine plane 0).
template <typename T, int DIM, typename Get>
__device__ __forceinline__ T fw_eval(const Get& get, const Geo& g, const Geo& gc, T wf, int I, int J, int64_t K)
{
    const T w3 = (T)3;
    T az = (T)0;
#pragma unroll
    for (int dz = 0; dz < (DIM == 3 ? 4 : 1); ++dz) {
        const int64_t k = DIM == 3 ? 2 * K - 1 + dz : 0;
        const bool kin = DIM == 2 || (g.z0 + k >= 0 && g.z0 + k < g.gnz);
        T ay = (T)0;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const int j = 2 * J - 1 + dy;
            const bool jin = kin && j >= 0 && j < g.ny;
            T x[4];
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
                const int i = 2 * I - 1 + dx;
                x[dx] = (jin && i >= 0 && i < g.nx) ? get(i, j, k) : (T)0;
            }
            const T ax = fw_axis(x[0], x[1], x[2], x[3], I == 0 ? wf : w3, I == gc.nx - 1 ? wf : w3);
            // ay = ((ax0 + wb ax1) + wc ax2) + ax3, accumulated row by row
            if (dy == 0) ay = ax;
            else if (dy == 1) ay = ay + (J == 0 ? wf : w3) * ax;
            else if (dy == 2) ay = ay + (J == gc.ny - 1 ? wf : w3) * ax;
            else ay = ay + ax;
        }
        if (DIM == 2) {
            az = ay;
        } else {
            const int64_t gK = gc.z0 + K;
            if (dz == 0) az = ay;
            else if (dz == 1) az = az + (gK == 0 ? wf : w3) * ay;
            else if (dz == 2) az = az + (gK == gc.gnz - 1 ? wf : w3) * ay;
            else az = az + ay;
        }
    }
    return (DIM == 3 ? (T)(1.0 / 512.0) : (T)(1.0 / 64.0)) * az;
}

// (P V) at fine cell (i, j, local plane k) from the packed coarse level V
template <typename T, int DIM, int LINEAR>
__device__ __forceinline__ T prolong_value(const T* V, const Geo& g, const Geo& gc, T cl, int i, int j, int64_t k)
{
    auto get = [&](int I, int J, int64_t K) { return V[pidx(gc, I, J, K)]; };
    return prolong_eval<T, DIM, LINEAR>(get, gc, cl, i, j, k);
}

// One fine slot of colour `color` of the prolongation + correction (scalar; any sizes).  C = double
// (cpu-raw.lua's float): P V evaluated in double and rounded into the real type (the vs[L] buffer,
// cpu-raw.lua:226), then addTo's u + v in double, rounded once (cpu-raw.lua:83-85).
template <typename T, int DIM, int LINEAR, typename C = T>
__device__ __forceinline__ void prolong_item(T* u, const T* V, const Geo& g, const Geo& gc, C cl, int color,
                                             int64_t it)
{
    const int m = (int)(it & (g.hw - 1));
    const int j = (int)((it >> g.lhw) & (g.ny - 1));
    const int64_t k = it >> (g.lhw + g.ly);
    const int o = color ^ (int)((j + g.z0 + k) & 1);
    const int i = 2 * m + o;
    if (i >= g.nx) return;
    const int64_t own = k * g.P + color * g.H + (int64_t)j * g.hw + m;
    auto get = [&](int I, int J, int64_t K) { return (C)V[pidx(gc, I, J, K)]; };
    const T v = (T)prolong_eval<C, DIM, LINEAR>(get, gc, cl, i, j, k);
    u[own] = (T)((C)u[own] + (C)v);
}

}  // namespace
}  // namespace mgp
