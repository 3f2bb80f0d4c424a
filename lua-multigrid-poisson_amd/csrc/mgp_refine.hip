// mgp_refine.hip — the two fp64 / fp32 streaming passes of mixed-precision defect correction on the finest
// level (mgp_refine_*; the outer loop cpu.lua:196-216 with real = 'double', around fp32 cycles):
//   k_defect      r = f - A psi in double from the fp64 psi and f (Op<double, DIM>::residual with level 0's cl:
//                 bit for bit launch_residual_field(rb = 8); CL = false is the cl = 0 pass, CL = true a separate
//                 instantiation with the boundary-modified diagonal of MGP_BC_FACE / _NEUMANN), stored as (float)r
//                 at the same packed slot of the fp32 level-0 f; sum r^2 (before narrowing) and sum f^2 in fp64; optionally +0.0f to the fp32 u
//                 (the zero guess of the inner cycles).  24 B per cell: read psi and f, write r32 and u32.
//   k_refine_add  psi += (double)e from the fp32 level-0 u, sum e^2 in fp64.  20 B per cell.
// The fp64 fields have level 0's packed red/black layout (Geo / pidx), so a cell has one index in all four arrays.
// Reductions have k_resnorm's shape: a butterfly per wave, the 4 wave sums of a workgroup in fixed order, then
// launch_sum_partials.
#include "mgp_device.h"

#include <algorithm>

namespace mgp {
namespace {

using V2 = Vec<double, 2>;
using F2 = Vec<float, 2>;

constexpr int kDefectGsBlocks = 2048;  // grid-stride form (XCD-banded), as the half-sweeps' kGsBlocks
constexpr int kDefectMaxBlocks = 4096;
constexpr int kAddMaxBlocks = 65536;   // one launch_sum_partials kernel (sum_scratch() == 0)

// rr, ff (per thread) -> one pair per workgroup: partials[b], partials[fofs + b]
__device__ __forceinline__ void block_pair(double rr, double ff, double* __restrict__ partials, int fofs)
{
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
        for (int k = 0; k < kBlock / 64; ++k) {
            a += ws[0][k];
            b += ws[1][k];
        }
        partials[blockIdx.x] = a;
        if (fofs) partials[fofs + blockIdx.x] = b;
    }
}

// Vector form (hw >= 2): an item is two consecutive cells of one colour in one row.  Items are ordered plane,
// colour, row, group, so a contiguous range of items is a contiguous range of every array and both colours of a
// plane (each the other's neighbours) are swept together.
struct DefectIn {
    V2 cen, yl, yr, zl, zr, fv, uc;
    double edge;
    int64_t own;
    int o;
    int nbyz, i0;  // CL: the cells' y / z faces on the box, x of the first cell
};

template <int DIM, bool CL>
__device__ __forceinline__ void defect_load(DefectIn& in, const double* __restrict__ psi, const double* __restrict__ f,
                                            const Geo& g, int64_t it)
{
    const int lg = g.lhw - 1;    // log2 groups per half row
    const int lpc = lg + g.ly;   // log2 items per colour of a plane
    const int64_t q = it >> lpc;
    const int64_t k = q >> 1;
    const int color = (int)(q & 1);
    const int grp = (int)(it & ((1 << lg) - 1));
    const int j = (int)((it >> lg) & (g.ny - 1));
    const int m0 = 2 * grp;
    const int o = color ^ (int)((j + g.z0 + k) & 1);  // x parity of this row's colour-c cells
    const int64_t own = k * g.P + color * g.H + (int64_t)j * g.hw + m0;
    const int64_t oth = k * g.P + (color ^ 1) * g.H + (int64_t)j * g.hw + m0;
    in.cen = vload<double, 2>(psi + oth);
    if (o == 0)
        in.edge = m0 > 0 ? psi[oth - 1] : 0.0;          // x-1 of the first cell
    else
        in.edge = m0 + 2 < g.hw ? psi[oth + 2] : 0.0;   // x+1 of the last cell
    in.yl = j > 0 ? vload<double, 2>(psi + oth - g.hw) : vzero<double, 2>();
    in.yr = j < g.ny - 1 ? vload<double, 2>(psi + oth + g.hw) : vzero<double, 2>();
    if (DIM == 3) {
        in.zl = vload<double, 2>(psi + oth - g.P);  // (a zero ghost plane at the box's ends)
        in.zr = vload<double, 2>(psi + oth + g.P);
    }
    in.fv = vload<double, 2>(f + own);
    in.uc = vload<double, 2>(psi + own);
    in.own = own;
    in.o = o;
    if (CL) {
        const int64_t gk = g.z0 + k;
        in.nbyz = (j == 0) + (j == g.ny - 1) + (DIM == 3 ? (gk == 0) + (gk == g.gnz - 1) : 0);
        in.i0 = 2 * m0 + o;
    }
}

template <int DIM, bool ZERO, bool CL>
__device__ __forceinline__ void defect_store(const DefectIn& in, float* __restrict__ r32, float* __restrict__ u32,
                                             const Op<double, DIM>& op, const Geo& g, double& rr, double& ff)
{
    const int o = in.o;
    F2 out;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const double xl = o == 0 ? (e == 0 ? in.edge : in.cen.v[0]) : in.cen.v[e];
        const double xr = o == 0 ? in.cen.v[e] : (e == 1 ? in.edge : in.cen.v[1]);
        double sm = xl + xr;
        sm = sm + in.yl.v[e];
        sm = sm + in.yr.v[e];
        if (DIM == 3) {
            sm = sm + in.zl.v[e];
            sm = sm + in.zr.v[e];
        }
        int nb = 0;
        if (CL) {
            const int i = in.i0 + 2 * e;
            nb = in.nbyz + (i == 0) + (i == g.nx - 1);
        }
        const double r = op.residual(sm, in.fv.v[e], in.uc.v[e], nb);
        out.v[e] = (float)r;
        rr = __builtin_fma(r, r, rr);
        ff = __builtin_fma(in.fv.v[e], in.fv.v[e], ff);
    }
    vstore<float, 2>(r32 + in.own, out);
    if (ZERO) vstore<float, 2>(u32 + in.own, vzero<float, 2>());
}

template <int DIM, bool ZERO, bool CL>
__global__ __launch_bounds__(kBlock) void k_defect(const double* __restrict__ psi, const double* __restrict__ f,
                                                   float* __restrict__ r32, float* __restrict__ u32, Geo g,
                                                   Op<double, DIM> op, int64_t items, double* __restrict__ partials,
                                                   int fofs)
{
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    double rr = 0.0, ff = 0.0;
    if (it < items) {
        DefectIn in;
        defect_load<DIM, CL>(in, psi, f, g, it);
        defect_store<DIM, ZERO, CL>(in, r32, u32, op, g, rr, ff);
    }
    block_pair(rr, ff, partials, fofs);
}

// Grid-stride form for large levels (gridDim.x a multiple of 8): the workgroups of XCD x (b % 8 == x) sweep the
// contiguous band x of the items, so y / z neighbours meet in that XCD's L2; two items' loads in flight per thread.
template <int DIM, bool ZERO, bool CL>
__global__ __launch_bounds__(kBlock) void k_defect_gs(const double* __restrict__ psi, const double* __restrict__ f,
                                                      float* __restrict__ r32, float* __restrict__ u32, Geo g,
                                                      Op<double, DIM> op, int64_t items, double* __restrict__ partials,
                                                      int fofs)
{
    const int nlb = gridDim.x >> 3;
    const int64_t band = (items + 7) >> 3;
    const int64_t base = (int64_t)(blockIdx.x & 7) * band;
    const int64_t end = base + band < items ? base + band : items;
    const int64_t step = (int64_t)nlb * kBlock;
    double rr = 0.0, ff = 0.0;
    for (int64_t i0 = base + (int64_t)(blockIdx.x >> 3) * kBlock + threadIdx.x; i0 < end; i0 += 2 * step) {
        const int64_t i1 = i0 + step;
        DefectIn a, c;
        defect_load<DIM, CL>(a, psi, f, g, i0);
        if (i1 < end) defect_load<DIM, CL>(c, psi, f, g, i1);
        defect_store<DIM, ZERO, CL>(a, r32, u32, op, g, rr, ff);
        if (i1 < end) defect_store<DIM, ZERO, CL>(c, r32, u32, op, g, rr, ff);
    }
    block_pair(rr, ff, partials, fofs);
}

// Scalar form for rows of one or two cells (hw < 2, nx = 1 included): a thread per packed slot, grid-stride.
// The empty slot of an nx = 1 row holds no cell: r32 = u32 = 0 there.
template <int DIM, bool ZERO, bool CL>
__global__ __launch_bounds__(kBlock) void k_defect_s(const double* __restrict__ psi, const double* __restrict__ f,
                                                     float* __restrict__ r32, float* __restrict__ u32, Geo g,
                                                     Op<double, DIM> op, double* __restrict__ partials, int fofs)
{
    const int64_t n = g.P * g.nz;
    double rr = 0.0, ff = 0.0;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        int i, j;
        int64_t k;
        float out = 0.0f;
        if (slot_cell(s, g, i, j, k)) {
            const int o = i & 1;
            // neighbours: the other colour, same row at m-1+o / m+o; rows j+-1 and planes k+-1 at m
            const int64_t oth = s + ((s - k * g.P) >= g.H ? -g.H : g.H);
            const double xl = i > 0 ? psi[oth - 1 + o] : 0.0;
            const double xr = i < g.nx - 1 ? psi[oth + o] : 0.0;
            double sm = xl + xr;
            sm = sm + (j > 0 ? psi[oth - g.hw] : 0.0);
            sm = sm + (j < g.ny - 1 ? psi[oth + g.hw] : 0.0);
            if (DIM == 3) {
                sm = sm + psi[oth - g.P];
                sm = sm + psi[oth + g.P];
            }
            const double fc = f[s];
            int nb = 0;
            if (CL) {
                const int64_t gk = g.z0 + k;
                nb = (i == 0) + (i == g.nx - 1) + (j == 0) + (j == g.ny - 1) +
                     (DIM == 3 ? (gk == 0) + (gk == g.gnz - 1) : 0);
            }
            const double r = op.residual(sm, fc, psi[s], nb);
            out = (float)r;
            rr = __builtin_fma(r, r, rr);
            ff = __builtin_fma(fc, fc, ff);
        }
        r32[s] = out;
        if (ZERO) u32[s] = 0.0f;
    }
    block_pair(rr, ff, partials, fofs);
}

// psi += (double)e over n packed slots (n even, both arrays 16- / 8-byte aligned), two slots per access, two
// accesses in flight per thread; slots that hold no cell carry e = 0
__global__ __launch_bounds__(kBlock) void k_refine_add(double* __restrict__ psi, const float* __restrict__ e32,
                                                       int64_t pairs, double* __restrict__ partials)
{
    const int64_t step = (int64_t)gridDim.x * kBlock;
    double ee = 0.0;
    for (int64_t p0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; p0 < pairs; p0 += 2 * step) {
        const int64_t p1 = p0 + step;
        const bool two = p1 < pairs;
        V2 a = vload<double, 2>(psi + 2 * p0), c = vzero<double, 2>();
        const F2 ea = vload<float, 2>(e32 + 2 * p0);
        F2 ec = vzero<float, 2>();
        if (two) {
            c = vload<double, 2>(psi + 2 * p1);
            ec = vload<float, 2>(e32 + 2 * p1);
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double da = (double)ea.v[e], dc = (double)ec.v[e];
            a.v[e] = a.v[e] + da;
            c.v[e] = c.v[e] + dc;
            ee = __builtin_fma(da, da, ee);
            ee = __builtin_fma(dc, dc, ee);
        }
        vstore<double, 2>(psi + 2 * p0, a);
        if (two) vstore<double, 2>(psi + 2 * p1, c);
    }
    block_pair(ee, 0.0, partials, 0);
}

// exact widening / round-to-nearest narrowing of n packed slots (mgp_refine_begin / mgp_refine_end)
__global__ __launch_bounds__(kBlock) void k_widen(const float* __restrict__ src, double* __restrict__ dst, int64_t n)
{
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock)
        dst[s] = (double)src[s];
}
__global__ __launch_bounds__(kBlock) void k_narrow(const double* __restrict__ src, float* __restrict__ dst, int64_t n)
{
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock)
        dst[s] = (float)src[s];
}

bool defect_vector(const Geo& g) { return g.hw >= 2; }
int64_t defect_items(const Geo& g) { return (g.H / 2) * 2 * g.nz; }
bool defect_gs(const Geo& g) { return defect_vector(g) && defect_items(g) >= (int64_t)kDefectGsBlocks * kBlock * 2; }

template <int DIM, bool ZERO, bool CL>
void defect_t(const double* psi, const double* f, float* r32, float* u32, Geo g, double h, double cl, double* partials,
              hipStream_t s)
{
    const Op<double, DIM> op = make_op<double, DIM>(h, cl);
    const int fofs = kDefectMaxBlocks;
    if (defect_gs(g)) {
        k_defect_gs<DIM, ZERO, CL><<<kDefectGsBlocks, kBlock, 0, s>>>(psi, f, r32, u32, g, op, defect_items(g), partials, fofs);
    } else if (defect_vector(g)) {
        const int64_t items = defect_items(g);
        k_defect<DIM, ZERO, CL><<<nblk(items), kBlock, 0, s>>>(psi, f, r32, u32, g, op, items, partials, fofs);
    } else {
        k_defect_s<DIM, ZERO, CL><<<(unsigned)defect_blocks(g), kBlock, 0, s>>>(psi, f, r32, u32, g, op, partials, fofs);
    }
}

}  // namespace

int defect_blocks(Geo g)
{
    if (defect_gs(g)) return kDefectGsBlocks;
    if (defect_vector(g)) return (int)nblk(defect_items(g));  // < 2 * kDefectGsBlocks
    return (int)std::min<int64_t>(kDefectMaxBlocks, std::max<int64_t>(1, nblk(g.P * g.nz)));
}

int refine_add_blocks(Geo g)
{
    const int64_t pairs = g.P * g.nz / 2;
    return (int)std::min<int64_t>(kAddMaxBlocks, std::max<int64_t>(1, (pairs + 2 * kBlock - 1) / (2 * kBlock)));
}

int refine_partials() { return std::max(2 * kDefectMaxBlocks, kAddMaxBlocks); }

template <int DIM, bool CL>
static void defect_d(const double* psi64, const double* f64, float* r32, float* u32_or_null, Geo g, double h, double cl,
                     double* partials, hipStream_t s)
{
    if (u32_or_null) defect_t<DIM, true, CL>(psi64, f64, r32, u32_or_null, g, h, cl, partials, s);
    else defect_t<DIM, false, CL>(psi64, f64, r32, nullptr, g, h, cl, partials, s);
}

hipError_t launch_defect(int dim, const double* psi64, const double* f64, float* r32, float* u32_or_null, Geo g,
                         double h, double cl, double* partials, double* out, hipStream_t s)
{
    if (dim == 3) {
        if (cl == 0.0) defect_d<3, false>(psi64, f64, r32, u32_or_null, g, h, cl, partials, s);
        else defect_d<3, true>(psi64, f64, r32, u32_or_null, g, h, cl, partials, s);
    } else {
        if (cl == 0.0) defect_d<2, false>(psi64, f64, r32, u32_or_null, g, h, cl, partials, s);
        else defect_d<2, true>(psi64, f64, r32, u32_or_null, g, h, cl, partials, s);
    }
    const int nb = defect_blocks(g);
    (void)launch_sum_partials(partials, nb, out, s);
    (void)launch_sum_partials(partials + kDefectMaxBlocks, nb, out + 1, s);
    return hipGetLastError();
}

hipError_t launch_refine_add(double* psi64, const float* e32, Geo g, double* partials, double* out, hipStream_t s)
{
    const int nb = refine_add_blocks(g);
    k_refine_add<<<nb, kBlock, 0, s>>>(psi64, e32, g.P * g.nz / 2, partials);
    (void)launch_sum_partials(partials, nb, out, s);
    return hipGetLastError();
}

hipError_t launch_refine_widen(const float* src, double* dst, int64_t n, hipStream_t s)
{
    k_widen<<<(unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, nblk(n))), kBlock, 0, s>>>(src, dst, n);
    return hipGetLastError();
}

hipError_t launch_refine_narrow(const double* src, float* dst, int64_t n, hipStream_t s)
{
    k_narrow<<<(unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, nblk(n))), kBlock, 0, s>>>(src, dst, n);
    return hipGetLastError();
}

}  // namespace mgp
