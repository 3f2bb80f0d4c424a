// mgp_kernels.hip — CDNA4 (gfx950) kernels of the multigrid cycle on the red/black packed layout
// (see Geo in mgp_internal.h).
//
// One kernel per piece of the reference's twoGrid (cpu-raw.lua:186-237, gpu.lua:83-200),
// re-cut for HBM traffic:
//   k_half            one colour of a red/black sweep (build-defined smoother; the deterministic
//                     replacement of the racy gpu.lua:61-81 GaussSeidel kernel).  Run on both
//                     colours out of place it is the reference Jacobi sweep (gpu.lua:83-102) without
//                     the enqueueCopyBuffer of gpu.lua:292.  Per cell it moves 1.5 reals (read the
//                     other colour, read f, write this colour): 3 reals per full sweep.
//   k_resrestrict     calcResidual + reduceResidual fused (gpu.lua:104-137): the fine residual
//                     never reaches HBM.
//   k_prolong         expandResidual + addTo fused (gpu.lua:139-171); injection or (tri)linear.
//   k_sqdiff / k_sum  calcFrobErr + the host sum of gpu.lua:189-200, 361-369 as a deterministic
//                     two-pass fp64 reduction on the device (also fused into the last half-sweep).
//
// Arithmetic follows the reference operation by operation: neighbour sum ((xl+xr)+yl)+yr[+zl+zr],
// askew = sum/h^2, (f - askew)/adiag, r = f - (askew + adiag*u), 1/4 (r00+r10+r01+r11) and
// 1/8 of the 8 children in x-fastest order.  The library is compiled with -ffp-contract=off.
// Two rewrites are exact: x / h^2 == x * 2^(2k) (h is a power of two), and the division by the
// interior diagonal uses y = RN(1/adiag) plus one FMA correction (q = RN(a y),
// q' = RN(q + RN(a - q d) y)), which equals the IEEE quotient for operands away from
// over/underflow (Markstein); boundary cells with a modified diagonal divide directly.  The GPU
// parity tests check every piece bit for bit against the C oracle's plain divisions.
//
// The other engines live in units of their own: k_zs and the fused phases' planning and dispatch (mgp_zs.h,
// mgp_zs.hip), the coarse tail (mgp_tail.hip), the tiled phases (mgp_blk.hip), the lexicographic sweep
// (mgp_gslex.hip).  Still here, built on mgp_zs.h's helpers: k_zs's stage-split variants and the 2D k_ys.
#include "mgp_cell.h"
#include "mgp_zs.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace mgp {
namespace {

// (kBlock, vectors, div_rn, Op, pidx, xcd_remap, block_partial, fw_axis, kMaxBlocks / nblk_gs: mgp_device.h)

// ---- init / pack / unpack -------------------------------------------------------------------

// (slot_cell: mgp_device.h)

template <typename T>
__global__ __launch_bounds__(kBlock) void k_init(T* __restrict__ u, T* __restrict__ f, Geo g, int64_t cx, int64_t cy,
                                                 int64_t cz, int dim3)
{
    const int64_t n = g.P * g.nz;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        int i, j;
        int64_t k;
        const bool cell = slot_cell(s, g, i, j, k);
        const double charge = 1e+6, epsilon0 = 1;
        const bool hit = cell && i == cx && j == cy && (!dim3 || g.z0 + k == cz);
        const T v = hit ? (T)(-charge / epsilon0) : (T)0;
        f[s] = v;
        u[s] = -v;  // psi = -f (cpu.lua:193): -0.0 off the charge, as in the oracle
    }
}

// lex: planes 0 .. g.nz-1 of the (sub)slab described by g (g.z0 = global index of its plane 0)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pack(const T* __restrict__ lex, T* __restrict__ out, Geo g)
{
    const int64_t n = g.P * g.nz;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        int i, j;
        int64_t k;
        out[s] = slot_cell(s, g, i, j, k) ? lex[(k * g.ny + j) * (int64_t)g.nx + i] : (T)0;
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_unpack(const T* __restrict__ in, T* __restrict__ lex, Geo g)
{
    const int64_t n = g.P * g.nz;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        int i, j;
        int64_t k;
        if (slot_cell(s, g, i, j, k)) lex[(k * g.ny + j) * (int64_t)g.nx + i] = in[s];
    }
}

// Order-independent fingerprint of a field (mgp_field_stats): per cell a 64-bit mix of its bit
// pattern and its global lexicographic index, summed modulo 2^64, so two fields have the same
// hash exactly when (with overwhelming probability) every cell is bit-identical, whatever the
// slab decomposition or reduction order.  Alongside: fp64 sum, sum of squares and max |x|.
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

template <typename T>
__device__ __forceinline__ uint64_t real_bits(T v)
{
    if constexpr (sizeof(T) == 8) {
        uint64_t b;
        __builtin_memcpy(&b, &v, 8);
        return b;
    } else {
        uint32_t b;
        __builtin_memcpy(&b, &v, 4);
        return b;
    }
}

// PAD: the plane stride is not 2 H (level_slot, mgp_device.h)
template <typename T, bool PAD = false>
__global__ __launch_bounds__(kBlock) void k_field_stats(const T* __restrict__ in, Geo g, uint64_t* __restrict__ hpart,
                                                        double* __restrict__ dpart)
{
    const int64_t n = (PAD ? 2 * g.H : g.P) * g.nz;
    uint64_t h = 0;
    double s = 0.0, q = 0.0, mx = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n; c += (int64_t)gridDim.x * kBlock) {
        const int64_t x = PAD ? level_slot(c, g.lhw + g.ly + 1, g.P) : c;
        int i, j;
        int64_t k;
        if (!slot_cell(x, g, i, j, k)) continue;
        const T v = in[x];
        const uint64_t gi = ((uint64_t)(g.z0 + k) * (uint64_t)g.ny + (uint64_t)j) * (uint64_t)g.nx + (uint64_t)i;
        h += mix64(real_bits(v) ^ mix64(gi));
        const double d = (double)v;
        s += d;
        q += d * d;
        mx = fmax(mx, fabs(d));
    }
    __shared__ uint64_t sh[kBlock];
    __shared__ double sd[3][kBlock];
    sh[threadIdx.x] = h;
    sd[0][threadIdx.x] = s;
    sd[1][threadIdx.x] = q;
    sd[2][threadIdx.x] = mx;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[threadIdx.x] += sh[threadIdx.x + w];
            sd[0][threadIdx.x] += sd[0][threadIdx.x + w];
            sd[1][threadIdx.x] += sd[1][threadIdx.x + w];
            sd[2][threadIdx.x] = fmax(sd[2][threadIdx.x], sd[2][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        hpart[blockIdx.x] = sh[0];
        for (int c = 0; c < 3; ++c) dpart[c * gridDim.x + blockIdx.x] = sd[c][0];
    }
}

// one workgroup: the nb partials of k_field_stats -> out_h[0], out_d[0..2]
__global__ __launch_bounds__(kBlock) void k_field_stats_final(const uint64_t* __restrict__ hpart,
                                                              const double* __restrict__ dpart, int nb,
                                                              uint64_t* __restrict__ out_h, double* __restrict__ out_d)
{
    uint64_t h = 0;
    double s = 0.0, q = 0.0, mx = 0.0;
    for (int b = threadIdx.x; b < nb; b += kBlock) {
        h += hpart[b];
        s += dpart[b];
        q += dpart[nb + b];
        mx = fmax(mx, dpart[2 * nb + b]);
    }
    __shared__ uint64_t sh[kBlock];
    __shared__ double sd[3][kBlock];
    sh[threadIdx.x] = h;
    sd[0][threadIdx.x] = s;
    sd[1][threadIdx.x] = q;
    sd[2][threadIdx.x] = mx;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[threadIdx.x] += sh[threadIdx.x + w];
            sd[0][threadIdx.x] += sd[0][threadIdx.x + w];
            sd[1][threadIdx.x] += sd[1][threadIdx.x + w];
            sd[2][threadIdx.x] = fmax(sd[2][threadIdx.x], sd[2][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out_h[0] = sh[0];
        out_d[0] = sd[0][0];
        out_d[1] = sd[1][0];
        out_d[2] = sd[2][0];
    }
}

// ---- red/black half-sweep -------------------------------------------------------------------

// Vector form: a thread owns N consecutive cells of colour `color` in one row (hw % N == 0).
// half_load gathers an item's operands (all loads issued), half_store computes and stores it, so
// a thread can keep several items' loads in flight.
template <typename T, int N>
struct HalfIn {
    Vec<T, N> cen, yl, yr, zl, zr, fv;
    T edge;
    int64_t own;
    int o, j, nbyz, m0;
    int64_t gk;
};

template <typename T, int DIM, bool NT = false>
__device__ __forceinline__ void half_load(HalfIn<T, VN<T>::n>& in, const T* __restrict__ other, const T* __restrict__ f,
                                          const Geo& g, int color, int64_t it)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int lgpr = g.lhw - LN;  // log2 groups per row
    const int grp = (int)(it & ((1 << lgpr) - 1));
    const int j = (int)((it >> lgpr) & (g.ny - 1));
    const int64_t k = it >> (lgpr + g.ly);
    const int m0 = grp * N;
    const int64_t gk = g.z0 + k;
    const int o = color ^ (int)((j + gk) & 1);  // x parity of this row's colour-c cells
    const int64_t own = k * g.P + color * g.H + (int64_t)j * g.hw + m0;
    const int64_t oth = k * g.P + (color ^ 1) * g.H + (int64_t)j * g.hw + m0;
    in.cen = vload<T, N>(other + oth);
    if (o == 0)
        in.edge = m0 > 0 ? other[oth - 1] : (T)0;      // x-1 of the first cell
    else
        in.edge = m0 + N < g.hw ? other[oth + N] : (T)0;  // x+1 of the last cell
    in.yl = j > 0 ? vload<T, N>(other + oth - g.hw) : vzero<T, N>();
    in.yr = j < g.ny - 1 ? vload<T, N>(other + oth + g.hw) : vzero<T, N>();
    if (DIM == 3) {
        in.zl = vload<T, N>(other + oth - g.P);
        in.zr = vload<T, N>(other + oth + g.P);
    }
    in.fv = NT ? vload_nt<T, N>(f + own) : vload<T, N>(f + own);
    in.own = own;
    in.o = o;
    in.j = j;
    in.m0 = m0;
    in.gk = gk;
    in.nbyz = (j == 0) + (j == g.ny - 1) + (DIM == 3 ? (gk == 0) + (gk == g.gnz - 1) : 0);
}

template <typename T, int DIM, bool ERR, bool NT = false>
__device__ __forceinline__ void half_store(const HalfIn<T, VN<T>::n>& in, T* __restrict__ dst, const T* __restrict__ old,
                                           const Geo& g, const Op<T, DIM>& op, double& acc)
{
    constexpr int N = VN<T>::n;
    const int o = in.o;
    T d0, y0, d1, y1;
    row_diag_fast(op, in.nbyz, d0, y0, d1, y1);
    Vec<T, N> out;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int i = 2 * (in.m0 + e) + o;
        const T xl = o == 0 ? (e == 0 ? in.edge : in.cen.v[e - 1]) : in.cen.v[e];
        const T xr = o == 0 ? in.cen.v[e] : (e == N - 1 ? in.edge : in.cen.v[e + 1]);
        T s = xl + xr;
        s = s + in.yl.v[e];
        s = s + in.yr.v[e];
        if (DIM == 3) {
            s = s + in.zl.v[e];
            s = s + in.zr.v[e];
        }
        const bool xf = i == 0 || i == g.nx - 1;
        out.v[e] = div_rn(in.fv.v[e] - s * op.inv_hSq, xf ? d1 : d0, xf ? y1 : y0);  // op.relax(s, f, nbyz + xf)
    }
    if (NT)
        vstore_nt<T, N>(dst + in.own, out);
    else
        vstore<T, N>(dst + in.own, out);
    if (ERR) {
        const Vec<T, N> w = NT ? vload_nt<T, N>(old + in.own) : vload<T, N>(old + in.own);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const double d = (double)out.v[e] - (double)w.v[e];
            acc += d * d;
        }
    }
}

template <typename T, int DIM, int TAG, bool ERR>
__global__ __launch_bounds__(kBlock) void k_half(const T* __restrict__ other, const T* __restrict__ f,
                                                 T* __restrict__ dst, const T* __restrict__ old,
                                                 double* __restrict__ partials, Geo g, int color,
                                                 Op<T, DIM> op)
{
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    double acc = 0.0;
    if ((it >> (g.lhw - (VN<T>::n == 4 ? 2 : 1) + g.ly)) < g.nz) {
        HalfIn<T, VN<T>::n> in;
        half_load<T, DIM, TAG == 2>(in, other, f, g, color, it);
        half_store<T, DIM, ERR, TAG == 2>(in, dst, old, g, op, acc);
    }
    if (ERR) block_partial<T>(acc, partials);
}

// Grid-stride form for large levels (kGsBlocks workgroups): the workgroups of XCD x (b % 8 == x)
// sweep the contiguous band x of the items, so y/z neighbours meet in that XCD's L2, and each
// thread keeps two items' loads in flight.
constexpr int kGsBlocks = 2048;

template <typename T, int DIM, int TAG, bool ERR>
__global__ __launch_bounds__(kBlock) void k_half_gs(const T* __restrict__ other, const T* __restrict__ f,
                                                    T* __restrict__ dst, const T* __restrict__ old,
                                                    double* __restrict__ partials, Geo g, int color,
                                                    Op<T, DIM> op, int64_t items)
{
    const int nlb = gridDim.x >> 3;
    const int64_t band = (items + 7) >> 3;
    const int64_t base = (int64_t)(blockIdx.x & 7) * band;
    const int64_t end = base + band < items ? base + band : items;
    const int64_t step = (int64_t)nlb * kBlock;
    double acc = 0.0;
    for (int64_t i0 = base + (int64_t)(blockIdx.x >> 3) * kBlock + threadIdx.x; i0 < end; i0 += 2 * step) {
        const int64_t i1 = i0 + step;
        HalfIn<T, VN<T>::n> a, c;
        half_load<T, DIM>(a, other, f, g, color, i0);
        if (i1 < end) half_load<T, DIM>(c, other, f, g, color, i1);
        half_store<T, DIM, ERR>(a, dst, old, g, op, acc);
        if (i1 < end) half_store<T, DIM, ERR>(c, dst, old, g, op, acc);
    }
    if (ERR) block_partial<T>(acc, partials);
}

// (half_item: mgp_cell.h)

// Scalar form for small levels (hw < N, nx = 1 included) and for the cpu-raw float arithmetic
// (C = double, every level): a thread per colour-c slot.
template <typename T, int DIM, bool ERR, typename C = T>
__global__ __launch_bounds__(kBlock) void k_half_s(const T* __restrict__ other, const T* __restrict__ f,
                                                   T* __restrict__ dst, const T* __restrict__ old,
                                                   double* __restrict__ partials, Geo g, int color,
                                                   Op<C, DIM> op)
{
    const int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double acc = 0.0;
    if (it < g.H * g.nz) {
        T v;
        const int64_t own = half_item<T, DIM, C>(other, f, dst, g, color, op, it, &v);
        if (ERR && own >= 0) {
            const double d = (double)v - (double)old[own];
            acc += d * d;
        }
    }
    if (ERR) block_partial<T>(acc, partials);
}

// First RB-GS sweep from a fresh zero guess (cpu.lua:138), both colours in one pass over f.
// With u = 0 the red half-sweep's neighbour sum is +0, so red = relax(0, f_red, nb): a pointwise
// function of f.  The black half-sweep then needs the red values of its six neighbours, which
// this thread recomputes from f (red rows j-1, j, j+1 and planes k-1, k+1 of its N-cell segment,
// plus one edge cell) with the same expression, so u after the sweep is bit-identical to the two
// half-sweeps reading a zero black input.  A thread owns the N red and N black cells at half
// positions m0 .. m0+N-1 of one row.  HBM: read f, write u (the per-piece pair also reads the
// zero input and re-reads the red cells).
// RED = false: the red cells are not stored (a later sweep's red half-sweep replaces them unread)
template <typename T, int DIM, bool RED = true>
__global__ __launch_bounds__(kBlock) void k_fresh(const T* __restrict__ f, T* __restrict__ u, Geo g, Op<T, DIM> op)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int lgpr = g.lhw - LN;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    const int grp = (int)(it & ((1 << lgpr) - 1));
    const int j = (int)((it >> lgpr) & (g.ny - 1));
    const int64_t k = it >> (lgpr + g.ly);
    if (k >= g.nz) return;
    const int m0 = grp * N;
    const int64_t gk = g.z0 + k;
    const int ob = 1 ^ (int)((j + gk) & 1);  // x parity of this row's black cells (red: ob ^ 1)
    // A row's diagonals are looked up once per row (Op::row_diag), so a cell's relax is div_rn with a select
    // between two of them.  relax(+0, f, nb) = div_rn(f - (+0), ..) = div_rn(f, ..) exactly (f - (+0) == f).
    struct RowDiag {
        T d0, y0, d1, y1;
    };
    auto row_diag = [&](int nbyz) {
        RowDiag r;
        row_diag_fast(op, nbyz, r.d0, r.y0, r.d1, r.y1);  // five rows per thread
        return r;
    };
    // Every load is issued before any arithmetic (round 4: with a load per red-row evaluation behind its box
    // test, each thread waited for five memory latencies one after another; 256^3 31.8 us)
    const int64_t own = k * g.P + (int64_t)j * g.hw + m0;
    const bool vyl = j > 0, vyr = j < g.ny - 1;
    const bool vzl = DIM == 3 && gk > 0, vzr = DIM == 3 && gk < g.gnz - 1;
    const Vec<T, N> fc = vload<T, N>(f + own);  // red half of the row (colour 0)
    const Vec<T, N> fyl = vload<T, N>(f + own - (vyl ? g.hw : 0));
    const Vec<T, N> fyr = vload<T, N>(f + own + (vyr ? g.hw : 0));
    Vec<T, N> fzl = fc, fzr = fc;
    if (DIM == 3) {
        fzl = vload<T, N>(f + own - (vzl ? g.P : 0));
        fzr = vload<T, N>(f + own + (vzr ? g.P : 0));
    }
    // the red x-neighbour outside the segment: m0 - 1 (black cells at even x) or m0 + N (odd x)
    const int me = ob == 0 ? m0 - 1 : m0 + N;
    const bool ve = me >= 0 && me < g.hw;
    const T fe = f[own + (ve ? me - m0 : 0)];
    const Vec<T, N> fb = vload<T, N>(f + own + g.H);
    // red values of row (jj, gkk) at m0 .. m0+N-1 from its f (0 outside the box)
    auto red_row = [&](const Vec<T, N>& fv, bool valid, int jj, int64_t gkk, Vec<T, N>& r) {
        if (!valid) {
            r = vzero<T, N>();
            return;
        }
        const int orr = (int)((jj + gkk) & 1);  // x parity of red cells in that row
        const int nbyz = (jj == 0) + (jj == g.ny - 1) + (DIM == 3 ? (gkk == 0) + (gkk == g.gnz - 1) : 0);
        const RowDiag rd = row_diag(nbyz);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int i = 2 * (m0 + e) + orr;
            const bool xf = i == 0 || i == g.nx - 1;
            r.v[e] = div_rn(fv.v[e], xf ? rd.d1 : rd.d0, xf ? rd.y1 : rd.y0);
        }
    };
    Vec<T, N> rc, ryl, ryr, rzl, rzr;
    red_row(fc, true, j, gk, rc);
    red_row(fyl, vyl, j - 1, gk, ryl);
    red_row(fyr, vyr, j + 1, gk, ryr);
    if (DIM == 3) {
        red_row(fzl, vzl, j, gk - 1, rzl);
        red_row(fzr, vzr, j, gk + 1, rzr);
    }
    const int nbyz = (j == 0) + (j == g.ny - 1) + (DIM == 3 ? (gk == 0) + (gk == g.gnz - 1) : 0);
    T edge = (T)0;
    if (ve) {
        const int i = 2 * me + (ob ^ 1);
        edge = op.relax((T)0, fe, nbyz + (i == 0) + (i == g.nx - 1));
    }
    const RowDiag bd = row_diag(nbyz);
    Vec<T, N> out;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int i = 2 * (m0 + e) + ob;
        const T xl = ob == 0 ? (e == 0 ? edge : rc.v[e - 1]) : rc.v[e];
        const T xr = ob == 0 ? rc.v[e] : (e == N - 1 ? edge : rc.v[e + 1]);
        T s = xl + xr;
        s = s + ryl.v[e];
        s = s + ryr.v[e];
        if (DIM == 3) {
            s = s + rzl.v[e];
            s = s + rzr.v[e];
        }
        const bool xf = i == 0 || i == g.nx - 1;
        out.v[e] = div_rn(fb.v[e] - s * op.inv_hSq, xf ? bd.d1 : bd.d0, xf ? bd.y1 : bd.y0);  // Op::relax
    }
    if (RED) vstore<T, N>(u + own, rc);
    vstore<T, N>(u + own + g.H, out);
}

// ---- fused residual + restriction -----------------------------------------------------------

// (residual_at, resrestrict_item, resrestrict_items: mgp_cell.h)

// ---- residual norm (north star: wavefront-level reductions for the residual norm) -------------

// (wave_sum: mgp_device.h)

// sum (f - A u)^2 and sum f^2 over both colours of a level (calcResidual, cpu.lua:108-123, squared
// and reduced on the device instead of materialising r).  Vector form: a thread owns N cells of one
// colour in one row (k_half's item; colour = the item's half of the grid), loads the other colour's
// neighbours with half_load and its own cells with one vector load.  Per wave a butterfly sum, per
// workgroup the 4 wave sums in fixed order, one fp64 pair per workgroup into partials[b] and
// partials[fofs + b] (fofs leaves room for the first row's sum_partials scratch).
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_resnorm(const T* __restrict__ u, const T* __restrict__ f, Geo g,
                                                    Op<T, DIM> op, int64_t items, double* __restrict__ partials,
                                                    int fofs)
{
    constexpr int N = VN<T>::n;
    const int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double rr = 0.0, ff = 0.0;
    if (it < 2 * items) {
        const int color = it >= items;
        HalfIn<T, N> in;
        half_load<T, DIM>(in, u, f, g, color, it - color * items);
        const Vec<T, N> uc = vload<T, N>(u + in.own);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int o = in.o;
            const int i = 2 * (in.m0 + e) + o;
            const T xl = o == 0 ? (e == 0 ? in.edge : in.cen.v[e - 1]) : in.cen.v[e];
            const T xr = o == 0 ? in.cen.v[e] : (e == N - 1 ? in.edge : in.cen.v[e + 1]);
            T sm = xl + xr;
            sm = sm + in.yl.v[e];
            sm = sm + in.yr.v[e];
            if (DIM == 3) {
                sm = sm + in.zl.v[e];
                sm = sm + in.zr.v[e];
            }
            const T r = op.residual(sm, in.fv.v[e], uc.v[e], in.nbyz + (i == 0) + (i == g.nx - 1));
            rr = __builtin_fma((double)r, (double)r, rr);
            ff = __builtin_fma((double)in.fv.v[e], (double)in.fv.v[e], ff);
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
        for (int k = 0; k < kBlock / 64; ++k) {
            a += ws[0][k];
            b += ws[1][k];
        }
        partials[blockIdx.x] = a;
        partials[fofs + blockIdx.x] = b;
    }
}

// 3D levels streamed through z: a thread owns N cells of each colour in one row (j, packed m0 .. m0 + N - 1)
// and walks kResZ planes, holding both colours of the row in planes k - 1, k, k + 1 in registers, so each
// plane of u and f is read once (rows j +- 1 come from L2, where the neighbouring rows' threads read them as
// their own).  The per-cell expressions are k_resnorm's; only the partial sums' grouping differs.
constexpr int kResZ = 16;
template <typename T>
__global__ __launch_bounds__(kBlock) void k_resnorm_z(const T* __restrict__ u, const T* __restrict__ f, Geo g,
                                                      Op<T, 3> op, double* __restrict__ partials, int fofs)
{
    constexpr int N = VN<T>::n;
    const int groups = g.hw / N;
    const int64_t cols = (int64_t)groups * g.ny;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double rr = 0.0, ff = 0.0;
    if (t < cols * (g.nz / kResZ)) {
        const int64_t col = t % cols;
        const int64_t k0 = (t / cols) * kResZ;
        const int grp = (int)(col % groups), j = (int)(col / groups), m0 = grp * N;
        const int64_t roff = (int64_t)j * g.hw + m0;
        Vec<T, N> A[2], B[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            A[c] = vload<T, N>(u + (k0 - 1) * g.P + c * g.H + roff);  // a ghost plane at the slab's ends
            B[c] = vload<T, N>(u + k0 * g.P + c * g.H + roff);
        }
        for (int64_t k = k0; k < k0 + kResZ; ++k) {
            const int64_t gk = g.z0 + k;
            const T* const pk = u + k * g.P + roff;
            Vec<T, N> C[2], YL[2], YR[2], F[2];
            T edge[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                C[c] = vload<T, N>(pk + g.P + c * g.H);
                YL[c] = j > 0 ? vload<T, N>(pk + c * g.H - g.hw) : vzero<T, N>();
                YR[c] = j < g.ny - 1 ? vload<T, N>(pk + c * g.H + g.hw) : vzero<T, N>();
                F[c] = vload<T, N>(f + k * g.P + c * g.H + roff);
                // x edge of colour c's cells, from the other colour's row: x - 1 of the first cell (x parity 0)
                // or x + 1 of the last (parity 1)
                const int o = c ^ (int)((j + gk) & 1);
                const T* const oth = pk + (c ^ 1) * g.H;
                if (o == 0)
                    edge[c] = m0 > 0 ? oth[-1] : (T)0;
                else
                    edge[c] = m0 + N < g.hw ? oth[N] : (T)0;
            }
            const int nbyz = (j == 0) + (j == g.ny - 1) + (gk == 0) + (gk == g.gnz - 1);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int oc = c ^ 1, o = c ^ (int)((j + gk) & 1);
                const Vec<T, N>& cen = B[oc];
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const int i = 2 * (m0 + e) + o;
                    const T xl = o == 0 ? (e == 0 ? edge[c] : cen.v[e - 1]) : cen.v[e];
                    const T xr = o == 0 ? cen.v[e] : (e == N - 1 ? edge[c] : cen.v[e + 1]);
                    T sm = xl + xr;
                    sm = sm + YL[oc].v[e];
                    sm = sm + YR[oc].v[e];
                    sm = sm + A[oc].v[e];
                    sm = sm + C[oc].v[e];
                    const T r = op.residual(sm, F[c].v[e], B[c].v[e], nbyz + (i == 0) + (i == g.nx - 1));
                    rr = __builtin_fma((double)r, (double)r, rr);
                    ff = __builtin_fma((double)F[c].v[e], (double)F[c].v[e], ff);
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                A[c] = B[c];
                B[c] = C[c];
            }
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

// Scalar form for small levels (hw < N, nx = 1 included), and for the cpu-raw float arithmetic (C = double:
// r evaluated in double and rounded to the real type, as rs[L] would hold it): a thread per packed slot.
template <typename T, int DIM, typename C = T>
__global__ __launch_bounds__(kBlock) void k_resnorm_s(const T* __restrict__ u, const T* __restrict__ f, Geo g,
                                                      Op<C, DIM> op, double* __restrict__ partials, int fofs)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double rr = 0.0, ff = 0.0;
    if (s < g.P * g.nz) {
        int i, j;
        int64_t k;
        if (slot_cell(s, g, i, j, k)) {
            const T r = (T)residual_at<T, DIM, C>(u, f, g, op, i, j, k);
            rr = (double)r * (double)r;
            ff = (double)f[s] * (double)f[s];
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
        for (int k = 0; k < kBlock / 64; ++k) {
            a += ws[0][k];
            b += ws[1][k];
        }
        partials[blockIdx.x] = a;
        partials[fofs + blockIdx.x] = b;
    }
}

// rs[L] of cpu-raw.lua:155-171 (calcResidual, cpu.lua:108-123) materialised on request (mgp_get_field
// MGP_FIELD_RESIDUAL): r at every packed slot, grid-stride.
template <typename T, int DIM, typename C = T>
__global__ __launch_bounds__(kBlock) void k_residual_field(const T* __restrict__ u, const T* __restrict__ f,
                                                           T* __restrict__ r, Geo g, Op<C, DIM> op)
{
    const int64_t n = g.P * g.nz;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        int i, j;
        int64_t k;
        r[s] = slot_cell(s, g, i, j, k) ? (T)residual_at<T, DIM, C>(u, f, g, op, i, j, k) : (T)0;
    }
}

// errorBuf of cpu-raw.lua:96-100 / gpu.lua:189-200 (calcFrobErr): (psi - psiOld)^2 per cell, evaluated in C
// (gpu.lua: real; cpu-raw.lua: LuaJIT double) and stored in real.
template <typename T, typename C = T>
__global__ __launch_bounds__(kBlock) void k_sqdiff_field(const T* __restrict__ a, const T* __restrict__ b,
                                                         T* __restrict__ out, int64_t n)
{
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock) {
        const C d = (C)a[s] - (C)b[s];
        out[s] = (T)(d * d);
    }
}

// Scalar form: a thread per coarse cell (any sizes; every level under the cpu-raw float arithmetic).
template <typename T, int DIM, typename C = T>
__global__ __launch_bounds__(kBlock) void k_resrestrict_s(const T* __restrict__ u, const T* __restrict__ f,
                                                          T* __restrict__ R, Geo g, Geo gc, Op<C, DIM> op)
{
    const int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (it >= resrestrict_items<T, DIM>(g)) return;
    resrestrict_item<T, DIM, C>(u, f, R, g, gc, op, it);
}

// Vector form: a thread owns N consecutive coarse cells I0 .. I0+N-1 of one coarse row.  Their
// fine children are, in every fine row, the N cells m = I0 .. of BOTH colours.  The thread loads
// each fine (plane, row, colour) vector it needs exactly once into registers — planes 2K, 2K+1
// with rows 2J-1 .. 2J+2, planes 2K-1, 2K+2 with rows 2J, 2J+1 — and keeps the reference order
//   R = 1/8 (((((((r000 + r100) + r010) + r110) + r001) + r101) + r011) + r111).
// NV: coarse cells per thread (default: one 16-byte vector; 2 gives mid-size levels more threads)
template <typename T, int DIM, int NV = VN<T>::n>
__global__ __launch_bounds__(kBlock) void k_resrestrict(const T* __restrict__ u, const T* __restrict__ f,
                                                        T* __restrict__ R, Geo g, Geo gc, Op<T, DIM> op)
{
    constexpr int N = NV;
    constexpr int LN = N == 4 ? 2 : (N == 2 ? 1 : 0);
    constexpr int NZ = DIM == 3 ? 2 : 1;  // fine planes per coarse plane
    const int cy = g.ny >> 1;
    const int lgpr = (g.lx - 1) - LN;  // log2 groups of N per coarse row
    const int64_t ncz = DIM == 3 ? (g.nz >> 1) : 1;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    const int grp = (int)(it & ((1 << lgpr) - 1));
    const int J = (int)((it >> lgpr) & (cy - 1));
    const int64_t K = it >> (lgpr + g.ly - 1);
    if (K >= ncz) return;
    const int m0 = grp * N;
    const int j0 = 2 * J;
    const int64_t k0 = DIM == 3 ? 2 * K : 0;

    const bool xlo = m0 == 0, xhi = m0 + N == g.hw;
    auto row = [&](int64_t k, int j, int c) {
        return (j >= 0 && j < g.ny) ? vload<T, N>(u + k * g.P + c * g.H + (int64_t)j * g.hw + m0) : vzero<T, N>();
    };
    // running sum in the reference order: the children of fine plane 2K, then of 2K+1
    T acc[N];
#pragma unroll
    for (int dz = 0; dz < NZ; ++dz) {
        const int64_t k = k0 + dz;
        const int64_t gk = g.z0 + k;
        // this plane's rows j0-1 .. j0+2 (both colours) and, in 3D, rows j0, j0+1 of planes k-1, k+1
        Vec<T, N> M[4][2], Z[2][2][2];
#pragma unroll
        for (int yi = 0; yi < 4; ++yi)
#pragma unroll
            for (int c = 0; c < 2; ++c) M[yi][c] = row(k, j0 - 1 + yi, c);
        if (DIM == 3) {
#pragma unroll
            for (int zz = 0; zz < 2; ++zz)
#pragma unroll
                for (int yi = 0; yi < 2; ++yi)
#pragma unroll
                    for (int c = 0; c < 2; ++c) Z[zz][yi][c] = row(k - 1 + 2 * zz, j0 + yi, c);
        }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int j = j0 + dy;
            const int p = (int)((j + gk) & 1);
            const int nbyz = (j == 0) + (j == g.ny - 1) + (DIM == 3 ? (gk == 0) + (gk == g.gnz - 1) : 0);
            const bool fast = op.cl == (T)0 || (nbyz == 0 && !xlo && !xhi);
            T rr[2][N];  // [x parity][e]
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int o = c ^ p;
                const int oc = c ^ 1;
                const Vec<T, N>& cen = M[dy + 1][oc];
                const Vec<T, N>& uc = M[dy + 1][c];
                const int64_t own = k * g.P + c * g.H + (int64_t)j * g.hw + m0;
                const int64_t oth = k * g.P + oc * g.H + (int64_t)j * g.hw + m0;
                const Vec<T, N> fv = vload<T, N>(f + own);
                const T edge = o == 0 ? (xlo ? (T)0 : u[oth - 1]) : (xhi ? (T)0 : u[oth + N]);
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const T xl = o == 0 ? (e == 0 ? edge : cen.v[e - 1]) : cen.v[e];
                    const T xr = o == 0 ? cen.v[e] : (e == N - 1 ? edge : cen.v[e + 1]);
                    T s = xl + xr;
                    s = s + M[dy][oc].v[e];
                    s = s + M[dy + 2][oc].v[e];
                    if (DIM == 3) {
                        s = s + Z[0][dy][oc].v[e];
                        s = s + Z[1][dy][oc].v[e];
                    }
                    T res;
                    if (fast) {
                        const T askew = s * op.inv_hSq;
                        const T a_u = askew + op.adiag * uc.v[e];
                        res = fv.v[e] - a_u;
                    } else {
                        const int i = 2 * (m0 + e) + o;
                        res = op.residual(s, fv.v[e], uc.v[e], nbyz + (i == 0) + (i == g.nx - 1));
                    }
                    rr[o][e] = res;
                }
            }
#pragma unroll
            for (int e = 0; e < N; ++e) {
                if (dz == 0 && dy == 0) {
                    acc[e] = rr[0][e] + rr[1][e];
                } else {
                    acc[e] = acc[e] + rr[0][e];
                    acc[e] = acc[e] + rr[1][e];
                }
            }
        }
    }
    // coarse cells I0 + e: colour (I0 + e + J + gK) & 1, packed position (I0 + e) >> 1
    const int64_t gK = gc.z0 + K;
    const int pc = (int)((J + gK) & 1);
    T val[N];
#pragma unroll
    for (int e = 0; e < N; ++e) val[e] = (DIM == 3 ? (T)0.125 : (T)0.25) * acc[e];
    const int64_t rowc = K * gc.P + (int64_t)J * gc.hw;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int I = m0 + e;
        R[rowc + ((I + pc) & 1) * gc.H + (I >> 1)] = val[e];
    }
}

// ---- full-weighting restriction (build-defined option, north_star) ------------------------------
//
// The cell-centred adjoint of the linear prolongation (oracle: restrict_fw in mgp_oracle_impl.h): per
// axis coarse I takes fine 2I-1 .. 2I+2 as ((r_a + w_b r_b) + w_c r_c) + r_d, w = 3 or, next to a box
// face, 3 - clc; fine cells outside the box are +0; x, then y, then z; times 1/8^DIM.  The residual is
// materialised first (k_resfield_v / k_residual_field into the level-sized scratch), because each fine
// residual feeds 2^DIM coarse cells; on a slab level one ghost plane of r is exchanged in between.

// (fw_eval: mgp_cell.h)

// r = f - A u at both colours of a level (vector form, k_half's item): the scratch of the full weighting
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_resfield_v(const T* __restrict__ u, const T* __restrict__ f,
                                                       T* __restrict__ r, Geo g, Op<T, DIM> op, int64_t items)
{
    constexpr int N = VN<T>::n;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    if (it >= 2 * items) return;
    const int color = it >= items;
    HalfIn<T, N> in;
    half_load<T, DIM>(in, u, f, g, color, it - color * items);
    const Vec<T, N> uc = vload<T, N>(u + in.own);
    const bool fast = op.cl == (T)0;
    Vec<T, N> out;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int o = in.o;
        const int i = 2 * (in.m0 + e) + o;
        const T xl = o == 0 ? (e == 0 ? in.edge : in.cen.v[e - 1]) : in.cen.v[e];
        const T xr = o == 0 ? in.cen.v[e] : (e == N - 1 ? in.edge : in.cen.v[e + 1]);
        T sm = xl + xr;
        sm = sm + in.yl.v[e];
        sm = sm + in.yr.v[e];
        if (DIM == 3) {
            sm = sm + in.zl.v[e];
            sm = sm + in.zr.v[e];
        }
        out.v[e] = fast ? op.residual(sm, in.fv.v[e], uc.v[e], 0)
                        : op.residual(sm, in.fv.v[e], uc.v[e], in.nbyz + (i == 0) + (i == g.nx - 1));
    }
    vstore<T, N>(r + in.own, out);
}

// Scalar form: a thread per coarse cell (any sizes), r packed with readable planes -1 and g.nz; evaluated in
// C (double under the cpu-raw float arithmetic) and rounded once
template <typename T, int DIM, typename C = T>
__global__ __launch_bounds__(kBlock) void k_fw_s(const T* __restrict__ r, T* __restrict__ R, Geo g, Geo gc, C wf)
{
    const int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (it >= resrestrict_items<T, DIM>(g)) return;
    const int cx = g.nx >> 1, cy = g.ny >> 1;
    const int I = (int)(it % cx), J = (int)((it / cx) % cy);
    const int64_t K = it / ((int64_t)cx * cy);
    auto get = [&](int i, int j, int64_t k) { return (C)r[pidx(g, i, j, k)]; };
    R[pidx(gc, I, J, K)] = (T)fw_eval<C, DIM>(get, g, gc, wf, I, J, K);
}

// Vector form (coarse nx >= N): a thread owns N consecutive coarse cells I0 .. of one coarse row; each
// of its 4 (2D) / 16 (3D) fine rows is two N-wide loads (even and odd x of fine cells 2 I0 .. 2 I0 + 2N - 1)
// plus the two edge cells, reduced along x at once and accumulated in fw_eval's order.
template <typename T, int DIM>
__global__ __launch_bounds__(kBlock) void k_fw_v(const T* __restrict__ r, T* __restrict__ R, Geo g, Geo gc, T wf)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int cx = g.nx >> 1, cy = g.ny >> 1;
    const int lgpr = (g.lx - 1) - LN;
    const int64_t ncz = DIM == 3 ? (g.nz >> 1) : 1;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    const int grp = (int)(it & ((1 << lgpr) - 1));
    const int J = (int)((it >> lgpr) & (cy - 1));
    const int64_t K = it >> (lgpr + g.ly - 1);
    if (K >= ncz) return;
    const int I0 = grp * N;
    const T w3 = (T)3;
    T az[N], ay[N];
#pragma unroll
    for (int e = 0; e < N; ++e) az[e] = (T)0;
#pragma unroll
    for (int dz = 0; dz < (DIM == 3 ? 4 : 1); ++dz) {
        const int64_t k = DIM == 3 ? 2 * K - 1 + dz : 0;
        const int64_t gk = g.z0 + k;
        const bool kin = DIM == 2 || (gk >= 0 && gk < g.gnz);
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const int j = 2 * J - 1 + dy;
            Vec<T, N> ev = vzero<T, N>(), od = vzero<T, N>();
            T left = (T)0, right = (T)0;
            if (kin && j >= 0 && j < g.ny) {
                const int pe = (int)((j + gk) & 1);  // colour of the row's even x
                const T* row = r + k * g.P + (int64_t)j * g.hw;
                ev = vload<T, N>(row + pe * g.H + I0);
                od = vload<T, N>(row + (pe ^ 1) * g.H + I0);
                if (I0 > 0) left = row[(pe ^ 1) * g.H + I0 - 1];  // fine 2 I0 - 1
                if (I0 + N < cx) right = row[pe * g.H + I0 + N];  // fine 2 I0 + 2N
            }
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const int I = I0 + e;
                const T a = e == 0 ? left : od.v[e - 1];
                const T d = e == N - 1 ? right : ev.v[e + 1];
                const T ax = fw_axis(a, ev.v[e], od.v[e], d, I == 0 ? wf : w3, I == cx - 1 ? wf : w3);
                if (dy == 0) ay[e] = ax;
                else if (dy == 1) ay[e] = ay[e] + (J == 0 ? wf : w3) * ax;
                else if (dy == 2) ay[e] = ay[e] + (J == cy - 1 ? wf : w3) * ax;
                else ay[e] = ay[e] + ax;
            }
        }
#pragma unroll
        for (int e = 0; e < N; ++e) {
            if (DIM == 2) {
                az[e] = ay[e];
            } else {
                const int64_t gK = gc.z0 + K;
                if (dz == 0) az[e] = ay[e];
                else if (dz == 1) az[e] = az[e] + (gK == 0 ? wf : w3) * ay[e];
                else if (dz == 2) az[e] = az[e] + (gK == gc.gnz - 1 ? wf : w3) * ay[e];
                else az[e] = az[e] + ay[e];
            }
        }
    }
    const int64_t gK = gc.z0 + K;
    const int pc = (int)((J + gK) & 1);
    const int64_t rowc = K * gc.P + (int64_t)J * gc.hw;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int I = I0 + e;
        R[rowc + ((I + pc) & 1) * gc.H + (I >> 1)] = (DIM == 3 ? (T)(1.0 / 512.0) : (T)(1.0 / 64.0)) * az[e];
    }
}

// ---- prolongation + correction --------------------------------------------------------------

// (prolong_value, prolong_item: mgp_cell.h)

// a thread per fine slot of colour `color` (any sizes)
template <typename T, int DIM, int LINEAR, typename C = T>
__global__ __launch_bounds__(kBlock) void k_prolong(T* __restrict__ u, const T* __restrict__ V, Geo g, Geo gc,
                                                    double clc, int color)
{
    const int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (it >= g.H * g.nz) return;
    prolong_item<T, DIM, LINEAR, C>(u, V, g, gc, (C)clc, color, it);
}

// Coarse samples x = I0-1 .. I0+N of coarse row (Jr, Kr) (Kr relative to the V pointer) into
// c[0 .. N+1]; samples outside the row are 0 (never used: the caller clamps to the parent).
// In the packed layout I0 .. I0+N-1 sit pairwise in the two halves at (I0 >> 1) ..: two 2-wide
// loads for fp32, plus the two edge samples.
template <typename T, int N>
__device__ __forceinline__ void coarse_row(const T* __restrict__ V, const Geo& gc, int Jr, int64_t Kr, int I0,
                                           T (&c)[N + 2])
{
    const int pc = (int)((Jr + gc.z0 + Kr) & 1);  // colour of even x in this row
    const int64_t row = Kr * gc.P + (int64_t)Jr * gc.hw;
    const T* hp = V + row + pc * gc.H;        // colour of I0, I0+2, ...
    const T* hq = V + row + (pc ^ 1) * gc.H;  // colour of I0+1, I0+3, ...
    const int cm = I0 >> 1;
    if constexpr (N == 4) {
        const Vec<T, 2> a = vload<T, 2>(hp + cm);
        const Vec<T, 2> b = vload<T, 2>(hq + cm);
        c[1] = a.v[0];
        c[2] = b.v[0];
        c[3] = a.v[1];
        c[4] = b.v[1];
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) c[e + 1] = ((e & 1) ? hq : hp)[cm + (e >> 1)];
    }
    c[0] = I0 > 0 ? hq[cm - 1] : (T)0;
    c[N + 1] = I0 + N < gc.nx ? hp[cm + N / 2] : (T)0;
}

// The coarse neighbourhood of fine row (j, k) above coarse cells I0 .. I0+N-1 (coarse rows J, Jn and
// planes K, Kn; Jn, Kn clamped to the parent row / plane outside the box, where the oracle's cval()
// factor applies) and the oracle's per-cell prolongation value of its cells.
template <typename T, int N, int DIM, int LINEAR>
struct PvRow {
    T c00[N + 2], c10[N + 2], c01[N + 2], c11[N + 2];  // [z: K / Kn][y: J / Jn]
    bool oy, oz, interior;
    int I0, cx;
    // load()'s flags with rows J / Jn (2D, or plane K with oz = false) already in registers
    __device__ __forceinline__ void set_rows(const Geo& gc, int j, int64_t k, int i0, const T (&r0)[N + 2],
                                             const T (&r1)[N + 2])
    {
        static_assert(DIM == 2, "set_rows: 2D rows");
        I0 = i0;
        cx = gc.nx;
        const int J = j >> 1;
        const int Jn = (j & 1) ? J + 1 : J - 1;
        oy = Jn < 0 || Jn >= gc.ny;
        oz = false;
        (void)k;
#pragma unroll
        for (int e = 0; e < N + 2; ++e) {
            c00[e] = r0[e];
            if (LINEAR) c10[e] = r1[e];
        }
        interior = !oy && I0 > 0 && I0 + N < cx;
    }
    __device__ __forceinline__ void load(const T* __restrict__ V, const Geo& gc, int j, int64_t k, int i0)
    {
        I0 = i0;
        cx = gc.nx;
        const int J = j >> 1;
        const int64_t K = DIM == 3 ? (k >> 1) : 0;
        int Jn = (j & 1) ? J + 1 : J - 1;
        oy = Jn < 0 || Jn >= gc.ny;
        if (oy) Jn = J;
        int64_t Kn = K;
        oz = false;
        if (DIM == 3) {
            Kn = (k & 1) ? K + 1 : K - 1;
            oz = gc.z0 + Kn < 0 || gc.z0 + Kn >= gc.gnz;
            if (oz) Kn = K;
        }
        coarse_row<T, N>(V, gc, J, K, I0, c00);
        if (LINEAR) {
            coarse_row<T, N>(V, gc, Jn, K, I0, c10);
            if (DIM == 3) {
                coarse_row<T, N>(V, gc, J, Kn, I0, c01);
                coarse_row<T, N>(V, gc, Jn, Kn, I0, c11);
            }
        }
        interior = !oy && !oz && I0 > 0 && I0 + N < cx;
    }
    // P V at the cell above coarse I0 + e with x parity o
    __device__ __forceinline__ T value(int e, int o, T cl) const
    {
        const T w0 = (T)0.75, w1 = (T)0.25;
        const int pe = e + 1;  // parent I0 + e
        if (!LINEAR) return c00[pe];
        if (interior) {  // no neighbour leaves the box: every factor is 1
            const T nb00 = o ? c00[e + 2] : c00[e];
            const T nb10 = o ? c10[e + 2] : c10[e];
            const T a00 = w0 * c00[pe] + w1 * nb00;
            const T a10 = w0 * c10[pe] + w1 * nb10;
            if (DIM == 2) return w0 * a00 + w1 * a10;
            const T nb01 = o ? c01[e + 2] : c01[e];
            const T nb11 = o ? c11[e + 2] : c11[e];
            const T a01 = w0 * c01[pe] + w1 * nb01;
            const T a11 = w0 * c11[pe] + w1 * nb11;
            const T b0 = w0 * a00 + w1 * a10;
            const T b1 = w0 * a01 + w1 * a11;
            return w0 * b0 + w1 * b1;
        }
        const bool ox = (o == 0 && I0 + e == 0) || (o == 1 && I0 + e == cx - 1);
        if (!oy && !oz) {
            // only the x neighbour can leave the box: the general form below with fy = fz = false, i.e. the
            // neighbour column replaced by the parent times the factor -cl (sv's s == 1 test kept)
            const T sx = -cl;
            auto nx_ = [&](const T (&cc)[N + 2]) {
                return ox ? (sx == (T)1 ? cc[pe] : sx * cc[pe]) : (o ? cc[e + 2] : cc[e]);
            };
            const T a00 = w0 * c00[pe] + w1 * nx_(c00);
            const T a10 = w0 * c10[pe] + w1 * nx_(c10);
            if (DIM == 2) return w0 * a00 + w1 * a10;
            const T a01 = w0 * c01[pe] + w1 * nx_(c01);
            const T a11 = w0 * c11[pe] + w1 * nx_(c11);
            const T b0 = w0 * a00 + w1 * a10;
            const T b1 = w0 * a01 + w1 * a11;
            return w0 * b0 + w1 * b1;
        }
        auto sv = [&](T val, bool fx, bool fy, bool fz) {
            T s = (T)1;
            if (fx) s = -cl * s;
            if (fy) s = -cl * s;
            if (fz) s = -cl * s;
            return s == (T)1 ? val : s * val;
        };
        // neighbour column: e (o = 0) or e + 2 (o = 1); the parent when out of the box
        auto col = [&](const T (&cc)[N + 2]) { return ox ? cc[pe] : (o ? cc[e + 2] : cc[e]); };
        const T a00 = w0 * c00[pe] + w1 * sv(col(c00), ox, false, false);
        const T a10 = w0 * sv(c10[pe], false, oy, false) + w1 * sv(col(c10), ox, oy, false);
        if (DIM == 2) return w0 * a00 + w1 * a10;
        const T a01 = w0 * sv(c01[pe], false, false, oz) + w1 * sv(col(c01), ox, false, oz);
        const T a11 = w0 * sv(c11[pe], false, oy, oz) + w1 * sv(col(c11), ox, oy, oz);
        const T b0 = w0 * a00 + w1 * a10;
        const T b1 = w0 * a01 + w1 * a11;
        return w0 * b0 + w1 * b1;
    }
};

// Vector form (coarse nx >= N): a thread owns the fine cells of one fine row (j, k) above N
// consecutive coarse cells I0 .. — fine m = I0 .. in BOTH colours (one N-wide access of u each) —
// and evaluates exactly the oracle's per-cell expression (PvRow).
// BLACK: only the black cells (the cycle's prolongation before a red/black post-smoothing, whose red
// half-sweep replaces every red cell without reading it)
template <typename T, int DIM, int LINEAR, bool BLACK = false>
__global__ __launch_bounds__(kBlock) void k_prolong_v(T* __restrict__ u, const T* __restrict__ V, Geo g, Geo gc,
                                                      T cl)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int lgpr = gc.lx - LN;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    const int grp = (int)(it & ((1 << lgpr) - 1));
    const int j = (int)((it >> lgpr) & (g.ny - 1));
    // the threads past the last item (the grid is whole workgroups) leave here in 2D as well: their j would
    // wrap onto rows that other threads update (u += P V twice, a cross-wave race)
    const int64_t k = it >> (lgpr + g.ly);
    if (k >= (DIM == 3 ? (int64_t)g.nz : 1)) return;
    const int I0 = grp * N;
    PvRow<T, N, DIM, LINEAR> pv;
    pv.load(V, gc, j, k, I0);
    const int p = (int)((j + g.z0 + k) & 1);
#pragma unroll
    for (int c = BLACK ? 1 : 0; c < 2; ++c) {
        const int o = c ^ p;  // x parity of this colour's cells in row j
        const int64_t own = k * g.P + c * g.H + (int64_t)j * g.hw + I0;
        Vec<T, N> uv = vload<T, N>(u + own);
#pragma unroll
        for (int e = 0; e < N; ++e) uv.v[e] = uv.v[e] + pv.value(e, o, cl);
        vstore<T, N>(u + own, uv);
    }
}

// Prolongation + correction fused with the first (red) half-sweep of the post-smoothing
// (prolong_correct + the red half of smooth's first sweep).  The red half-sweep replaces every red
// cell without reading it, and the black half-sweep after it replaces every black cell without
// reading it, so u + P V is only ever read on black cells by this red half-sweep: each thread
// evaluates it (PvRow, k_prolong_v's expressions) for the black neighbours of its N red cells —
// its own row, rows j +- 1 and planes k +- 1, plus one edge cell — and writes only the red cells.
// The black cells keep u without P V until the black half-sweep overwrites them.  HBM: read black u,
// red f and V, write red u (the per-piece pair also writes and re-reads both colours of u).
template <typename T, int DIM, int LINEAR>
__global__ __launch_bounds__(kBlock) void k_post1(T* __restrict__ u, const T* __restrict__ V,
                                                  const T* __restrict__ f, Geo g, Geo gc, Op<T, DIM> op, T clc)
{
    constexpr int N = VN<T>::n;
    constexpr int LN = N == 4 ? 2 : 1;
    const int lgpr = g.lhw - LN;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t it = (int64_t)b * kBlock + threadIdx.x;
    const int grp = (int)(it & ((1 << lgpr) - 1));
    const int j = (int)((it >> lgpr) & (g.ny - 1));
    const int64_t k = it >> (lgpr + g.ly);
    if (k >= g.nz) return;
    const int m0 = grp * N;
    const int64_t gk = g.z0 + k;
    const int orr = (int)((j + gk) & 1);  // x parity of this row's red cells (black: orr ^ 1)
    // u + P V of black row (jj, kk) at m0 .. m0+N-1 (0 outside the box)
    auto black_row = [&](int jj, int64_t kk, Vec<T, N>& r) {
        const int64_t gkk = g.z0 + kk;
        if (jj < 0 || jj >= g.ny || (DIM == 3 && (gkk < 0 || gkk >= g.gnz))) {
            r = vzero<T, N>();
            return;
        }
        const int ob = 1 ^ (int)((jj + gkk) & 1);
        r = vload<T, N>(u + kk * g.P + g.H + (int64_t)jj * g.hw + m0);
        PvRow<T, N, DIM, LINEAR> pv;
        pv.load(V, gc, jj, kk, m0);
#pragma unroll
        for (int e = 0; e < N; ++e) r.v[e] = r.v[e] + pv.value(e, ob, clc);
    };
    Vec<T, N> bc, byl, byr, bzl, bzr;
    black_row(j, k, bc);
    black_row(j - 1, k, byl);
    black_row(j + 1, k, byr);
    if (DIM == 3) {
        black_row(j, k - 1, bzl);
        black_row(j, k + 1, bzr);
    }
    // the black x-neighbour outside the segment: m0 - 1 (red cells at even x) or m0 + N (odd x)
    const int me = orr == 0 ? m0 - 1 : m0 + N;
    T edge = (T)0;
    if (me >= 0 && me < g.hw) {
        const int i = 2 * me + (orr ^ 1);
        edge = u[k * g.P + g.H + (int64_t)j * g.hw + me] + prolong_value<T, DIM, LINEAR>(V, g, gc, clc, i, j, k);
    }
    const int64_t own = k * g.P + (int64_t)j * g.hw + m0;
    const Vec<T, N> fr = vload<T, N>(f + own);
    const int nbyz = (j == 0) + (j == g.ny - 1) + (DIM == 3 ? (gk == 0) + (gk == g.gnz - 1) : 0);
    Vec<T, N> out;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int i = 2 * (m0 + e) + orr;
        const T xl = orr == 0 ? (e == 0 ? edge : bc.v[e - 1]) : bc.v[e];
        const T xr = orr == 0 ? bc.v[e] : (e == N - 1 ? edge : bc.v[e + 1]);
        T s = xl + xr;
        s = s + byl.v[e];
        s = s + byr.v[e];
        if (DIM == 3) {
            s = s + bzl.v[e];
            s = s + bzr.v[e];
        }
        out.v[e] = op.relax(s, fr.v[e], nbyz + (i == 0) + (i == g.nx - 1));
    }
    vstore<T, N>(u + own, out);
}

// (k_zs, its build knobs, ZsShape and the zs_* helpers: mgp_zs.h)

// ---- k_zs PRE with its stages split over two groups of waves (fp32, cl = 0, the 2^3-average restriction) ----
//
// k_zs's step is a chain: stage k's newest z-neighbour is the plane stage k - 1 computed in the same step, so the
// tile wave that sits alone on its SIMD runs stage 0, four half-sweeps and the residual back to back, with nothing
// to cover its LDS round trips.  Here two groups of waves share the chain:
//   group A  stage 0 (the prefetched black u and f) and stages 1 .. 3: at step p planes p .. p - 3, as k_zs
//   group B  stage 4, the store of the smoothed black plane and the residual + restriction, one step behind:
//            at step p planes p - 5, p - 5 and p - 6
// The hand-off is stage 3's output, which k_zs already leaves in a 4-slot LDS ring for stage 4's in-plane neighbours:
// B reads the newest plane of its own column from it (plane p - 4, written one step earlier) into its register ring
// W3, so k_zs's slots keep their layout and the step keeps its single barrier..  Stage 4 needs the black cells of stage
// 2 nowhere (a Gauss-Seidel update does not read the value it replaces), so no u crosses otherwise..  A leaves the f of
// B's planes in two LDS rings of their own (red f of plane p - 3, black f of plane p - 2, both in its registers
// anyway), so B issues no global load: fetching those lines a second time, three and four steps after A, cost more
// than the split gained (PRE 416 against 317 us at 512^3)..  A's threads are k_zs's (the full H = 5 trapezoid, the same
// wave roles); B's cover the rows within 1 of the tile..  The 20 threads of B's two halo rows share a wave with the 40
// of A's rows d >= 4 (both run one light stage), which keeps the workgroup at 12 waves: three on a SIMD, 168
// VGPRs..  Every expression is k_zs's, in its order: the results are bit-identical. The warm-up and the drain of a chunk
// grow by one step; the planes read from HBM (and the ghost planes of a slab) do not change.
template <typename T>
struct ZsSplit {
    using S = ZsShape<T, true, true>;
    static_assert(S::XPAIR && S::H == 5 && S::NS3 == 4 && kZsRask, "the split follows k_zs's 64 x 32 PRE layout");
    static constexpr int NTW = S::TC / 64;  // tile waves of each group
    // Wave order: A's tile waves, B's tile waves, A's x-halo wave, B's x-halo wave, A's rows d = 1..3, then the
    // mixed wave (lanes [0, MA): A's rows d >= 4, lanes [MA, MA + MB): B's rows d = 1).  With waves dealt to the
    // four SIMDs in turn, every SIMD gets one tile wave of each group and one halo wave.
    static constexpr int NW = 2 * NTW + 4, NTL = 64 * NW, WMIX = NW - 1;
    static constexpr int MA = S::YT2 - S::YT2S, MB = 2 * S::G;
    static_assert(NTW == 4 && S::NTL == 64 * 7 && S::YT2S == 64 * 6 && S::YT0 == 64 * 5 && MA + MB <= 64, "wave order");
    // wave w: 0 group A, 1 group B, 2 mixed; its wave index within the group's own thread numbering
    static constexpr int wave_kind(int w) { return w == WMIX ? 2 : (w < 2 * NTW ? w >= NTW : ((w - 2 * NTW) & 1)); }
    static constexpr int local_wave(int w) { return w < 2 * NTW ? w % NTW : NTW + (w - 2 * NTW) / 2; }
    // B's thread t: the tile rows and their x-halo groups as k_zs's threads, then the rows d = 1
    static constexpr int BT1 = S::YT0 + MB;
    static __device__ __forceinline__ int b_yrow(int t)
    {
        if (t < S::YT0) return S::yrow(t);
        if (t < BT1) return t - S::YT0 < S::G ? S::H - 1 : S::H + S::TY;
        return -1;
    }
    static __device__ __forceinline__ int b_ycol(int t) { return t < S::YT0 ? S::ycol(t) : (t - S::YT0) % S::G; }
    // LDS: k_zs's layout, then the f hand-off: rings of 4 planes of red f and of black f over B's rows
    static constexpr int FROWS = S::TY + 2, FSLOT = FROWS * S::HWE;
    static constexpr int OFFFR = (int)(S::lds_bytes / sizeof(T)), OFFFB = OFFFR + 4 * FSLOT;
    static constexpr size_t lds_bytes = (size_t)(OFFFB + 4 * FSLOT) * sizeof(T);
    // one workgroup per CU: <= 1024 threads, <= 160 KiB LDS, and at 12 waves (3 on a SIMD) <= 168 VGPRs, which the
    // launch bound makes the compiler's limit
    static_assert(NTL <= 1024 && NW <= 12, "too many waves for 168 VGPRs");
    static_assert(lds_bytes <= 160 * 1024, "LDS");
};

//
// CLZ = false (k_zs_split_cl): a level with a boundary-modified operator (cl != 0, the fused levels below the finest and
// the 256^3 level of the 512^3 box), from a fresh zero guess.  The tile and the layout are the same; the steady steps
// take k_zs's steady diagonals (ZsDiag, zs_dvals), the generic ones the row's table entries (zs_diag): the table
// Markstein division equals the plain one for every such divisor (mgp_device.h), so these are bit-identical to k_zs's
// relax_direct / residual_direct without their divergent IEEE division.  A warm guess (ZSRC = false) stays on k_zs:
// that instantiation needs 22 VGPRs beyond the 168 of 12 waves and spills.
template <typename T, bool ZSRC, bool CLZ>
__device__ __forceinline__ void zs_split_body(const T* __restrict__ src, const T* __restrict__ f, T* __restrict__ dst,
                                              T* __restrict__ R, const Geo& g, const Geo& gc, const Op<T, 3>& op, int zc,
                                              int gz, int patch)
{
    using SP = ZsSplit<T>;
    static_assert(CLZ || (ZsShape<T, true, false>::TX == SP::S::TX && ZsShape<T, true, false>::TY == SP::S::TY &&
                          ZsShape<T, true, false>::N == SP::S::N),
                  "the split's cl != 0 levels run the cl = 0 tile");
    using S = typename SP::S;
    constexpr int N = S::N, H = S::H, HWE = S::HWE, G = S::G, YE = S::YE, SLOT = S::SLOT, TX = S::TX, TY = S::TY,
                  NS3 = S::NS3;
    using VT = Vec<T, N>;
    using PF = ZsPrefetch<T, N>;
    constexpr int PFD = ZS_PFD_PRE, NPF = PFD + 1, UNR = NPF == 3 ? 12 : 4;
    static_assert(PFD >= 1 && PFD <= 3, "prefetch distance 1..3");
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

    // my wave's kind, my group, my thread of it and its column of the extended tile (as k_zs)
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wk = SP::wave_kind(wv), lw = SP::local_wave(wv);
    const bool grp_b = wk == 1 || (wk == 2 && lane >= SP::MA);
    const int lt = wk == 2 ? (grp_b ? S::YT0 + lane - SP::MA : S::YT2S + lane) : 64 * lw + lane;
    const int yr_ = grp_b ? SP::b_yrow(lt) : S::yrow(lt);
    const bool on = yr_ >= 0;
    const int gx = on ? (grp_b ? SP::b_ycol(lt) : S::ycol(lt)) : 0, ye = on ? yr_ : 0;
    const int gy = Y0 - H + ye;
    const int m0 = gx * N;
    ZsCol col;
    col.lrow = ye * HWE + m0;
    col.lym = (ye > 0 ? ye - 1 : ye) * HWE + m0;
    col.lyp = (ye < YE - 1 ? ye + 1 : ye) * HWE + m0;
    col.gm = (X0 - S::HX) / 2 + m0;  // global packed m of my first cell
    col.x_first = gx == 0;
    col.x_last = gx == G - 1;
    col.lxm = col.x_first ? col.lrow : col.lrow - N;
    col.lxp = col.x_last ? col.lrow : col.lrow + N;
    const bool in_xy = on && gy >= 0 && gy < g.ny && col.gm >= 0 && col.gm < hw;
    col.xin = true;  // (unused: no stage takes k_zs's direct boundary path)
    // columns outside the box load from a clamped in-plane position; their results never reach LDS or HBM
    const int cgy = gy < 0 ? 0 : (gy >= g.ny ? g.ny - 1 : gy);
    const int cgm = col.gm < 0 ? 0 : (col.gm > hw - N ? hw - N : col.gm);
    const int goff = cgy * hw + cgm;  // in-plane offset (nx * ny < 2^31)
    const bool tile_xy = on && ye >= H && ye < H + TY && gx >= S::HXG && gx < G - S::HXG;
    // my column in a slot of the f hand-off (B's rows: those within 1 of the tile)
    const bool frow = on && ye >= H - 1 && ye <= H + TY;
    const int lf = frow ? (ye - (H - 1)) * HWE + m0 : 0;
    auto fslot = [&](int off, int q) { return lds + off + (q & 3) * SP::FSLOT + lf; };
    const int zlo = Z0 - H;
    ZsDiag<T> dz = {};  // (cl = 0: unused)
    if constexpr (!CLZ) {  // as k_zs
        const int nby = (gy == 0) + (gy == g.ny - 1);  // 0 .. 2 (ny >= 2)
        dz.db = nby == 0 ? op.dg[0] : (nby == 1 ? op.dg[1] : op.dg[2]);
        dz.yb = nby == 0 ? op.ydg[0] : (nby == 1 ? op.ydg[1] : op.ydg[2]);
        dz.de = nby == 0 ? op.dg[1] : (nby == 1 ? op.dg[2] : op.dg[3]);
        dz.ye = nby == 0 ? op.ydg[1] : (nby == 1 ? op.ydg[2] : op.ydg[3]);
        dz.left = col.gm == 0;
        dz.right = col.gm + N == hw;
    }
    // y / z faces of my row at plane q (the generic steps' table index; the steady steps' planes are off the z faces)
    constexpr bool FAI = ZS_FACE_AS_INTERIOR && !CLZ;  // (timing experiment, see k_zs)
    auto nbyz = [&](int q) {
        if (FAI) return (gy == 0) + (gy == g.ny - 1);
        return CLZ ? 0 : (gy == 0) + (gy == g.ny - 1) + (z0 + q == 0) + (z0 + q == gnz - 1);
    };
    const int p_end = Z0 + zc + 6;
    auto inz = [&](int q) { return FAI || (z0 + q >= 0 && z0 + q < gnz); };  // inside the global box
    auto pcl = [&](int q) { return q < qlo ? qlo : (q > qhi ? qhi : q); };
    auto slot = [&](int off, int ns, int q) { return lds + off + (q & (ns - 1)) * SLOT; };
    const int rowpar = (gy + z0) & 1;
    auto par = [&](int q) { return rowpar ^ (q & 1); };
    const VT vz = vzero<T, N>();

    for (int i = tid; i < (int)(SP::lds_bytes / sizeof(T)); i += SP::NTL) lds[i] = (T)0;
    __syncthreads();

    // steady steps [ps, pe], as k_zs: every plane a step touches (p .. p - 6) inside the box (cl != 0: and every stage's
    // plane off the z faces), the prefetched planes readable, even z0 and Z0 (static plane parity).  The generic steps
    // before them are whole groups of UNR steps.  PART (the cl != 0 levels, whose chunks are short): the steady range
    // ends where it ends, in a partial group that the epilogue completes, so a chunk away from the z faces runs no
    // generic step at all (rounded to whole groups, 8 of a 32-plane chunk's 44 steps were generic).  Level 0 keeps
    // whole groups: with every steady step behind a bound test its 268-step launch measured 292 against 276 us, for
    // 4 generic steps saved.
    constexpr bool PART = !CLZ;
    int ps = zlo, pe = p_end;
    if (!FAI) ps = ps > 7 - z0 ? ps : 7 - z0;
    ps = ps > qlo + 4 ? ps : qlo + 4;
    if (!FAI) pe = pe < gnz - 1 - z0 ? pe : gnz - 1 - z0;
    pe = pe < qhi - PFD ? pe : qhi - PFD;
    ps += (UNR - (ps - zlo) % UNR) % UNR;
    if (!PART) pe -= (pe - ps + 1) % UNR;
    if (pe < ps || ((z0 | Z0) & 1)) ps = pe = zlo - 1;
    const std::false_type GEN;
    const std::true_type STY;
    // Every wave runs the same steps, whatever its kind, and each step ends in the step's one barrier: the bounds
    // above are the workgroup's.  prefetch / step: the wave kind's.
    auto run = [&](auto&& prefetch, auto&& step) __attribute__((always_inline)) {
        PF pb[NPF];
#pragma unroll
        for (int k = 0; k < PFD; ++k) prefetch(GEN, pb[k], zlo + k);
        int p = zlo;
        // the steps pfirst .. plim of the group of UNR steps from p0 (p0 - zlo a multiple of UNR: ring slot k & 3,
        // buffers k % NPF and (k + PFD) % NPF)
        auto group = [&](auto st, int p0, int pfirst, int plim) __attribute__((always_inline)) {
            zs_unroll<UNR>([&](auto kk) __attribute__((always_inline)) {
                constexpr int k = decltype(kk)::value;
                if (p0 + k >= pfirst && p0 + k <= plim) {
                    step(st, std::integral_constant<int, (k & 3)>(), pb[k % NPF], pb[(k + PFD) % NPF], p0 + k);
                    lds_barrier();
                }
            });
        };
        for (; p < ps; p += UNR) group(GEN, p, p, p + UNR);
        for (; p + UNR - 1 <= pe; p += UNR) group(STY, p, p, p + UNR);  // (whole groups: the bound tests fold away)
        int pf = p;
        if constexpr (PART) {
            if (p <= pe) {  // the partial steady group; the epilogue's first group completes it
                group(STY, p, p, pe);
                pf = pe + 1;
            }
        }
        for (; p <= p_end; p += UNR) group(GEN, p, PART ? pf : p, p_end);
    };

    // ---- group A: stages 0 .. 3 (k_zs's, with its wave roles: rows d >= 4 run stage 1 only) ----
    const T* const src_black = ZSRC ? nullptr : src + Hh;
    auto prefetch_a = [&](auto st, PF& r, int p) __attribute__((always_inline)) {
        constexpr bool ST = decltype(st)::value;
        if (ST && !FAI) {
            const int64_t pP = (int64_t)p * P;
            if constexpr (ZSRC)
                r.u = vzero<T, N>();
            else
                r.u = gload<T, N, kZsNTL>(src_black + pP + goff);
            r.f1 = gload<T, N, kZsNTL>(f + (pP - P) + goff);
            r.f2 = gload<T, N, kZsNTL>(f + (pP - 2 * P) + Hh + goff);
        } else {
            if constexpr (ZSRC)
                r.u = vzero<T, N>();
            else
                r.u = gload<T, N, kZsNTL>(src_black + (int64_t)pcl(p) * P + goff);
            r.f1 = gload<T, N, kZsNTL>(f + (int64_t)pcl(p - 1) * P + goff);
            r.f2 = gload<T, N, kZsNTL>(f + (int64_t)pcl(p - 2) * P + Hh + goff);
        }
    };
    // W0: A0 black at p-2 .. p; W1: A1 red at p-3 .. p-1; W2: A2 black at p-4 .. p-2; FR: red f of planes
    // p-3 .. p-1 (plane q in slot (q - zlo) & 3; every step knows its slot offset at compile time, as k_zs)
    VT W0[4], W1[4], W2[4], FR[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) W0[i] = W1[i] = W2[i] = FR[i] = vz;
    // ro: the wave's role (0, 1: every stage of the group; 2: rows d >= 4, stage 1 only)
    auto step_a = [&](auto st, auto rt, const PF& cur, PF& nxt, int p, int ro) __attribute__((always_inline)) {
        constexpr bool ST = decltype(st)::value;
        constexpr int RS = decltype(rt)::value;  // (p - zlo) & 3
        auto sl = [](int k) constexpr { return (RS - k) & 3; };  // ring slot of plane p - k
        if (ST) p = (p & ~1) | ((H + RS) & 1);  // steady: Z0 even, so p's parity is zlo's plus RS
        zs_hold<T, N>(cur.u);
        zs_hold<T, N>(cur.f1);
        zs_hold<T, N>(cur.f2);
        asm volatile("" ::: "memory");
        if (ST || p + PFD <= p_end) prefetch_a(st, nxt, p + PFD);
        ZsNb<T, N> n1, n2, n3;
        VT a0 = cur.u;
        if (!ST && !inz(p)) a0 = vz;
        W0[sl(0)] = a0;
        zs_nb_load<T, N>(n1, slot(0, 2, p - 1), col);
        VT o1 = zs_relax<T, N, CLZ, ST, !CLZ>(W0[sl(2)], W0[sl(1)], W0[sl(0)], n1, cur.f1, col, par(p - 1), nbyz(p - 1), g.nx, op, dz);
        if (!ST && !inz(p - 1)) o1 = vz;
        W1[sl(1)] = o1;
        VT o2 = vz, o3 = vz;
        if (ro < 2) {
            zs_nb_load<T, N>(n2, slot(S::OFF1, 2, p - 2), col);
            o2 = zs_relax<T, N, CLZ, ST, !CLZ>(W1[sl(3)], W1[sl(2)], W1[sl(1)], n2, cur.f2, col, 1 ^ par(p - 2), nbyz(p - 2), g.nx, op, dz);
            if (!ST && !inz(p - 2)) o2 = vz;
            W2[sl(2)] = o2;
            zs_nb_load<T, N>(n3, slot(S::OFF2, 2, p - 3), col);
            o3 = zs_relax<T, N, CLZ, ST, !CLZ>(W2[sl(4)], W2[sl(3)], W2[sl(2)], n3, FR[sl(3)], col, par(p - 3), nbyz(p - 3), g.nx, op, dz);
            if (!ST && !inz(p - 3)) o3 = vz;
        }
        if (in_xy) {  // (slots no stage of this step reads; columns outside the box stay 0)
            vstore<T, N>(slot(0, 2, p) + col.lrow, a0);
            vstore<T, N>(slot(S::OFF1, 2, p - 1) + col.lrow, o1);
            if (ro < 2) {
                vstore<T, N>(slot(S::OFF2, 2, p - 2) + col.lrow, o2);
                vstore<T, N>(slot(S::OFF3, NS3, p - 3) + col.lrow, o3);
            }
            if (frow) {  // B reads them three steps later (stage 4: black f of plane p - 5, the residual: red f of p - 6)
                vstore<T, N>(fslot(SP::OFFFR, p - 3), FR[sl(3)]);
                vstore<T, N>(fslot(SP::OFFFB, p - 2), cur.f2);
            }
        }
        FR[sl(1)] = cur.f1;  // red f of plane p - 1
    };

    // ---- group B: stage 4, the smoothed black plane, the residual + restriction (tile waves only) ----
    auto prefetch_b = [](auto, PF&, int) {};  // (no global loads: its f comes from A through LDS)
    // W3: A3 red at p-6 .. p-4 (from LDS); W4: A4 black at p-7 .. p-5; FB: black f of planes p-6, p-5; AS: stage
    // 4's askew of the last two steps (ZS_RASK); acc: the restriction's sum
    VT W3[4], W4[4], FB[4];
    T AS[2][N], acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) AS[0][e] = AS[1][e] = acc[e] = (T)0;
#pragma unroll
    for (int i = 0; i < 4; ++i) W3[i] = W4[i] = FB[i] = vz;
    const bool even_row = (gy & 1) == 0;
    T* const xbase = lds + S::OFFX + (((ye + (H & 1)) >> 1) * G + gx) * 2 * N;
    auto xs = [&](int q) { return xbase + (q & 1) * (S::XPAIRS * G * 2 * N); };
    // tw: a tile wave (the others run stage 4 only)
    auto step_b = [&](auto st, auto rt, auto tw, int p) __attribute__((always_inline)) {
        constexpr bool ST = decltype(st)::value;
        constexpr int RS = decltype(rt)::value;  // (p - zlo) & 3
        auto sl = [](int k) constexpr { return (RS - k) & 3; };  // ring slot of plane p - k
        if (ST) p = (p & ~1) | ((H + RS) & 1);
        const int zz0 = ST ? (z0 & ~1) : z0;
        ZsNb<T, N> n4, nk;
        const VT fb = vload<T, N>(fslot(SP::OFFFB, p - 5));  // black f of plane p - 5
        // ---- stage 4 on plane p - 5: A's stage-3 planes p - 6 .. p - 4, the newest written one step ago ----
        W3[sl(4)] = vload<T, N>(slot(S::OFF3, NS3, p - 4) + col.lrow);
        zs_nb_load<T, N>(n4, slot(S::OFF3, NS3, p - 5), col);
        VT o4 = zs_relax_a<T, N, CLZ, ST, !CLZ>(W3[sl(6)], W3[sl(5)], W3[sl(4)], n4, fb, col, 1 ^ par(p - 5), nbyz(p - 5), g.nx, op, dz,
                                           AS[RS & 1]);
        if (!ST && !inz(p - 5)) o4 = vz;
        W4[sl(5)] = o4;
        if (in_xy) vstore<T, N>(slot(S::OFF4, 2, p - 5) + col.lrow, o4);
        if constexpr (decltype(tw)::value) {
            // ---- the smoothed plane p - 5: its black cells (POST never reads the red ones, see k_zs) ----
            {
                const int q = p - 5;
                if (q >= Z0 && q < Z0 + zc && tile_xy) gstore<T, N, kZsNTS>(dst + (int64_t)q * P + Hh + goff, o4);
            }
            // ---- residual + restriction of plane p - 6 ----
            const int q = p - 6;
            const int pq = par(q);
            zs_nb_load<T, N>(nk, slot(S::OFF4, 2, q), col);  // black of A4 at q
            T xr[2 * N];
            {
                const T* x = xs(q - 1);  // the odd row's residuals of plane q - 1 (even rows read them)
#pragma unroll
                for (int e = 0; e < 2 * N; ++e) xr[e] = x[e];
            }
            // red cells (x parity pq) see black neighbours; the black cells' neighbours are the red cells of the last
            // step's stage 4 (its askew, ZS_RASK)
            T rred[N], rblk[N], rr[2][N];  // rr: [x parity][e]
            const VT fr = vload<T, N>(fslot(SP::OFFFR, q));  // red f of plane q
            zs_residual<T, N, CLZ, ST, !CLZ>(W4[sl(7)], W4[sl(6)], W4[sl(5)], nk, W3[sl(6)], fr, col, pq, nbyz(q), g.nx, op, dz, rred);
            zs_residual_a<T, N, CLZ, ST, !CLZ>(AS[(RS & 1) ^ 1], W4[sl(6)], FB[sl(6)], col, 1 ^ pq, nbyz(q), g.nx, op, dz, rblk);
#pragma unroll
            for (int e = 0; e < N; ++e) {
                rr[0][e] = pq == 0 ? rred[e] : rblk[e];
                rr[1][e] = pq == 0 ? rblk[e] : rred[e];
            }
            const int dq = q - (ST ? (Z0 & ~1) : Z0);
            if (dq >= 0 && dq <= zc && tile_xy)
                zs_restrict_avg<T, N>(rr, xr, acc, dq, zc, even_row, xs(q), R, (zz0 + q - 1) >> 1, gy >> 1, col.gm, cz0, gc);
            FB[sl(5)] = fb;  // black f of plane p - 5
        }
    };

    if (wk == 0) {
        const int wrole = S::wave_role(lw);
        run(prefetch_a, [&](auto st, auto rt, const PF& cur, PF& nxt, int p) __attribute__((always_inline)) {
            step_a(st, rt, cur, nxt, p, decltype(st)::value ? wrole : 0);  // (every generic step runs the full work)
        });
    } else if (wk == 1) {
        if (lw < SP::NTW)
            run(prefetch_b, [&](auto st, auto rt, const PF& cur, PF& nxt, int p) __attribute__((always_inline)) {
                step_b(st, rt, STY, p);
            });
        else
            run(prefetch_b, [&](auto st, auto rt, const PF& cur, PF& nxt, int p) __attribute__((always_inline)) {
                step_b(st, rt, GEN, p);
            });
    } else {
        // (two separate conditionals, not an if / else: the compiler merges the two arms' stores into one store
        // through a selected address, which puts the rings in private memory)
        run(
            [&](auto st, PF& r, int p) __attribute__((always_inline)) {
                if (!grp_b) prefetch_a(st, r, p);
            },
            [&](auto st, auto rt, const PF& cur, PF& nxt, int p) __attribute__((always_inline)) {
                if (!grp_b) step_a(st, rt, cur, nxt, p, 2);
                asm volatile("" ::: "memory");
                if (grp_b) step_b(st, rt, GEN, p);
            });
    }
}

template <typename T, bool ZSRC>
__global__ __launch_bounds__((ZsSplit<T>::NTL)) void k_zs_split(const T* __restrict__ src, const T* __restrict__ f,
                                                                 T* __restrict__ dst, T* __restrict__ R, Geo g, Geo gc,
                                                                 Op<T, 3> op, int zc, int gz, int patch)
{
    zs_split_body<T, ZSRC, true>(src, f, dst, R, g, gc, op, zc, gz, patch);
}

// a level with a boundary-modified operator (cl != 0), from a fresh zero guess
template <typename T>
__global__ __launch_bounds__((ZsSplit<T>::NTL)) void k_zs_split_cl(const T* __restrict__ f, T* __restrict__ dst,
                                                                    T* __restrict__ R, Geo g, Geo gc, Op<T, 3> op, int zc,
                                                                    int gz, int patch)
{
    zs_split_body<T, true, false>(nullptr, f, dst, R, g, gc, op, zc, gz, patch);
}

// ---- k_zs POST with its stages split over two groups of waves (fp32, cl = 0, trilinear P, the wide tile) ----
//
// The stage split of k_zs_split applied to POST, on 16-byte columns (N = 4 on the 128 x 16 tile: half k_zs's
// instructions per cell, which at k_zs's one group of 7 waves only made up for the waves it lost):
//   group A  stage 0 (the prefetched black u + the coarse correction, k_zs's BQ cache) and half-sweeps 1 and 2: at step
//            p planes p .. p - 2, over the whole extended tile (G x YE threads)
//   group B  half-sweeps 3 and 4, the err and the stores of the smoothed plane, one step behind: at step p planes
//            p - 4 and p - 5, over the rows within 1 of the tile
// The hand-off is stage 2's output, which k_zs leaves in an LDS ring for stage 3's in-plane neighbours: the ring has 4
// slots here (the fourth is the one A fills meanwhile), and B reads the three planes of its own column from it as well,
// the newest (plane p - 3) written one step earlier: a register ring for them made B spill.  Stage 4 reads no stage-2
// value of its own cell, so no other u crosses.  A leaves the f of B's planes in two 4-slot LDS rings over B's rows (red
// f of plane p - 1, black f of plane p - 2), so B loads no f; B loads psiOld itself (tile columns only) and fills the
// coarse staging ring, which A reads (A's BQ cache): with the coarse planes in flight A needed more than 168 VGPRs.
// B's rows d = 1 hold the tile's own column groups only (half-sweep 4 reads nothing else of them), so B is 320 threads,
// five whole waves, and with A's 432 the workgroup has 12 waves (3 on a SIMD, 168 VGPRs) without a wave that mixes the
// groups (A's threads beside B's in one wave spilled); A's last wave holds rows d >= 3 and skips half-sweep 2.  Every
// expression is k_zs's, in its order: psi is bit-identical.  So is the err: a B thread keeps one (err, err1) pair per
// 2-cell group, the accumulators of the k_zs (N = 2) thread that owned those cells, and the workgroup sums them in
// k_zs's tree over k_zs's thread numbering.  The warm-up and the drain of a chunk grow by one step; the planes read
// from HBM do not change (neither group loads anything for the added step).
template <typename T>
struct ZsSplitPost {
    using S = ZsShape<T, false, true, true, false, 4>;
    static_assert(S::N == 4 && S::H == 4 && S::HXG == 1 && S::NS3 == 2 && !S::PS && !S::YROLE, "POST's wide tile, 16-byte columns");
    // A: the extended tile: the rows d <= 2 from the tile in y (every stage of A), then d = 3 (stages 0 and 1), then
    // d = 4 (stage 0), so that its last MA threads, a wave of their own, skip half-sweep 2
    static constexpr int G = S::G, NA = S::NT, NA2 = G * (S::TY + 4), NA3 = NA2 + 2 * G;
    // B: the tile rows (every column group: the x-halo groups feed half-sweep 4's x neighbours), then the rows d = 1,
    // of which half-sweep 4 reads the tile's own column groups only: GC per row, which makes B whole waves
    static constexpr int BROWS = S::TY + 2, GC = G - 2 * S::HXG, NBT = G * S::TY, NB = NBT + 2 * GC;
    static constexpr int NWA = NA / 64, NWB = NB / 64, MA = NA - 64 * NWA;
    static constexpr int NW = NWA + NWB + 1, NTL = 64 * NW, WLAST = NW - 1;
    // Wave order (bit w of BMASK: wave w is B's; the last wave holds A's last MA threads): A B A B  B A B A  A B A A'.
    // With waves dealt to the four SIMDs in turn, every SIMD gets waves of both groups.
    static constexpr unsigned BMASK = 0x25A;
    static_assert(NWA == 6 && NWB == 5 && NB == 64 * NWB && MA > 0 && NW == 12, "wave order");
    // wave w: 0 group A (every stage), 1 group B, 2 A's last wave (rows d >= 3: stages 0 and 1)
    static __device__ __forceinline__ int wave_kind(int w) { return w == WLAST ? 2 : (int)((BMASK >> w) & 1u); }
    static __device__ __forceinline__ int local_wave(int w)  // its index among the waves of its kind
    {
        const unsigned below = (1u << w) - 1u;
        return __builtin_popcount(((BMASK >> w) & 1u) ? (BMASK & below) : (~BMASK & below));
    }
    static_assert(NA2 <= 64 * NWA, "A's last wave holds rows d >= 3 only");
    static __device__ __forceinline__ int a_yrow(int t)
    {
        if (t < NA2) return 2 + t / G;
        if (t < NA3) return t - NA2 < G ? 1 : S::YE - 2;
        if (t < NA) return t - NA3 < G ? 0 : S::YE - 1;
        return -1;
    }
    static __device__ __forceinline__ int b_yrow(int t)
    {
        if (t < NBT) return S::H + t / G;
        return t - NBT < GC ? S::H - 1 : S::H + S::TY;
    }
    static __device__ __forceinline__ int b_ycol(int t) { return t < NBT ? t % G : S::HXG + (t - NBT) % GC; }
    // LDS: stage 0 and stage 1 (2 slots each), the stage-2 ring (4), stage 3 (2), the coarse ring, the f rings
    static constexpr int SLOT = S::SLOT, OFF1 = 2 * SLOT, OFF2 = 4 * SLOT, OFF3 = 8 * SLOT, OFFC = 10 * SLOT;
    static constexpr int FSLOT = BROWS * S::HWE;
    static constexpr int OFFFR = OFFC + 4 * S::CSLOT, OFFFB = OFFFR + 4 * FSLOT;
    static constexpr size_t lds_bytes = (size_t)(OFFFB + 4 * FSLOT) * sizeof(T);
    // the err partial's array: k_zs's threads (8-byte columns on the same tile: x halo 4, row-major, whole waves)
    static constexpr int EG = (S::TX + 8) / 4, ENT = (EG * S::YE + 63) / 64 * 64;
    static_assert(OFFC % 4 == 0 && S::CPAIRS <= 2 * NB, "coarse staging: two pairs per thread of B");
    static_assert(NTL <= 1024 && NW <= 12, "too many waves for 168 VGPRs");
    static_assert(lds_bytes + ENT * sizeof(double) <= 160 * 1024, "LDS");
    static_assert(ENT <= 1024 && ENT - 512 <= NTL, "the sum's first level within the workgroup");
};

template <typename T, bool ERR>
__global__ __launch_bounds__((ZsSplitPost<T>::NTL)) void k_zs_split_post(const T* __restrict__ src, const T* __restrict__ f,
                                                                          T* __restrict__ dst, const T* old,
                                                                          const T* __restrict__ V,
                                                                          double* __restrict__ partials, Geo g, Geo gc,
                                                                          Op<T, 3> op, T clc, int zc, int gz, int patch)
{
    using SP = ZsSplitPost<T>;
    using S = typename SP::S;
    constexpr int N = S::N, H = S::H, HWE = S::HWE, G = S::G, YE = S::YE, SLOT = S::SLOT, TX = S::TX, TY = S::TY;
    using VT = Vec<T, N>;
    using PF = ZsPrefetch<T, N>;
    constexpr int PFD = 1, NPF = PFD + 1, UNR = 4;
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

    // my wave's kind, my group, my thread of it and its column of the extended tile (as k_zs)
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wk = SP::wave_kind(wv), lw = SP::local_wave(wv);
    const bool grp_b = wk == 1;
    const int lt = wk == 2 ? 64 * SP::NWA + lane : 64 * lw + lane;
    const int yr_ = grp_b ? SP::b_yrow(lt) : SP::a_yrow(lt);
    const bool on = yr_ >= 0;
    const int gx = on ? (grp_b ? SP::b_ycol(lt) : lt % G) : 0, ye = on ? yr_ : 0;
    const int gy = Y0 - H + ye;
    const int m0 = gx * N;
    ZsCol col;
    col.lrow = ye * HWE + m0;
    col.lym = (ye > 0 ? ye - 1 : ye) * HWE + m0;
    col.lyp = (ye < YE - 1 ? ye + 1 : ye) * HWE + m0;
    col.gm = (X0 - S::HX) / 2 + m0;  // global packed m of my first cell
    col.x_first = gx == 0;
    col.x_last = gx == G - 1;
    col.lxm = col.x_first ? col.lrow : col.lrow - N;
    col.lxp = col.x_last ? col.lrow : col.lrow + N;
    const bool in_xy = on && gy >= 0 && gy < g.ny && col.gm >= 0 && col.gm < hw;
    col.xin = true;  // (unused: cl = 0)
    // columns outside the box load from a clamped in-plane position; their results never reach LDS or HBM
    const int cgy = gy < 0 ? 0 : (gy >= g.ny ? g.ny - 1 : gy);
    const int cgm = col.gm < 0 ? 0 : (col.gm > hw - N ? hw - N : col.gm);
    const int goff = cgy * hw + cgm;  // in-plane offset (nx * ny < 2^31)
    const bool tile_xy = on && ye >= H && ye < H + TY && gx >= S::HXG && gx < G - S::HXG;
    // the y-halo rows load only the f their stages can use (k_zs's ZS_FHALO)
    const int ydist = ye < H ? H - ye : (ye >= H + TY ? ye - (H + TY) + 1 : 0);
    const bool need_f1 = !ZS_FHALO || ydist <= H - 1, need_f2 = !ZS_FHALO || ydist <= H - 2;
    // my column in a slot of the f hand-off (B's rows: those within 1 of the tile)
    const bool frow = on && ye >= H - 1 && ye <= H + TY;
    const int lf = frow ? (ye - (H - 1)) * HWE + m0 : 0;
    auto fslot = [&](int off, int q) { return lds + off + (q & 3) * SP::FSLOT + lf; };
    const int zlo = Z0 - H;
    const ZsDiag<T> dz = {};  // (cl = 0: unused)
    // B's last step is p_end; A's last plane is k_zs's (p_end - 1): it loads nothing for the step the split adds
    const int p_end = Z0 + zc + 4;
    auto inz = [&](int q) { return z0 + q >= 0 && z0 + q < gnz; };  // inside the global box
    auto pcl = [&](int q) { return q < qlo ? qlo : (q > qhi ? qhi : q); };
    auto slot = [&](int off, int ns, int q) { return lds + off + (q & (ns - 1)) * SLOT; };
    const int rowpar = (gy + z0) & 1;
    auto par = [&](int q) { return rowpar ^ (q & 1); };
    const VT vz = vzero<T, N>();

    for (int i = tid; i < (int)(SP::lds_bytes / sizeof(T)); i += SP::NTL) lds[i] = (T)0;
    __syncthreads();

    // ---- the coarse staging ring, plane K in slot K & 3 (planes clamped to the box), as k_zs; B's threads fill it (A,
    // which reads it, has no registers to spare for the planes in flight) ----
    const int Ia = X0 / 2 - 8, Ja = Y0 / 2 - 3;
    auto ckl = [&](int K) { return K < 0 ? 0 : (K >= gc.gnz ? gc.gnz - 1 : K); };
    auto cslot = [&](int K) { return lds + SP::OFFC + (K & 3) * S::CSLOT; };
    // my two pairs of the region: the in-plane offset of the pair's even cell (-1: none, or outside the coarse box) and
    // the parity of I + J
    int coff[2], cpar[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = lt + i * SP::NB;
        const int J = Ja + t / (S::CI / 2), I = Ia + 2 * (t % (S::CI / 2));
        const bool ok = grp_b && t < S::CPAIRS && J >= 0 && J < gc.ny && I >= 0 && I < gc.nx;
        // I even: cells I and I + 1 sit at m = I / 2 of the two colour halves
        coff[i] = ok ? J * gc.hw + (I >> 1) : -1;
        cpar[i] = (I + J) & 1;
    }
    auto cload = [&](PF& r, int K) {
        K = ckl(K);
        const T* const pl = V + (int64_t)(K - cz0) * gc.P;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            r.cv[i].v[0] = r.cv[i].v[1] = (T)0;
            if (coff[i] >= 0) {
                const int ce = (cpar[i] + K) & 1;
                r.cv[i].v[0] = pl[coff[i] + ce * (int)gc.H];
                r.cv[i].v[1] = pl[coff[i] + (ce ^ 1) * (int)gc.H];
            }
        }
    };
    auto cstore = [&](const PF& r, int K) {
        T* const sl = cslot(ckl(K));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t = lt + i * SP::NB;
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
    if (grp_b) {  // the coarse planes the first fine plane needs
        PF r;
        const int K = (z0 + zlo) >> 1;
        for (int k = K - 1; k <= K + 1; ++k) {
            cload(r, k);
            cstore(r, k);
        }
    }
    __syncthreads();

    // steady steps [ps, pe], as k_zs's POST: every plane a step touches (p .. p - 5) inside the box, Kn inside the coarse
    // box, the prefetched planes readable, even z0 and Z0 and (z0 + Z0) % 4 == 0 (static parity of the plane and of the
    // coarse plane), whole groups of UNR steps.  They end before the step the split adds.
    int ps = zlo, pe = p_end - 1;
    ps = ps > 6 - z0 ? ps : 6 - z0;
    ps = ps > qlo + 4 ? ps : qlo + 4;
    pe = pe < gnz - 2 - z0 ? pe : gnz - 2 - z0;
    pe = pe < qhi - PFD ? pe : qhi - PFD;
    ps += (UNR - (ps - zlo) % UNR) % UNR;
    pe -= (pe - ps + 1) % UNR;
    if (pe < ps || ((z0 | Z0) & 1) || ((z0 + Z0) & 3)) ps = pe = zlo - 1;
    const std::false_type GEN;
    const std::true_type STY;
    // Every wave runs the same steps, whatever its kind, and each step ends in the step's one barrier: the bounds
    // above are the workgroup's.  prefetch / step: the wave kind's; first_steady: before the first steady step.
    auto run = [&](auto&& prefetch, auto&& first_steady, auto&& step) __attribute__((always_inline)) {
        PF pb[NPF];
#pragma unroll
        for (int k = 0; k < NPF; ++k) pb[k].f1 = pb[k].f2 = vz;  // (the halo rows that skip f loads keep zeros)
#pragma unroll
        for (int k = 0; k < PFD; ++k) prefetch(GEN, pb[k], zlo + k);
        int p = zlo;
        // the steps up to plim of the group of UNR steps from p0 (p0 - zlo a multiple of UNR: ring slot k & 3, buffers
        // k % NPF and (k + PFD) % NPF)
        auto group = [&](auto st, int p0, int plim) __attribute__((always_inline)) {
            zs_unroll<UNR>([&](auto kk) __attribute__((always_inline)) {
                constexpr int k = decltype(kk)::value;
                if (p0 + k <= plim) {
                    step(st, std::integral_constant<int, (k & 3)>(), pb[k % NPF], pb[(k + PFD) % NPF], p0 + k);
                    lds_barrier();
                }
            });
        };
        for (; p < ps; p += UNR) group(GEN, p, p + UNR);
        if (p <= pe) first_steady(p);
        for (; p <= pe; p += UNR) group(STY, p, p + UNR);  // (whole groups: the bound tests fold away)
        for (; p <= p_end; p += UNR) group(GEN, p, p_end);
    };

    // ---- group A: stage 0 with the coarse correction, half-sweeps 1 and 2 (k_zs's) ----
    const T* const src_black = src + Hh;
    auto prefetch_a = [&](auto st, PF& r, int p) __attribute__((always_inline)) {
        constexpr bool ST = decltype(st)::value;
        if (ST) {
            const int64_t pP = (int64_t)p * P;
            r.u = gload<T, N, kZsNTL>(src_black + pP + goff);
            if (need_f1) r.f1 = gload<T, N, kZsNTL>(f + (pP - P) + goff);
            if (need_f2) r.f2 = gload<T, N, kZsNTL>(f + (pP - 2 * P) + Hh + goff);
        } else {
            r.u = gload<T, N, kZsNTL>(src_black + (int64_t)pcl(p) * P + goff);
            if (need_f1) r.f1 = gload<T, N, kZsNTL>(f + (int64_t)pcl(p - 1) * P + goff);
            if (need_f2) r.f2 = gload<T, N, kZsNTL>(f + (int64_t)pcl(p - 2) * P + Hh + goff);
        }
    };
    // W0: A0 black at p-2 .. p; W1: A1 red at p-3 .. p-1 (plane q in slot (q - zlo) & 3; every step knows its slot
    // offset at compile time, as k_zs)
    VT W0[4], W1[4];
    // the per-lane half of the interior test of the coarse correction (lanes without a column do not vote)
    const bool corr_lane = (cgy >> 1) + ((cgy & 1) ? 1 : -1) >= 0 && (cgy >> 1) + ((cgy & 1) ? 1 : -1) < gc.ny && cgm > 0 &&
                           cgm + N < gc.nx;
    const bool corr_fast = __all(!on || corr_lane);
    // steady steps: BQ[K & 1][q][e] = zs_bq of coarse plane K for the black cells of the fine planes of parity 1 ^ q (see
    // k_zs)
    T BQ[2][2][N];
    // (each group's rings start from zeros in its own branch below: nothing of the other group's stays live in it)
    auto init_a = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) W0[i] = W1[i] = vz;
#pragma unroll
        for (int i = 0; i < 2 * 2 * N; ++i) (&BQ[0][0][0])[i] = (T)0;
    };
    const int bq_J = cgy >> 1;
    int bq_Jn = (cgy & 1) ? bq_J + 1 : bq_J - 1;
    const bool bq_oy = bq_Jn < 0 || bq_Jn >= gc.ny;
    if (bq_oy) bq_Jn = bq_J;
    auto bq_fill = [&](T (&bq)[2][N], int K) __attribute__((always_inline)) {
        const int cp = cgy & 1;
        T c0[N + 2], c1[N + 2];
        crow(K, bq_J, c0);
        crow(K, bq_Jn, c1);
#pragma unroll
        for (int q = 0; q < 2; ++q) zs_bq<T, N>(bq[q], c0, c1, q ^ cp, cgm, gc.nx, bq_oy, clc, corr_fast);
    };
    auto first_steady_a = [&](int p) __attribute__((always_inline)) {
        // the first steady step (even, K & 1 == 0) reads coarse planes K and K - 1
        const int K = (z0 + p) >> 1;
        bq_fill(BQ[0], K);
        bq_fill(BQ[1], K - 1);
    };
    // full: every stage of A (false: A's last wave, rows d >= 3: stages 0 and 1)
    auto step_a = [&](auto st, auto rt, auto full, const PF& cur, PF& nxt, int p) __attribute__((always_inline)) {
        constexpr bool ST = decltype(st)::value, FULL = decltype(full)::value;
        constexpr int RS = decltype(rt)::value;  // (p - zlo) & 3
        auto sl = [](int k) constexpr { return (RS - k) & 3; };  // ring slot of plane p - k
        if (!ST && p >= p_end) return;  // the step the split adds: nothing of A's would be read (cur holds no new plane)
        if (ST) p = (p & ~1) | ((H + RS) & 1);  // steady: Z0 even, so p's parity is zlo's plus RS
        const int zz0 = ST ? (z0 & ~1) : z0;
        zs_hold<T, N>(cur.u);
        zs_hold<T, N>(cur.f1);
        zs_hold<T, N>(cur.f2);
        asm volatile("" ::: "memory");
        if (ST || p + PFD <= p_end - 1) prefetch_a(st, nxt, p + PFD);
        ZsNb<T, N> n1, n2;
        // ---- stage 0: black cells of plane p ----
        VT a0 = cur.u;
        if constexpr (ST) {
            // (z0 + Z0) % 4 == 0 in steady steps: K & 1 and p & 1 are static
            constexpr int KS = (RS >> 1) & 1, Q = 1 ^ (RS & 1);
            if constexpr ((RS & 1) != 0) bq_fill(BQ[KS ^ 1], ((zz0 + p) >> 1) + 1);
            const T w0 = (T)0.75, w1 = (T)0.25;
#pragma unroll
            for (int e = 0; e < N; ++e) a0.v[e] = a0.v[e] + (w0 * BQ[KS][Q][e] + w1 * BQ[KS ^ 1][Q][e]);
        } else if (inz(p)) {
            const int J = cgy >> 1, K = (zz0 + p) >> 1;
            int Jn = (cgy & 1) ? J + 1 : J - 1;
            int Kn = ((zz0 + p) & 1) ? K + 1 : K - 1;
            const bool oy = Jn < 0 || Jn >= gc.ny, oz = Kn < 0 || Kn >= gc.gnz;
            if (oy) Jn = J;
            if (oz) Kn = K;
            ZsCoarse<T, N> cc;
            crow(K, J, cc.c00);
            crow(K, Jn, cc.c10);
            crow(Kn, J, cc.c01);
            crow(Kn, Jn, cc.c11);
            zs_correct<T, N, 1>(a0, cc, 1 ^ ((cgy + zz0 + p) & 1), cgm, gc.nx, oy, oz, clc,
                                __all(!oy && !oz && cgm > 0 && cgm + N < gc.nx));
        }
        if (!ST && !inz(p)) a0 = vz;
        W0[sl(0)] = a0;
        // ---- half-sweeps 1 and 2 on planes p - 1 (red) and p - 2 (black) ----
        zs_nb_load<T, N>(n1, slot(0, 2, p - 1), col);
        VT o1 = zs_relax<T, N, true, ST>(W0[sl(2)], W0[sl(1)], W0[sl(0)], n1, cur.f1, col, par(p - 1), 0, g.nx, op, dz);
        if (!ST && !inz(p - 1)) o1 = vz;
        W1[sl(1)] = o1;
        VT o2 = vz;
        if constexpr (FULL) {
            zs_nb_load<T, N>(n2, slot(SP::OFF1, 2, p - 2), col);
            o2 = zs_relax<T, N, true, ST>(W1[sl(3)], W1[sl(2)], W1[sl(1)], n2, cur.f2, col, 1 ^ par(p - 2), 0, g.nx, op, dz);
            if (!ST && !inz(p - 2)) o2 = vz;
        }
        if (in_xy) {  // (slots no stage of this step reads; columns outside the box stay 0)
            vstore<T, N>(slot(0, 2, p) + col.lrow, a0);
            vstore<T, N>(slot(SP::OFF1, 2, p - 1) + col.lrow, o1);
            // (B reads its own column of it in the next step, the neighbours in the step after)
            if constexpr (FULL) vstore<T, N>(slot(SP::OFF2, 4, p - 2) + col.lrow, o2);
            if (FULL && frow) {  // B reads them three steps later (stage 3: red f of plane p - 4, stage 4: black f of p - 5)
                vstore<T, N>(fslot(SP::OFFFR, p - 1), cur.f1);
                vstore<T, N>(fslot(SP::OFFFB, p - 2), cur.f2);
            }
        }
    };

    // ---- group B: half-sweeps 3 and 4, the err, the smoothed plane ----
    auto prefetch_b = [&](auto st, PF& r, int p) __attribute__((always_inline)) {
        constexpr bool ST = decltype(st)::value;
        const int zz0 = ST ? (z0 & ~1) : z0;
        // fine plane 2m + 1 is the first to need coarse plane m + 1; it is loaded with the prefetch of plane 2m and put
        // in the ring at the top of step 2m (none for the step the split adds: A corrects no plane there)
        if ((ST || p < p_end) && ((zz0 + p) & 1) == 0) cload(r, ((zz0 + p) >> 1) + 1);
        if (ERR && tile_xy) {  // psiOld of plane p - 5 (the plane step p finalizes), for the tile's own columns only
            const T* dp = old + (ST ? (int64_t)p * P - 5 * P : (int64_t)pcl(p - 5) * P);
            r.o0 = gload<T, N, kZsNTO>(dp + goff);
            r.o1 = gload<T, N, kZsNTO>(dp + Hh + goff);
        }
    };
    // W3: A3 red at p-6 .. p-4 (A2's planes p-5 .. p-3 of my column come from the stage-2 ring every step: its fourth
    // slot is the one A fills meanwhile, and B has no registers to keep them in)
    VT W3[4];
    // err[j], err1[j]: the accumulators of k_zs's thread that owns my cells 2j, 2j + 1 of each colour
    double err[2], err1[2];
    double esum[2] = {0.0, 0.0};  // err[j] + err1[j] after the last step
    auto step_b = [&](auto st, auto rt, const PF& cur, PF& nxt, int p) __attribute__((always_inline)) {
        constexpr bool ST = decltype(st)::value;
        constexpr int RS = decltype(rt)::value;  // (p - zlo) & 3
        auto sl = [](int k) constexpr { return (RS - k) & 3; };  // ring slot of plane p - k
        if (ST) p = (p & ~1) | ((H + RS) & 1);
        const int zz0 = ST ? (z0 & ~1) : z0;
        if (ERR) {
            zs_hold<T, N>(cur.o0);
            zs_hold<T, N>(cur.o1);
        }
        zs_hold<T, 2>(cur.cv[0]);
        zs_hold<T, 2>(cur.cv[1]);
        asm volatile("" ::: "memory");
        // the coarse plane cur's prefetch loaded (A first reads it one step on; the slot it replaces was last read three
        // steps back)
        if ((ST || p < p_end) && ((zz0 + p) & 1) == 0) cstore(cur, ((zz0 + p) >> 1) + 1);
        if (ST || p + PFD <= p_end) prefetch_b(st, nxt, p + PFD);
        ZsNb<T, N> n3, n4;
        // ---- half-sweep 3 on plane p - 4: A's stage-2 planes p - 5 .. p - 3, the newest written one step ago ----
        const VT w2l = vload<T, N>(slot(SP::OFF2, 4, p - 5) + col.lrow), w2c = vload<T, N>(slot(SP::OFF2, 4, p - 4) + col.lrow),
                 w2r = vload<T, N>(slot(SP::OFF2, 4, p - 3) + col.lrow);
        const VT fr = vload<T, N>(fslot(SP::OFFFR, p - 4));  // red f of plane p - 4
        zs_nb_load<T, N>(n3, slot(SP::OFF2, 4, p - 4), col);
        VT o3 = zs_relax<T, N, true, ST>(w2l, w2c, w2r, n3, fr, col, par(p - 4), 0, g.nx, op, dz);
        if (!ST && !inz(p - 4)) o3 = vz;
        if (in_xy) vstore<T, N>(slot(SP::OFF3, 2, p - 4) + col.lrow, o3);
        W3[sl(4)] = o3;
        // ---- half-sweep 4 on plane p - 5 ----
        const VT fb = vload<T, N>(fslot(SP::OFFFB, p - 5));  // black f of plane p - 5
        zs_nb_load<T, N>(n4, slot(SP::OFF3, 2, p - 5), col);
        VT o4 = zs_relax<T, N, true, ST>(W3[sl(6)], W3[sl(5)], W3[sl(4)], n4, fb, col, 1 ^ par(p - 5), 0, g.nx, op, dz);
        if (!ST && !inz(p - 5)) o4 = vz;
        // ---- the smoothed plane p - 5: red final after stage 3, black after stage 4 (the chunk test is wave-uniform) ----
        const int q = p - 5;
        if (q >= Z0 && q < Z0 + zc && tile_xy) {
            if (ERR) {
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    // (psi - psiOld)^2 in fp64, fused multiply-add, in the order of k_zs's thread of the pair
                    const double d0 = (double)W3[sl(5)].v[e] - (double)cur.o0.v[e];
                    const double d1 = (double)o4.v[e] - (double)cur.o1.v[e];
                    err[e >> 1] = __builtin_fma(d0, d0, err[e >> 1]);
                    err1[e >> 1] = __builtin_fma(d1, d1, err1[e >> 1]);
                }
            }
            T* dp = dst + (int64_t)q * P;
            gstore<T, N, kZsNTS>(dp + goff, W3[sl(5)]);
            gstore<T, N, kZsNTS>(dp + Hh + goff, o4);
        }
    };

    if (wk == 0) {
        init_a();
        run(prefetch_a, first_steady_a, [&](auto st, auto rt, const PF& cur, PF& nxt, int p) __attribute__((always_inline)) {
            step_a(st, rt, STY, cur, nxt, p);
        });
    } else if (wk == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) W3[i] = vz;
        err[0] = err[1] = err1[0] = err1[1] = 0.0;
        run(prefetch_b, [](int) {}, step_b);
        esum[0] = err[0] + err1[0];
        esum[1] = err[1] + err1[1];
    } else {
        init_a();
        run(prefetch_a, first_steady_a, [&](auto st, auto rt, const PF& cur, PF& nxt, int p) __attribute__((always_inline)) {
            step_a(st, rt, GEN, cur, nxt, p);
        });
    }
    if constexpr (ERR) {
        // k_zs's workgroup sum (block_partial_t over its ENT threads): thread row x EG + column group holds err + err1
        // of its cells; my pair j is column group 2 gx - 1 + j of k_zs's row
        __shared__ double red[SP::ENT];
        for (int i = tid; i < SP::ENT; i += SP::NTL) red[i] = 0.0;
        __syncthreads();
        // (my row and column group again, from the thread index: nothing of them stays live through A's loops)
        int t2 = tid;
        asm volatile("" : "+v"(t2));
        const int w2 = t2 >> 6, l2 = SP::local_wave(w2) * 64 + (t2 & 63);
        const int y2 = SP::b_yrow(l2), x2 = SP::b_ycol(l2);
        if (SP::wave_kind(w2) == 1 && y2 >= H && y2 < H + TY && x2 >= S::HXG && x2 < G - S::HXG) {
            red[y2 * SP::EG + 2 * x2 - 1] = esum[0];
            red[y2 * SP::EG + 2 * x2] = esum[1];
        }
        __syncthreads();
        for (int w = 512; w > 0; w >>= 1) {
            if (tid < w && tid + w < SP::ENT) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) partials[blockIdx.x] = red[0];
    }
}

// ---- y-streamed temporally blocked smoothing (2D, red/black 2+2) -------------------------------
//
// k_ys is k_zs for a 2D level: rows take the place of planes.  A workgroup owns an x-segment of TX cells
// (plus HX halo cells per side) and a chunk of yc rows, and streams through y; every thread owns one
// column group of the segment: N consecutive cells of each colour (packed m0 .. m0 + N - 1).  At step p:
//   stage 0   black cells of row p (POST: plus the prolongation, PvRow: k_prolong_v's expressions)
//   stage k   half-sweep k (k = 1..4, red first) on row p - k
//   last      row p - 4 is final and stored; PRE: residual of row p - 5 and the restriction (both fine rows
//             of a coarse row belong to the same thread, so the children are summed in registers in the
//             reference order); POST: (psi - psiOld)^2 partials.
// The y-neighbours of stage k are the thread's own register windows of stage k - 1; the only operands
// from other threads are the two x-edge cells, which every stage leaves in LDS (first and last cell of
// its group) for the next stage one step later: one barrier per step.  Halo cells are recomputed by the
// neighbouring segments (the trapezoid shrinks by one cell per stage); rows outside the box are 0.  With
// yc even, Y0 is even and the parity of row p is a compile-time function of the ring slot.  Arithmetic is
// k_half's / k_resrestrict's / k_prolong_v's, so results are bit-identical to the per-piece path.
#ifndef YS_TX_F32
#define YS_TX_F32 1024
#endif
#ifndef YS_TX_F64
#define YS_TX_F64 512
#endif
template <typename T>
constexpr int ys_tx_full() { return sizeof(T) == 4 ? YS_TX_F32 : YS_TX_F64; }
// TXV: segment width (ys_tx_full, or half of it on levels whose full-width segments make too few workgroups)
template <typename T, bool PRE, int TXV = ys_tx_full<T>()>
struct YsShape {
    static constexpr int N = 16 / sizeof(T);
    static constexpr int TX = TXV;
    static constexpr int H = PRE ? 5 : 4;
    static constexpr int HX = 2 * N * ((H + 2 * N - 1) / (2 * N));  // whole column groups
    static constexpr int HWE = TX / 2 + HX;                          // packed cells per colour of a row
    static constexpr int G = HWE / N;                                // column groups (threads with work)
    static constexpr int HXG = HX / 2 / N;
    static constexpr int NTL = (G + 63) / 64 * 64;
    // edge slots (first, last cell of every group): stages 0..2 two rows each, stage 3 four (PRE reads
    // its row p - 5 at step p), stage 4 two (PRE)
    static constexpr int ES = 2 * G;
    static constexpr int OFF1 = 2 * ES, OFF2 = 4 * ES, OFF3 = 6 * ES, OFF4 = 10 * ES;
    // POST: ring of 4 coarse rows (cells I in [X0/2 - 8, X0/2 + TX/2 + 8), x order, both colours)
    static constexpr int CI = PRE ? 0 : TX / 2 + 16, CPAIRS = CI / 2, OFFC = 12 * ES;
    static constexpr size_t lds_floats = 12 * ES + 4 * CI;
    static_assert(CPAIRS <= 2 * NTL, "coarse staging: two pairs per thread");
    static_assert(NTL <= 1024, "too many threads");
    static_assert(2 * N * HXG >= H, "x halo too small");
};

// Rows prefetched YS_PF steps ahead (a ring of 4 buffers, so every index stays static in the 4-step loop).
#ifndef YS_PF
#define YS_PF 2
#endif
static_assert(YS_PF >= 1 && YS_PF <= 3, "prefetch distance 1..3");
template <typename T>
struct YsPrefetch {
    static constexpr int N = 16 / sizeof(T);
    Vec<T, N> u, f1, f2, o0, o1;  // black u of row p; red f of p - 1; black f of p - 2; psiOld of p - 4
    Vec<T, 2> cv[2];              // POST, even p: this thread's coarse pairs of coarse row p / 2 + 1
};

// relax of my N cells of x parity o: rows ym / yp above and below (other colour), cen my row's other
// colour, ep / en the x-edge cells beyond my group; nby = y faces of the row (0 with CLZ).  ask: the cells'
// neighbour sums times 1/h^2, written (AIN = false) or, for a residual whose neighbours a half-sweep of the
// previous step saw (PRE's black cells, as k_zs's ZS_RASK), read instead of re-summing them
template <typename T, int N, bool CLZ, bool RES, bool AIN = false>
__device__ __forceinline__ void ys_cells(const Vec<T, N>& ym, const Vec<T, N>& cen, const Vec<T, N>& yp, T ep, T en,
                                         const Vec<T, N>& fv, const Vec<T, N>& uc, int o, int nby, int gm, int nx,
                                         bool xin, const Op<T, 2>& op, T (&out)[N], T (&ask)[N])
{
    if (!AIN) {
        ZsNb<T, N> nb;
        nb.yl = ym;
        nb.yr = yp;
        nb.ep = ep;
        nb.en = en;
        T t[N];
        zs_xsum<T, N>(cen, nb, o, t);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            t[e] = t[e] + ym.v[e];
            t[e] = t[e] + yp.v[e];
            ask[e] = t[e] * op.inv_hSq;
        }
    }
    // cl != 0: nby is the row's (uniform across the workgroup), so the row's two diagonals (off / on an x
    // face) are one uniform table walk and a cell selects between them: no divergent boundary path (a
    // segment at an x face would otherwise hold its whole workgroup at every step's barrier)
    T d0 = op.adiag, y0 = op.yadiag, d1 = op.adiag, y1 = op.yadiag;
    if (!CLZ) row_diag_fast(op, nby, d0, y0, d1, y1);
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int i = 2 * (gm + e) + o;
        const bool xf = !CLZ && (i == 0 || i == nx - 1);
        const T d = xf ? d1 : d0;
        if (RES) {
            const T a_u = ask[e] + d * uc.v[e];
            out[e] = fv.v[e] - a_u;
        } else {
            out[e] = div_rn(fv.v[e] - ask[e], d, xf ? y1 : y0);
        }
    }
    (void)xin;
}

// PRE: LINEAR selects the restriction (0: residual + 2x2 average here; 1: none, both colours stored)
template <typename T, bool PRE, int LINEAR, bool ERR, bool CLZ, int TXV>
__global__ __launch_bounds__((YsShape<T, PRE, TXV>::NTL)) void k_ys(const T* __restrict__ src, const T* __restrict__ f,
                                                               T* __restrict__ dst, const T* old, T* __restrict__ R,
                                                               const T* __restrict__ V, double* __restrict__ partials,
                                                               Geo g, Geo gc, Op<T, 2> op, T clc, int yc)
{
    using S = YsShape<T, PRE, TXV>;
    constexpr int N = S::N, H = S::H, G = S::G, TX = S::TX, NTL = S::NTL, ES = S::ES;
    constexpr bool RR = PRE && LINEAR == 0;
    using VT = Vec<T, N>;
    using PF = YsPrefetch<T>;
    __shared__ __align__(16) T lds[S::lds_floats];
    const int tid = threadIdx.x;
    const int tiles_x = g.nx / TX;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int X0 = (b % tiles_x) * TX, Y0 = (b / tiles_x) * yc;
    const int hw = g.hw, Hh = (int)g.H, ny = g.ny;
    const bool on = tid < G;
    const int gx = on ? tid : 0;
    const int gm = (X0 - S::HX) / 2 + gx * N;  // global packed m of my first cell
    const bool inx = on && gm >= 0 && gm < hw;
    const bool xin = !inx || (gm > 0 && 2 * (gm + N) < g.nx);  // no cell of the group on an x face
    const int cgm = gm < 0 ? 0 : (gm > hw - N ? hw - N : gm);
    const bool tile_x = on && gx >= S::HXG && gx < G - S::HXG;
    const int zlo = Y0 - H;
    const int p_end = Y0 + yc + (PRE ? 4 : 3);
    auto iny = [&](int q) { return q >= 0 && q < ny; };
    auto rcl = [&](int q) { return q < 0 ? 0 : (q >= ny ? ny - 1 : q); };
    auto nby = [&](int q) { return CLZ ? 0 : (q == 0) + (q == ny - 1); };
    for (int i = tid; i < (int)S::lds_floats; i += NTL) lds[i] = (T)0;
    __syncthreads();
    // edge slot of stage base `off` with `ns` rows, row q
    auto eslot = [&](int off, int ns, int q) { return lds + off + (q & (ns - 1)) * ES; };
    auto put = [&](T* sl, const VT& v) {
        if (inx) {
            sl[2 * gx] = v.v[0];
            sl[2 * gx + 1] = v.v[N - 1];
        }
    };
    auto edges = [&](const T* sl, T& ep, T& en) {  // left group's last cell, right group's first
        ep = gx > 0 ? sl[2 * gx - 1] : (T)0;
        en = gx < G - 1 ? sl[2 * gx + 2] : (T)0;
    };
    // ---- POST: coarse staging ring, row J in slot J & 3 (rows clamped to the box) ----
    const int Ia = X0 / 2 - 8;
    auto cjl = [&](int J) { return J < 0 ? 0 : (J >= gc.ny ? gc.ny - 1 : J); };
    auto cslot = [&](int J) { return lds + S::OFFC + (J & 3) * S::CI; };
    auto cload = [&](PF& r, int J) {
        J = cjl(J);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t = tid + i * NTL;
            const int I = Ia + 2 * t;
            r.cv[i].v[0] = r.cv[i].v[1] = (T)0;
            if (t < S::CPAIRS && I >= 0 && I < gc.nx) {  // I even: cells I, I + 1 at m = I / 2 of the two halves
                const T* row = V + (int64_t)J * gc.hw + (I >> 1);
                const int ce = (I + J) & 1;
                r.cv[i].v[0] = row[ce * gc.H];
                r.cv[i].v[1] = row[(ce ^ 1) * gc.H];
            }
        }
    };
    auto cstore = [&](const PF& r, int J) {
        T* const sl = cslot(cjl(J));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t = tid + i * NTL;
            if (t < S::CPAIRS) vstore<T, 2>(sl + 2 * t, r.cv[i]);
        }
    };
    auto crow = [&](int J, T (&c)[N + 2]) {  // cells cgm - 1 .. cgm + N of coarse row J
        const T* const sl = cslot(cjl(J)) + (cgm - Ia);
        const Vec<T, N> mid = vload<T, N>(sl);
        c[0] = vload_lds_whole<T, N>(sl - N).v[N - 1];
#pragma unroll
        for (int e = 0; e < N; ++e) c[e + 1] = mid.v[e];
        c[N + 1] = vload_lds_whole<T, N>(sl + N).v[0];
    };
    auto prefetch = [&](PF& r, int p) {
        r.u = vload<T, N>(src + Hh + (int64_t)rcl(p) * hw + cgm);
        r.f1 = vload<T, N>(f + (int64_t)rcl(p - 1) * hw + cgm);
        r.f2 = vload<T, N>(f + Hh + (int64_t)rcl(p - 2) * hw + cgm);
        if (!PRE && ERR && tile_x) {
            const int64_t ro = (int64_t)rcl(p - 4) * hw + cgm;
            r.o0 = vload<T, N>(old + ro);
            r.o1 = vload<T, N>(old + Hh + ro);
        }
        // POST: fine row 2m + 1 is the first to need coarse row m + 1; it is loaded with the prefetch of row
        // 2m and put in the ring at the top of step 2m
        if (!PRE && (p & 1) == 0) cload(r, (p >> 1) + 1);
    };
    const VT vz = vzero<T, N>();
    VT W0[4], W1[4], W2[4], W3[4], W4[4], FR[4], FB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) W0[i] = W1[i] = W2[i] = W3[i] = W4[i] = FR[i] = FB[i] = vz;
    T AS[2][N], askd[N];  // PRE: stage 4's askew of the last two steps (row p - 4 at slot RS & 1); scratch
#pragma unroll
    for (int e = 0; e < N; ++e) AS[0][e] = AS[1][e] = askd[e] = (T)0;
    T acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = (T)0;
    double err = 0.0, err1 = 0.0;

    PF pf[4];
    auto step = [&](auto rt, int p) {
        constexpr int RS = decltype(rt)::value;  // (p - zlo) & 3
        const PF& cur = pf[RS];
        auto sl = [](int k) constexpr { return (RS - k) & 3; };
        constexpr int PP = (H + RS) & 1;  // parity of p (Y0 even)
        auto par = [](int k) constexpr { return (PP + k) & 1; };  // parity of row p - k (mod 2)
        zs_hold<T, N>(cur.u);
        zs_hold<T, N>(cur.f1);
        zs_hold<T, N>(cur.f2);
        if (!PRE && ERR) {
            zs_hold<T, N>(cur.o0);
            zs_hold<T, N>(cur.o1);
        }
        if (!PRE && PP == 0) {
            zs_hold<T, 2>(cur.cv[0]);
            zs_hold<T, 2>(cur.cv[1]);
        }
        asm volatile("" ::: "memory");
        // POST: the coarse row this row's prefetch loaded (first read one step on; the slot it replaces was
        // last read three steps back)
        if (!PRE && PP == 0) cstore(cur, (p >> 1) + 1);
        if (p + YS_PF <= p_end) prefetch(pf[(RS + YS_PF) & 3], p + YS_PF);

        // ---- stage 0: black cells of row p (POST: + P V) ----
        VT a0 = cur.u;
        if (!iny(p) || !inx) {
            a0 = vz;
        } else if (!PRE) {
            PvRow<T, N, 2, LINEAR> pv;
            T c0[N + 2], c1[N + 2];
            const int J = p >> 1;
            crow(J, c0);
            if (LINEAR) crow((p & 1) ? J + 1 : J - 1, c1);  // Jn (clamped: PvRow's oy factor applies)
            pv.set_rows(gc, p, 0, cgm, c0, c1);
            const int ob = 1 ^ par(0);  // x parity of row p's black cells
#pragma unroll
            for (int e = 0; e < N; ++e) a0.v[e] = a0.v[e] + pv.value(e, ob, clc);
        }
        W0[sl(0)] = a0;
        // ---- stages 1..4: half-sweep k on row p - k (red, black, red, black) ----
        T ep, en;
        VT o1, o2, o3, o4;
        edges(eslot(0, 2, p - 1), ep, en);
        ys_cells<T, N, CLZ, false>(W0[sl(2)], W0[sl(1)], W0[sl(0)], ep, en, cur.f1, vz, par(1), nby(p - 1), gm, g.nx, xin,
                                   op, o1.v, askd);
        if (!iny(p - 1) || !inx) o1 = vz;
        W1[sl(1)] = o1;
        edges(eslot(S::OFF1, 2, p - 2), ep, en);
        ys_cells<T, N, CLZ, false>(W1[sl(3)], W1[sl(2)], W1[sl(1)], ep, en, cur.f2, vz, 1 ^ par(2), nby(p - 2), gm, g.nx,
                                   xin, op, o2.v, askd);
        if (!iny(p - 2) || !inx) o2 = vz;
        W2[sl(2)] = o2;
        edges(eslot(S::OFF2, 2, p - 3), ep, en);
        ys_cells<T, N, CLZ, false>(W2[sl(4)], W2[sl(3)], W2[sl(2)], ep, en, FR[sl(3)], vz, par(3), nby(p - 3), gm, g.nx,
                                   xin, op, o3.v, askd);
        if (!iny(p - 3) || !inx) o3 = vz;
        W3[sl(3)] = o3;
        edges(eslot(S::OFF3, 4, p - 4), ep, en);
        ys_cells<T, N, CLZ, false>(W3[sl(5)], W3[sl(4)], W3[sl(3)], ep, en, FB[sl(4)], vz, 1 ^ par(4), nby(p - 4), gm,
                                   g.nx, xin, op, o4.v, AS[RS & 1]);
        if (!iny(p - 4) || !inx) o4 = vz;
        W4[sl(4)] = o4;
        // ---- edge writes (slots no stage of this step reads) ----
        put(eslot(0, 2, p), a0);
        put(eslot(S::OFF1, 2, p - 1), o1);
        put(eslot(S::OFF2, 2, p - 2), o2);
        put(eslot(S::OFF3, 4, p - 3), o3);
        if (RR) put(eslot(S::OFF4, 2, p - 4), o4);
        // ---- the smoothed row p - 4: red final after stage 3, black after stage 4 ----
        {
            const int q = p - 4;
            if (q >= Y0 && q < Y0 + yc && tile_x) {
                if (!PRE && ERR) {
#pragma unroll
                    for (int e = 0; e < N; ++e) {
                        const double d0 = (double)W3[sl(4)].v[e] - (double)cur.o0.v[e];
                        const double d1 = (double)o4.v[e] - (double)cur.o1.v[e];
                        err = __builtin_fma(d0, d0, err);
                        err1 = __builtin_fma(d1, d1, err1);
                    }
                }
                T* dp = dst + (int64_t)q * hw + gm;
                if (!RR) vstore<T, N>(dp, W3[sl(4)]);  // PRE's red cells are read by no one (POST loads black)
                vstore<T, N>(dp + Hh, o4);
            }
        }
        // ---- PRE: residual of row p - 5 and the 2 x 2 restriction ----
        if (RR) {
            const int q = p - 5;
            T rred[N], rblk[N];
            T bep, ben, rep = (T)0, ren = (T)0;
            edges(eslot(S::OFF4, 2, q), bep, ben);  // black (stage 4) cells of row q
            ys_cells<T, N, CLZ, true>(W4[sl(6)], W4[sl(5)], W4[sl(4)], bep, ben, FR[sl(5)], W3[sl(5)], par(5), nby(q), gm,
                                      g.nx, xin, op, rred, askd);
            // the black cells' neighbours are the red cells the last step's stage 4 summed (its askew)
            if (kZsRask) {
                ys_cells<T, N, CLZ, true, true>(W3[sl(6)], W3[sl(5)], W3[sl(4)], rep, ren, FB[sl(5)], W4[sl(5)], 1 ^ par(5),
                                                nby(q), gm, g.nx, xin, op, rblk, AS[(RS & 1) ^ 1]);
            } else {
                edges(eslot(S::OFF3, 4, q), rep, ren);  // red (stage 3) cells of row q
                ys_cells<T, N, CLZ, true>(W3[sl(6)], W3[sl(5)], W3[sl(4)], rep, ren, FB[sl(5)], W4[sl(5)], 1 ^ par(5), nby(q),
                                          gm, g.nx, xin, op, rblk, askd);
            }
            if (q >= Y0 && q < Y0 + yc && tile_x) {
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const T r0 = par(5) == 0 ? rred[e] : rblk[e];  // x parity 0 (cell 2I) and 1 (2I + 1)
                    const T r1 = par(5) == 0 ? rblk[e] : rred[e];
                    if (par(5) == 0) {
                        acc[e] = r0 + r1;
                    } else {
                        acc[e] = acc[e] + r0;
                        acc[e] = acc[e] + r1;
                    }
                }
                if (par(5) == 1) {  // coarse row q >> 1 complete
                    const int J = q >> 1;
                    T* rowc = R + (int64_t)J * gc.hw;
#pragma unroll
                    for (int e = 0; e < N; ++e) {
                        const int I = gm + e;
                        rowc[((I + J) & 1) * gc.H + (I >> 1)] = (T)0.25 * acc[e];
                    }
                }
            }
        }
        FR[sl(1)] = cur.f1;
        FB[sl(2)] = cur.f2;
        lds_barrier();
    };

    const std::integral_constant<int, 0> R0;
    const std::integral_constant<int, 1> R1;
    const std::integral_constant<int, 2> R2;
    const std::integral_constant<int, 3> R3;
    if (!PRE) {  // the coarse rows the first fine row needs
        const int J = zlo >> 1;
        for (int k = J - 1; k <= J + 1; ++k) {
            cload(pf[0], k);
            cstore(pf[0], k);
        }
        __syncthreads();
    }
#pragma unroll
    for (int d = 0; d < YS_PF; ++d) prefetch(pf[d], zlo + d);
    for (int p = zlo; p <= p_end; p += 4) {
        step(R0, p);
        if (p + 1 <= p_end) step(R1, p + 1);
        if (p + 2 <= p_end) step(R2, p + 2);
        if (p + 3 <= p_end) step(R3, p + 3);
    }
    if (ERR) block_partial_t<NTL>(err + err1, partials);
}

// (k_tail, k_tail_c: mgp_tail.hip; k_blk: mgp_blk.hip)

// ---- copy-bandwidth probe ("a measured copy-kernel peak is also reported") --------

// Narrow-lane copies (W = 8 or 4 bytes per lane, one pass, 4 elements per thread a workgroup apart): the
// FETCH_SIZE calibration of loads narrower than 16 bytes (tools/fetch_calib.py; mgp_copy_bandwidth runs
// them only under MGP_COPY_CALIB=1).
template <int W>
__global__ __launch_bounds__(kBlock) void k_copy_w(const void* __restrict__ src, void* __restrict__ dst, int64_t n)
{
    typedef float f2v __attribute__((ext_vector_type(2)));
    using E = typename std::conditional<W == 8, f2v, float>::type;
    const E* s = reinterpret_cast<const E*>(src);
    E* d = reinterpret_cast<E*>(dst);
    const int64_t base = (int64_t)blockIdx.x * (4 * kBlock) + threadIdx.x;
    E v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + k * kBlock;
        if (i < n) v[k] = s[i];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + k * kBlock;
        if (i < n) d[i] = v[k];
    }
}

// dst = src in 16-byte lanes.  kind 0: grid-stride, 4 independent loads in flight per thread per
// iteration; kind 1: one pass, each thread 4 vectors a workgroup apart; kind 2: kind 1 with non-temporal
// loads and stores.  The probe reports the fastest.
template <int KIND>
__global__ __launch_bounds__(kBlock) void k_copy16(const float4* __restrict__ src, float4* __restrict__ dst, int64_t n)
{
    if (KIND == 0) {
        const int64_t stride = (int64_t)gridDim.x * kBlock;
        int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        for (; i + 3 * stride < n; i += 4 * stride) {
            const float4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
            dst[i] = a;
            dst[i + stride] = b;
            dst[i + 2 * stride] = c;
            dst[i + 3 * stride] = d;
        }
        for (; i < n; i += stride) dst[i] = src[i];
        return;
    }
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v* s4 = reinterpret_cast<const f4v*>(src);
    f4v* d4 = reinterpret_cast<f4v*>(dst);
    const int64_t base = (int64_t)blockIdx.x * (4 * kBlock) + threadIdx.x;
    f4v v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + k * kBlock;
        if (i < n) v[k] = KIND == 2 ? __builtin_nontemporal_load(s4 + i) : s4[i];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + k * kBlock;
        if (i < n) {
            if (KIND == 2) __builtin_nontemporal_store(v[k], d4 + i);
            else d4[i] = v[k];
        }
    }
}

// ---- reductions -----------------------------------------------------------------------------

// ROUND: each square is first stored into the real-typed errorBuf (cpu-raw.lua:96-100, 249-253)
// PAD: n counts a level's own slots, planes of 2^lp of them at a stride of P (level_slot, mgp_device.h)
template <typename T, bool ROUND = false, bool PAD = false>
__global__ __launch_bounds__(kBlock) void k_sqdiff_partial(const T* __restrict__ a, const T* __restrict__ b,
                                                           int64_t n, double* __restrict__ partials, int lp = 0,
                                                           int64_t P = 0)
{
    double acc = 0.0;
    for (int64_t x = (int64_t)blockIdx.x * kBlock + threadIdx.x; x < n; x += (int64_t)gridDim.x * kBlock) {
        const int64_t c = PAD ? level_slot(x, lp, P) : x;
        const double d = (double)a[c] - (double)b[c];
        acc += ROUND ? (double)(T)(d * d) : d * d;
    }
    block_partial<T>(acc, partials);
}

// calcRelErr + count + calcFrobErr of gpu.lua:173-200 / test-gpu-obj.lua:96-123, 216-247 in one
// pass: per workgroup sum |1 - psi/psiOld| (in real, as errorBuf holds it), the number of nonzero
// errorBuf entries and sum (psi - psiOld)^2, each into its own block of kSumBlocks partials.
template <typename T, bool PAD = false>
__global__ __launch_bounds__(kBlock) void k_metrics_partial(const T* __restrict__ psi, const T* __restrict__ old,
                                                            int64_t n, double* __restrict__ partials, int lp = 0,
                                                            int64_t P = 0)
{
    double rel = 0.0, cnt = 0.0, sq = 0.0;
    for (int64_t x = (int64_t)blockIdx.x * kBlock + threadIdx.x; x < n; x += (int64_t)gridDim.x * kBlock) {
        const int64_t c = PAD ? level_slot(x, lp, P) : x;
        const T p = psi[c], o = old[c];
        const T e = (o != (T)0 && o != p) ? (T)fabs(1.0 - (double)(p / o)) : (T)0;
        if (e != (T)0) {
            rel += (double)e;
            cnt += 1.0;
        }
        const double d = (double)p - (double)o;
        sq += d * d;
    }
    __shared__ double red[3][kBlock];
    red[0][threadIdx.x] = rel;
    red[1][threadIdx.x] = cnt;
    red[2][threadIdx.x] = sq;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int q = 0; q < 3; ++q) partials[q * gridDim.x + blockIdx.x] = red[q][0];
}

// First level of a two-level fixed-order sum: block b sums partials [b*chunk, (b+1)*chunk).
__global__ __launch_bounds__(1024) void k_sum_chunks(const double* __restrict__ partials, int n, int chunk,
                                                     double* __restrict__ out)
{
    __shared__ double sh[1024];
    const int lo = blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double a = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += 1024) a += partials[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// ctr != nullptr: the result goes to out[*ctr] and *ctr advances (a replayed graph fills consecutive
// err slots without a per-cycle copy)
__global__ __launch_bounds__(1024) void k_sum_n(const double* __restrict__ partials, int n, double* __restrict__ out,
                                                int* __restrict__ ctr = nullptr)
{
    __shared__ double sh[1024];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) a += partials[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (ctr) {
            const int k = *ctr;
            out[k] = sh[0];
            *ctr = k + 1;
        } else {
            *out = sh[0];
        }
    }
}

template <typename T>
constexpr int lnv() { return VN<T>::n == 4 ? 2 : 1; }

}  // namespace

// =============================================================================================
// launchers
// =============================================================================================

// (MGP_REAL: mgp_device.h)

hipError_t launch_init_point_charge(int rb, int dim, void* u, void* f, Geo g, int64_t cx, int64_t cy, int64_t cz,
                                    hipStream_t s)
{
    const int64_t n = g.P * g.nz;
    MGP_REAL(rb, (k_init<T><<<nblk_gs(n), kBlock, 0, s>>>((T*)u, (T*)f, g, cx, cy, cz, dim == 3)));
    return hipGetLastError();
}

hipError_t launch_pack(int rb, const void* lex, void* packed, Geo g, hipStream_t s)
{
    const int64_t n = g.P * g.nz;
    MGP_REAL(rb, (k_pack<T><<<nblk_gs(n), kBlock, 0, s>>>((const T*)lex, (T*)packed, g)));
    return hipGetLastError();
}

hipError_t launch_unpack(int rb, const void* packed, void* lex, Geo g, hipStream_t s)
{
    const int64_t n = g.P * g.nz;
    MGP_REAL(rb, (k_unpack<T><<<nblk_gs(n), kBlock, 0, s>>>((const T*)packed, (T*)lex, g)));
    return hipGetLastError();
}

// k_resnorm_z: 3D levels whose rows hold whole vectors and whose planes split into kResZ-plane chunks
static bool resnorm_z_ok(int rb, const Geo& g)
{
    const int n = 16 / rb;
    return g.nz % kResZ == 0 && g.hw >= n && g.hw % n == 0 && g.nx >= 2;
}

int resnorm_blocks(int rb, Geo g)
{
    if (rb == kRealF32D) return (int)nblk(g.P * g.nz);
    const int n = 16 / rb;
    if (resnorm_z_ok(rb, g)) return (int)nblk((int64_t)(g.hw / n) * g.ny * (g.nz / kResZ));
    return (g.hw >= n && g.nx >= 2) ? (int)nblk(2 * (g.H / n) * g.nz) : (int)nblk(g.P * g.nz);
}

template <typename T, int D>
static void resnorm_t(const void* u, const void* f, Geo g, double h, double cl, double* partials, double* out,
                      hipStream_t s)
{
    const Op<T, D> op = make_op<T, D>(h, cl);
    constexpr int n = VN<T>::n;
    const unsigned nb = (unsigned)resnorm_blocks(sizeof(T), g);
    const int fofs = (int)nb + sum_scratch((int)nb);
    if (D == 3 && resnorm_z_ok(sizeof(T), g)) {
        k_resnorm_z<T><<<nb, kBlock, 0, s>>>((const T*)u, (const T*)f, g, make_op<T, 3>(h, cl), partials, fofs);
    } else if (g.hw >= n && g.nx >= 2) {
        const int64_t items = (g.H / n) * g.nz;
        k_resnorm<T, D><<<nb, kBlock, 0, s>>>((const T*)u, (const T*)f, g, op, items, partials, fofs);
    } else {
        k_resnorm_s<T, D><<<nb, kBlock, 0, s>>>((const T*)u, (const T*)f, g, op, partials, fofs);
    }
    // the two rows of partials (sum r^2, sum f^2), each to one value in fixed order
    (void)launch_sum_partials(partials, (int)nb, out, s);
    (void)launch_sum_partials(partials + fofs, (int)nb, out + 1, s);
}

hipError_t launch_residual_norm(int rb, int dim, const void* u, const void* f, Geo g, double h, double cl,
                                double* partials, double* out, hipStream_t s)
{
    if (rb == kRealF32D) {  // the scalar form, r evaluated in double (resnorm_blocks(kRealF32D) counts it)
        const unsigned nb = (unsigned)resnorm_blocks(rb, g);
        const int fofs = (int)nb + sum_scratch((int)nb);
        if (dim == 3)
            k_resnorm_s<float, 3, double><<<nb, kBlock, 0, s>>>((const float*)u, (const float*)f, g,
                                                                make_op<double, 3>(h, cl), partials, fofs);
        else
            k_resnorm_s<float, 2, double><<<nb, kBlock, 0, s>>>((const float*)u, (const float*)f, g,
                                                                make_op<double, 2>(h, cl), partials, fofs);
        (void)launch_sum_partials(partials, (int)nb, out, s);
        (void)launch_sum_partials(partials + fofs, (int)nb, out + 1, s);
        return hipGetLastError();
    }
    if (rb == 8) {
        if (dim == 3) resnorm_t<double, 3>(u, f, g, h, cl, partials, out, s);
        else resnorm_t<double, 2>(u, f, g, h, cl, partials, out, s);
    } else {
        if (dim == 3) resnorm_t<float, 3>(u, f, g, h, cl, partials, out, s);
        else resnorm_t<float, 2>(u, f, g, h, cl, partials, out, s);
    }
    return hipGetLastError();
}

hipError_t launch_residual_field(int rb, int dim, const void* u, const void* f, void* r, Geo g, double h, double cl,
                                 hipStream_t s)
{
    const unsigned nb = nblk_gs(g.P * g.nz);
    if (rb == kRealF32D) {
        if (dim == 3) k_residual_field<float, 3, double><<<nb, kBlock, 0, s>>>((const float*)u, (const float*)f, (float*)r, g, make_op<double, 3>(h, cl));
        else k_residual_field<float, 2, double><<<nb, kBlock, 0, s>>>((const float*)u, (const float*)f, (float*)r, g, make_op<double, 2>(h, cl));
        return hipGetLastError();
    }
    if (rb == 8) {
        if (dim == 3) k_residual_field<double, 3><<<nb, kBlock, 0, s>>>((const double*)u, (const double*)f, (double*)r, g, make_op<double, 3>(h, cl));
        else k_residual_field<double, 2><<<nb, kBlock, 0, s>>>((const double*)u, (const double*)f, (double*)r, g, make_op<double, 2>(h, cl));
    } else {
        if (dim == 3) k_residual_field<float, 3><<<nb, kBlock, 0, s>>>((const float*)u, (const float*)f, (float*)r, g, make_op<float, 3>(h, cl));
        else k_residual_field<float, 2><<<nb, kBlock, 0, s>>>((const float*)u, (const float*)f, (float*)r, g, make_op<float, 2>(h, cl));
    }
    return hipGetLastError();
}

hipError_t launch_sqdiff_field(int rb, const void* a, const void* b, void* out, int64_t n, hipStream_t s)
{
    if (rb == kRealF32D) {
        k_sqdiff_field<float, double><<<nblk_gs(n), kBlock, 0, s>>>((const float*)a, (const float*)b, (float*)out, n);
        return hipGetLastError();
    }
    MGP_REAL(rb, (k_sqdiff_field<T><<<nblk_gs(n), kBlock, 0, s>>>((const T*)a, (const T*)b, (T*)out, n)));
    return hipGetLastError();
}

hipError_t launch_field_stats(int rb, const void* packed, Geo g, uint64_t* hpart, double* dpart, uint64_t* out_h,
                              double* out_d, hipStream_t s)
{
    const int nb = kSumBlocks;
    if (g.P != 2 * g.H) MGP_REAL(rb, (k_field_stats<T, true><<<nb, kBlock, 0, s>>>((const T*)packed, g, hpart, dpart)));
    else MGP_REAL(rb, (k_field_stats<T><<<nb, kBlock, 0, s>>>((const T*)packed, g, hpart, dpart)));
    k_field_stats_final<<<1, kBlock, 0, s>>>(hpart, dpart, nb, out_h, out_d);
    return hipGetLastError();
}

static bool half_vector(int rb, const Geo& g) { return g.hw >= 16 / rb && g.nx >= 2; }

static int64_t half_items(int rb, const Geo& g)
{
    const int n = 16 / rb;
    return half_vector(rb, g) ? (g.H / n) * g.nz : g.H * g.nz;
}

static bool half_gs(int rb, const Geo& g, bool gs)
{
    return gs && half_vector(rb, g) && half_items(rb, g) >= (int64_t)kGsBlocks * kBlock * 2;
}

int half_blocks(int rb, Geo g, bool gs)
{
    if (rb == kRealF32D) return (int)nblk(g.H * g.nz);  // scalar k_half_s
    return half_gs(rb, g, gs) ? kGsBlocks : (int)nblk(half_items(rb, g));
}

template <typename T, int D>
static void half_t(bool fine, bool err, bool vec, bool gs, unsigned nb, int color, const void* other, const void* f, void* dst,
                   const void* old, double* partials, Geo g, double h, double cl, bool nt, hipStream_t s)
{
    const Op<T, D> op = make_op<T, D>(h, cl);
    const T* o_ = (const T*)other;
    const T* f_ = (const T*)f;
    T* d_ = (T*)dst;
    const T* w_ = (const T*)old;
    if (vec && gs && half_gs(sizeof(T), g, gs)) {
        const int64_t items = half_items(sizeof(T), g);
        if (fine) {
            if (err) k_half_gs<T, D, 1, true><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op, items);
            else k_half_gs<T, D, 1, false><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op, items);
        } else {
            if (err) k_half_gs<T, D, 0, true><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op, items);
            else k_half_gs<T, D, 0, false><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op, items);
        }
    } else if (vec) {
        if (fine && nt) {
            if (err) k_half<T, D, 2, true><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op);
            else k_half<T, D, 2, false><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op);
        } else if (fine) {
            if (err) k_half<T, D, 1, true><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op);
            else k_half<T, D, 1, false><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op);
        } else {
            if (err) k_half<T, D, 0, true><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op);
            else k_half<T, D, 0, false><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op);
        }
    } else {
        if (err) k_half_s<T, D, true><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op);
        else k_half_s<T, D, false><<<nb, kBlock, 0, s>>>(o_, f_, d_, w_, partials, g, color, op);
    }
}

// cpu-raw.lua's float arithmetic: a thread per slot, evaluated in double, stored as float
template <int D>
static void half_f32d(bool err, unsigned nb, int color, const void* other, const void* f, void* dst, const void* old,
                      double* partials, Geo g, double h, double cl, hipStream_t s)
{
    const Op<double, D> op = make_op<double, D>(h, cl);
    const float *o_ = (const float*)other, *f_ = (const float*)f, *w_ = (const float*)old;
    if (err) k_half_s<float, D, true, double><<<nb, kBlock, 0, s>>>(o_, f_, (float*)dst, w_, partials, g, color, op);
    else k_half_s<float, D, false, double><<<nb, kBlock, 0, s>>>(o_, f_, (float*)dst, w_, partials, g, color, op);
}

PieceTuning piece_tuning_from_env()
{
    PieceTuning t;
    if (const char* v = std::getenv("MGP_RR_SCALAR_CELLS")) t.rr_scalar_cells = std::atoll(v), t.rr_scalar_env = true;
    if (const char* v = std::getenv("MGP_RR_PAIR_CELLS")) t.rr_pair_cells = std::atoll(v);
    if (const char* v = std::getenv("MGP_BRES_VN")) t.bres_vn = std::atoi(v);
    if (const char* v = std::getenv("MGP_NT")) t.nt = std::atoi(v) != 0;
    return t;
}

hipError_t launch_half_sweep(int rb, int dim, bool fine, int color, const void* other, const void* f, void* dst,
                             const void* old, double* partials, Geo g, double h, double cl, bool gs,
                             const PieceTuning& pt, hipStream_t s)
{
    const unsigned nb = (unsigned)half_blocks(rb, g, gs);
    if (rb == kRealF32D) {
        if (dim == 3) half_f32d<3>(old != nullptr, nb, color, other, f, dst, old, partials, g, h, cl, s);
        else half_f32d<2>(old != nullptr, nb, color, other, f, dst, old, partials, g, h, cl, s);
        return hipGetLastError();
    }
    const bool err = old != nullptr, vec = half_vector(rb, g);
    if (rb == 8) {
        if (dim == 3) half_t<double, 3>(fine, err, vec, gs, nb, color, other, f, dst, old, partials, g, h, cl, pt.nt, s);
        else half_t<double, 2>(fine, err, vec, gs, nb, color, other, f, dst, old, partials, g, h, cl, pt.nt, s);
    } else {
        if (dim == 3) half_t<float, 3>(fine, err, vec, gs, nb, color, other, f, dst, old, partials, g, h, cl, pt.nt, s);
        else half_t<float, 2>(fine, err, vec, gs, nb, color, other, f, dst, old, partials, g, h, cl, pt.nt, s);
    }
    return hipGetLastError();
}

template <typename T, int D>
static hipError_t fresh_t(const void* f, void* u, Geo g, double h, double cl, bool red, hipStream_t s)
{
    const int64_t items = half_items(sizeof(T), g);
    if (red) k_fresh<T, D, true><<<nblk(items), kBlock, 0, s>>>((const T*)f, (T*)u, g, make_op<T, D>(h, cl));
    else k_fresh<T, D, false><<<nblk(items), kBlock, 0, s>>>((const T*)f, (T*)u, g, make_op<T, D>(h, cl));
    return hipGetLastError();
}

bool fresh_supported(int rb, const Geo& g) { return half_vector(rb, g); }

template <typename T, int D>
static hipError_t post1_t(int linear, void* u, const void* V, const void* f, Geo g, Geo gc, double h, double cl,
                          double clc, hipStream_t s)
{
    const int64_t items = half_items(sizeof(T), g);
    const Op<T, D> op = make_op<T, D>(h, cl);
    if (linear) k_post1<T, D, 1><<<nblk(items), kBlock, 0, s>>>((T*)u, (const T*)V, (const T*)f, g, gc, op, (T)clc);
    else k_post1<T, D, 0><<<nblk(items), kBlock, 0, s>>>((T*)u, (const T*)V, (const T*)f, g, gc, op, (T)clc);
    return hipGetLastError();
}

// the red cells of a row segment and their black neighbours' coarse rows come in whole vectors
bool post1_supported(int rb, const Geo& g, const Geo& gc)
{
    const int n = 16 / rb;
    return half_vector(rb, g) && gc.nx >= n && 2 * gc.nx == g.nx && g.z0 == 0 && g.gnz == g.nz;
}

hipError_t launch_post_first(int rb, int dim, int linear, void* u, const void* V, const void* f, Geo g, Geo gc,
                             double h, double cl, double clc, hipStream_t s)
{
    if (!post1_supported(rb, g, gc)) return hipErrorInvalidValue;
    if (rb == 8)
        return dim == 3 ? post1_t<double, 3>(linear, u, V, f, g, gc, h, cl, clc, s)
                        : post1_t<double, 2>(linear, u, V, f, g, gc, h, cl, clc, s);
    return dim == 3 ? post1_t<float, 3>(linear, u, V, f, g, gc, h, cl, clc, s)
                    : post1_t<float, 2>(linear, u, V, f, g, gc, h, cl, clc, s);
}

hipError_t launch_fresh_sweep(int rb, int dim, const void* f, void* u, Geo g, double h, double cl, hipStream_t s,
                              bool store_red)
{
    if (!fresh_supported(rb, g)) return hipErrorInvalidValue;
    if (rb == 8)
        return dim == 3 ? fresh_t<double, 3>(f, u, g, h, cl, store_red, s) : fresh_t<double, 2>(f, u, g, h, cl, store_red, s);
    return dim == 3 ? fresh_t<float, 3>(f, u, g, h, cl, store_red, s) : fresh_t<float, 2>(f, u, g, h, cl, store_red, s);
}

template <typename T, int D>
static void rr_t(const void* u, const void* f, void* R, Geo g, Geo gc, double h, double cl, const PieceTuning& pt,
                 hipStream_t s)
{
    const Op<T, D> op = make_op<T, D>(h, cl);
    constexpr int n = VN<T>::n;
    const int cx = g.nx / 2;
    const int64_t ncz = D == 3 ? g.nz / 2 : 1;
    // below 2^22 coarse cells one thread per coarse cell (more parallelism, shorter per-thread
    // chains) beats n cells along x: 256^3 -> 128^3 and below, 1.609 -> 1.570 ms per 512^3 cycle
    const int64_t scalar_below = pt.rr_scalar_cells;  // (MGP_RR_SCALAR_CELLS)
    // from MGP_RR_PAIR_CELLS coarse cells up to scalar_below: two coarse cells per thread (default: 2D from 2^18,
    // the 2048^2 level of configs[1]: cycle 0.2655 -> 0.2604 ms; 3D off, neutral at 512^3)
    const int64_t pair_env = pt.rr_pair_cells;
    const int64_t pair_from = pair_env >= 0 ? pair_env : (D == 2 ? (int64_t)1 << 18 : INT64_MAX);
    const int64_t ccells = (int64_t)cx * (g.ny / 2) * ncz;
    if (cx >= n && ccells >= scalar_below) {
        const int64_t items = (int64_t)(cx / n) * (g.ny / 2) * ncz;
        k_resrestrict<T, D><<<nblk(items), kBlock, 0, s>>>((const T*)u, (const T*)f, (T*)R, g, gc, op);
    } else if (n > 2 && cx >= 2 && ccells >= pair_from) {
        const int64_t items = (int64_t)(cx / 2) * (g.ny / 2) * ncz;
        k_resrestrict<T, D, 2><<<nblk(items), kBlock, 0, s>>>((const T*)u, (const T*)f, (T*)R, g, gc, op);
    } else {
        const int64_t items = (int64_t)cx * (g.ny / 2) * ncz;
        k_resrestrict_s<T, D><<<nblk(items), kBlock, 0, s>>>((const T*)u, (const T*)f, (T*)R, g, gc, op);
    }
}

hipError_t launch_residual_restrict(int rb, int dim, const void* u, const void* f, void* R, Geo g, Geo gc, double h,
                                    double cl, const PieceTuning& pt, hipStream_t s)
{
    if (rb == kRealF32D) {
        const int64_t items = (int64_t)(g.nx / 2) * (g.ny / 2) * (dim == 3 ? g.nz / 2 : 1);
        if (dim == 3)
            k_resrestrict_s<float, 3, double><<<nblk(items), kBlock, 0, s>>>((const float*)u, (const float*)f, (float*)R, g,
                                                                            gc, make_op<double, 3>(h, cl));
        else
            k_resrestrict_s<float, 2, double><<<nblk(items), kBlock, 0, s>>>((const float*)u, (const float*)f, (float*)R, g,
                                                                            gc, make_op<double, 2>(h, cl));
        return hipGetLastError();
    }
    if (rb == 8) {
        if (dim == 3) rr_t<double, 3>(u, f, R, g, gc, h, cl, pt, s);
        else rr_t<double, 2>(u, f, R, g, gc, h, cl, pt, s);
    } else {
        if (dim == 3) rr_t<float, 3>(u, f, R, g, gc, h, cl, pt, s);
        else rr_t<float, 2>(u, f, R, g, gc, h, cl, pt, s);
    }
    return hipGetLastError();
}

template <typename T, int D>
static void resfield_t(const void* u, const void* f, void* r, Geo g, double h, double cl, hipStream_t s)
{
    const Op<T, D> op = make_op<T, D>(h, cl);
    if (half_vector(sizeof(T), g)) {
        const int64_t items = half_items(sizeof(T), g);
        k_resfield_v<T, D><<<nblk(2 * items), kBlock, 0, s>>>((const T*)u, (const T*)f, (T*)r, g, op, items);
    } else {
        k_residual_field<T, D><<<nblk_gs(g.P * g.nz), kBlock, 0, s>>>((const T*)u, (const T*)f, (T*)r, g, op);
    }
}

hipError_t launch_residual_field_v(int rb, int dim, const void* u, const void* f, void* r, Geo g, double h, double cl,
                                   hipStream_t s)
{
    if (rb == kRealF32D) return launch_residual_field(rb, dim, u, f, r, g, h, cl, s);
    if (rb == 8) {
        if (dim == 3) resfield_t<double, 3>(u, f, r, g, h, cl, s);
        else resfield_t<double, 2>(u, f, r, g, h, cl, s);
    } else {
        if (dim == 3) resfield_t<float, 3>(u, f, r, g, h, cl, s);
        else resfield_t<float, 2>(u, f, r, g, h, cl, s);
    }
    return hipGetLastError();
}

template <typename T, int D>
static void fw_t(const void* r, void* R, Geo g, Geo gc, double clc, hipStream_t s)
{
    constexpr int n = VN<T>::n;
    const int cx = g.nx / 2;
    const int64_t ncz = D == 3 ? g.nz / 2 : 1;
    const T wf = (T)3 - (T)clc;
    if (cx >= n) {
        const int64_t items = (int64_t)(cx / n) * (g.ny / 2) * ncz;
        k_fw_v<T, D><<<nblk(items), kBlock, 0, s>>>((const T*)r, (T*)R, g, gc, wf);
    } else {
        const int64_t items = (int64_t)cx * (g.ny / 2) * ncz;
        k_fw_s<T, D><<<nblk(items), kBlock, 0, s>>>((const T*)r, (T*)R, g, gc, wf);
    }
}

hipError_t launch_fw_restrict(int rb, int dim, const void* r, void* R, Geo g, Geo gc, double clc, hipStream_t s)
{
    if (rb == kRealF32D) {
        const int64_t items = (int64_t)(g.nx / 2) * (g.ny / 2) * (dim == 3 ? g.nz / 2 : 1);
        const double wf = 3.0 - clc;
        if (dim == 3) k_fw_s<float, 3, double><<<nblk(items), kBlock, 0, s>>>((const float*)r, (float*)R, g, gc, wf);
        else k_fw_s<float, 2, double><<<nblk(items), kBlock, 0, s>>>((const float*)r, (float*)R, g, gc, wf);
        return hipGetLastError();
    }
    if (rb == 8) {
        if (dim == 3) fw_t<double, 3>(r, R, g, gc, clc, s);
        else fw_t<double, 2>(r, R, g, gc, clc, s);
    } else {
        if (dim == 3) fw_t<float, 3>(r, R, g, gc, clc, s);
        else fw_t<float, 2>(r, R, g, gc, clc, s);
    }
    return hipGetLastError();
}

template <typename T, int D>
static hipError_t pr_t(int linear, void* u, const void* V, Geo g, Geo gc, double clc, bool black, hipStream_t s)
{
    constexpr int n = VN<T>::n;
    if (gc.nx >= n) {
        const int64_t items = (int64_t)(gc.nx / n) * g.ny * g.nz;
        const unsigned nb = nblk(items);
        if (black) {
            if (linear) k_prolong_v<T, D, 1, true><<<nb, kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, (T)clc);
            else k_prolong_v<T, D, 0, true><<<nb, kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, (T)clc);
        } else {
            if (linear) k_prolong_v<T, D, 1><<<nb, kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, (T)clc);
            else k_prolong_v<T, D, 0><<<nb, kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, (T)clc);
        }
        return hipGetLastError();
    }
    for (int color = black ? 1 : 0; color < 2; ++color) {
        const unsigned nb = nblk(g.H * g.nz);
        if (linear) k_prolong<T, D, 1><<<nb, kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, clc, color);
        else k_prolong<T, D, 0><<<nb, kBlock, 0, s>>>((T*)u, (const T*)V, g, gc, clc, color);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int D>
static hipError_t pr_f32d(int linear, void* u, const void* V, Geo g, Geo gc, double clc, bool black, hipStream_t s)
{
    for (int color = black ? 1 : 0; color < 2; ++color) {
        const unsigned nb = nblk(g.H * g.nz);
        if (linear) k_prolong<float, D, 1, double><<<nb, kBlock, 0, s>>>((float*)u, (const float*)V, g, gc, clc, color);
        else k_prolong<float, D, 0, double><<<nb, kBlock, 0, s>>>((float*)u, (const float*)V, g, gc, clc, color);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_prolong_correct(int rb, int dim, int linear, void* u, const void* V, Geo g, Geo gc, double clc,
                                  hipStream_t s, bool black_only)
{
    if (rb == kRealF32D)
        return dim == 3 ? pr_f32d<3>(linear, u, V, g, gc, clc, black_only, s) : pr_f32d<2>(linear, u, V, g, gc, clc, black_only, s);
    if (rb == 8)
        return dim == 3 ? pr_t<double, 3>(linear, u, V, g, gc, clc, black_only, s)
                        : pr_t<double, 2>(linear, u, V, g, gc, clc, black_only, s);
    return dim == 3 ? pr_t<float, 3>(linear, u, V, g, gc, clc, black_only, s)
                    : pr_t<float, 2>(linear, u, V, g, gc, clc, black_only, s);
}

// ---- the stage-split fused launches and the 2D phases (called by fused_dispatch / launch_fused, mgp_zs.hip) ----

// PRE with the 2^3-average restriction, fp32, cl = 0: the stage-split kernel (ZSRC: a fresh zero guess)
template <bool ZSRC>
static hipError_t zs_split_launch(const FusedArgs& a, hipStream_t s)
{
    using SP = ZsSplit<float>;
    const Op<float, 3> op = make_op<float, 3>(a.h, a.cl);
    const ZsGrid gr = zs_grid<SP::S>(a, true, SP::NTL);
    if (a.info) std::snprintf(a.info->name, sizeof a.info->name, "k_zs_split<float, %s>", tf(ZSRC));
    k_zs_split<float, ZSRC><<<gr.nb, SP::NTL, SP::lds_bytes, s>>>((const float*)a.src, (const float*)a.f, (float*)a.dst,
                                                                   (float*)a.R, a.g, a.gc, op, a.zc, a.ghost, gr.patch);
    return hipGetLastError();
}

hipError_t launch_zs_split(const FusedArgs& a, hipStream_t s)
{
    return a.src ? zs_split_launch<false>(a, s) : zs_split_launch<true>(a, s);
}

// The same on a level with a boundary-modified operator (cl != 0), from a fresh zero guess
hipError_t launch_zs_split_cl(const FusedArgs& a, hipStream_t s)
{
    using SP = ZsSplit<float>;
    const Op<float, 3> op = make_op<float, 3>(a.h, a.cl);
    const ZsGrid gr = zs_grid<SP::S>(a, true, SP::NTL);
    if (a.info) std::snprintf(a.info->name, sizeof a.info->name, "k_zs_split_cl<float>");
    k_zs_split_cl<float><<<gr.nb, SP::NTL, SP::lds_bytes, s>>>((const float*)a.f, (float*)a.dst, (float*)a.R, a.g, a.gc, op,
                                                              a.zc, a.ghost, gr.patch);
    return hipGetLastError();
}

// POST with trilinear prolongation, fp32, cl = 0, on the wide tile: the stage-split kernel (fused_dispatch: levels of
// at least FusedTuning::split_post_min_cells cells).  Its tile, its workgroups and their order are k_zs's.
template <bool ERR>
static hipError_t zs_split_post_launch(const FusedArgs& a, hipStream_t s)
{
    using SP = ZsSplitPost<float>;
    static_assert(ZsSplitPost<float>::S::TX == ZsTile<float>::TXPOST_W && ZsSplitPost<float>::S::TY == ZsTile<float>::TYPOST_W,
                  "the split POST runs on the wide tile");
    const Op<float, 3> op = make_op<float, 3>(a.h, a.cl);
    const ZsGrid gr = zs_grid<SP::S>(a, false, SP::NTL);
    if (a.info) std::snprintf(a.info->name, sizeof a.info->name, "k_zs_split_post<float, %s>", tf(ERR));
    k_zs_split_post<float, ERR><<<gr.nb, SP::NTL, SP::lds_bytes, s>>>(
        (const float*)a.src, (const float*)a.f, (float*)a.dst, (const float*)(a.old ? a.old : a.dst), (const float*)a.V,
        a.partials, a.g, a.gc, op, (float)a.clc, a.zc, a.ghost, gr.patch);
    return hipGetLastError();
}

hipError_t launch_zs_split_post(const FusedArgs& a, hipStream_t s)
{
    return a.partials ? zs_split_post_launch<true>(a, s) : zs_split_post_launch<false>(a, s);
}

hipError_t zs_split_attr(int rb)
{
    if (rb != 4) return hipSuccess;  // fp32 only
    const auto A = hipFuncAttributeMaxDynamicSharedMemorySize;
    const int w = (int)ZsSplit<float>::lds_bytes;
    hipError_t e = hipFuncSetAttribute((const void*)k_zs_split<float, false>, A, w);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs_split<float, true>, A, w);
    const int wp = (int)ZsSplitPost<float>::lds_bytes;
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs_split_post<float, true>, A, wp);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs_split_post<float, false>, A, wp);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_zs_split_cl<float>, A, w);
    return e;
}

// 2D (k_ys): rows per z-chunk of a workgroup (FusedTuning::ys_rows, default 32; even)
int ys_rows(const Geo& g, const FusedTuning& tu)
{
    int r = tu.ys_rows;
    while (r > 8 && g.ny % r != 0) r /= 2;
    return r;
}

// segment width of a 2D level: the full width, or half of it when the full width gives fewer than
// FusedTuning::wgs (default 256) workgroups (FusedTuning::ys_half: -1 that rule, 0 never, 1 always)
int ys_tx(int rb, const Geo& g, const FusedTuning& tu)
{
    const int mode = tu.ys_half;
    const int64_t target = tu.wgs;
    const int full = rb == 4 ? ys_tx_full<float>() : ys_tx_full<double>();
    if (mode == 0 || g.nx % (full / 2) != 0) return full;
    if (mode == 1 || g.nx % full != 0) return full / 2;
    return (int64_t)(g.nx / full) * (g.ny / ys_rows(g, tu)) < target ? full / 2 : full;
}

template <typename T, bool PRE, int LINEAR, bool ERR, bool CLZ, int TXV>
static hipError_t ys_launch_tx(const FusedArgs& a, hipStream_t s)
{
    using S = YsShape<T, PRE, TXV>;
    const Op<T, 2> op = make_op<T, 2>(a.h, a.cl);
    const unsigned nb = (unsigned)((a.g.nx / S::TX) * (a.g.ny / a.zc));
    if (a.info) {
        std::snprintf(a.info->name, sizeof a.info->name, "k_ys<%s, %s, %d, %s, %s, %d>", sizeof(T) == 4 ? "float" : "double",
                      tf(PRE), LINEAR, tf(ERR), tf(CLZ), TXV);
        a.info->grid = (int64_t)nb * S::NTL;
    }
    k_ys<T, PRE, LINEAR, ERR, CLZ, TXV><<<nb, S::NTL, 0, s>>>((const T*)a.src, (const T*)a.f, (T*)a.dst,
                                                         (const T*)(a.old ? a.old : a.dst), (T*)a.R, (const T*)a.V,
                                                         a.partials, a.g, a.gc, op, (T)a.clc, a.zc);
    return hipGetLastError();
}

template <typename T, bool PRE, int LINEAR, bool ERR, bool CLZ>
static hipError_t ys_launch(const FusedArgs& a, hipStream_t s)
{
    constexpr int F = ys_tx_full<T>();
    return ys_tx(sizeof(T), a.g, a.tu) == F ? ys_launch_tx<T, PRE, LINEAR, ERR, CLZ, F>(a, s)
                                      : ys_launch_tx<T, PRE, LINEAR, ERR, CLZ, F / 2>(a, s);
}

template <typename T, bool CLZ>
static hipError_t fused_dispatch_2d(const FusedArgs& a, hipStream_t s)
{
    const bool err = a.partials != nullptr;
    if (a.pre) return a.linear ? ys_launch<T, true, 1, false, CLZ>(a, s) : ys_launch<T, true, 0, false, CLZ>(a, s);
    if (a.linear) return err ? ys_launch<T, false, 1, true, CLZ>(a, s) : ys_launch<T, false, 1, false, CLZ>(a, s);
    return err ? ys_launch<T, false, 0, true, CLZ>(a, s) : ys_launch<T, false, 0, false, CLZ>(a, s);
}

hipError_t launch_fused_2d(int rb, const FusedArgs& a, hipStream_t s)
{
    const bool clz = a.cl == 0.0;
    if (rb == 4) return clz ? fused_dispatch_2d<float, true>(a, s) : fused_dispatch_2d<float, false>(a, s);
    return clz ? fused_dispatch_2d<double, true>(a, s) : fused_dispatch_2d<double, false>(a, s);
}

hipError_t launch_copy16(int kind, const void* src, void* dst, int64_t bytes, hipStream_t s)
{
    const int64_t n = bytes / 16;
    const unsigned one_pass = (unsigned)((n + 4 * kBlock - 1) / (4 * kBlock));
    if (kind == 0) k_copy16<0><<<2048, kBlock, 0, s>>>((const float4*)src, (float4*)dst, n);
    else if (kind == 1) k_copy16<1><<<one_pass, kBlock, 0, s>>>((const float4*)src, (float4*)dst, n);
    else if (kind == 2) k_copy16<2><<<one_pass, kBlock, 0, s>>>((const float4*)src, (float4*)dst, n);
    else if (kind == 3) k_copy_w<8><<<one_pass * 2, kBlock, 0, s>>>(src, dst, n * 2);
    else k_copy_w<4><<<one_pass * 4, kBlock, 0, s>>>(src, dst, n * 4);
    return hipGetLastError();
}

hipError_t launch_sqdiff_sum(int rb, const void* a, const void* b, int64_t n, double* partials, double* out,
                             hipStream_t s, int* ctr, const Geo* lev)
{
    const bool pad = lev && lev->P != 2 * lev->H;
    const int lp = pad ? lev->lhw + lev->ly + 1 : 0;
    const int64_t P = pad ? lev->P : 0;
    if (pad) n = n / P * 2 * lev->H;
    if (rb == kRealF32D) {  // cpu-raw.lua's float errorBuf: each square rounded to float before the sum
        if (pad)
            k_sqdiff_partial<float, true, true><<<kSumBlocks, kBlock, 0, s>>>((const float*)a, (const float*)b, n,
                                                                              partials, lp, P);
        else k_sqdiff_partial<float, true><<<kSumBlocks, kBlock, 0, s>>>((const float*)a, (const float*)b, n, partials);
    } else if (pad) {
        MGP_REAL(rb, (k_sqdiff_partial<T, false, true><<<kSumBlocks, kBlock, 0, s>>>((const T*)a, (const T*)b, n,
                                                                                    partials, lp, P)));
    } else {
        MGP_REAL(rb, (k_sqdiff_partial<T><<<kSumBlocks, kBlock, 0, s>>>((const T*)a, (const T*)b, n, partials)));
    }
    k_sum_n<<<1, 1024, 0, s>>>(partials, kSumBlocks, out, ctr);
    return hipGetLastError();
}

hipError_t launch_metrics(int rb, const void* psi, const void* old, int64_t n, double* partials, double* out,
                          hipStream_t s, const Geo* lev)
{
    if (lev && lev->P != 2 * lev->H) {
        const int64_t nl = n / lev->P * 2 * lev->H;
        MGP_REAL(rb, (k_metrics_partial<T, true><<<kSumBlocks, kBlock, 0, s>>>((const T*)psi, (const T*)old, nl, partials,
                                                                              lev->lhw + lev->ly + 1, lev->P)));
    } else {
        MGP_REAL(rb, (k_metrics_partial<T><<<kSumBlocks, kBlock, 0, s>>>((const T*)psi, (const T*)old, n, partials)));
    }
    for (int q = 0; q < 3; ++q) k_sum_n<<<1, 1024, 0, s>>>(partials + q * kSumBlocks, kSumBlocks, out + q);
    return hipGetLastError();
}

// ---- test hook of the communication deadline (mgp_api.cpp stream_wait; MGP_TEST_STALL) ----

// One wave polls a host-pinned flag with system-scope vector loads (never the scalar cache) and leaves when it is
// set or after max_ticks of the 100 MHz wall clock: a stream held like an exchange whose peer never arrives.
__global__ __launch_bounds__(64) void k_stall(const int* flag, uint64_t max_ticks)
{
    const uint64_t t0 = wall_clock64();
    const int* p = flag + (threadIdx.x >> 6);  // a per-lane (VGPR) address
    while (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0 && wall_clock64() - t0 < max_ticks)
        __builtin_amdgcn_s_sleep(127);
}

hipError_t launch_stall(const int* flag, double max_s, hipStream_t s)
{
    int khz = 0;  // wall clock rate in kHz (100 MHz on CDNA)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess ||
        khz <= 0)
        khz = 100000;
    const uint64_t ticks = (uint64_t)(std::min(max_s, 120.0) * 1e3 * khz);
    k_stall<<<1, 64, 0, s>>>(flag, ticks);
    return hipGetLastError();
}

// The reference's debugging check (cpu-raw.lua:135-139, gpu.lua:279-283: error "found a nan" when a dumped grid
// holds a non-finite cell): any cell of p[0, n) with an all-ones exponent lowers *first to `id`, the check's
// position in the cycle, so the host names the first phase that produced one.  16-byte loads, grid-stride.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_nonfinite(const T* __restrict__ p, int64_t n, int id, int* first, bool vec)
{
    using U = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;
    constexpr U kExp = sizeof(T) == 8 ? (U)0x7ff0000000000000ull : (U)0x7f800000u;
    constexpr int V = 16 / sizeof(T);
    const int64_t nv = vec ? n / V : 0;  // (vec: p is 16-byte aligned)
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nv; i += stride) {
        const uint4 q = reinterpret_cast<const uint4*>(p)[i];
        const U* w = reinterpret_cast<const U*>(&q);
#pragma unroll
        for (int k = 0; k < V; ++k) bad = bad || (w[k] & kExp) == kExp;
    }
    for (int64_t i = nv * V + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        U w;
        __builtin_memcpy(&w, p + i, sizeof(U));
        bad = bad || (w & kExp) == kExp;
    }
    if (bad) atomicMin(first, id);
}

hipError_t launch_nonfinite_check(int rb, const void* p, int64_t n, int id, int* first, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const int64_t want = (n / (16 / (rb == 8 ? 8 : 4)) + kBlock - 1) / kBlock;
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, 2048));
    MGP_REAL(rb, (k_nonfinite<T><<<nb, kBlock, 0, s>>>((const T*)p, n, id, first, ((uintptr_t)p & 15) == 0)));
    return hipGetLastError();
}

// one fixed-order kernel up to 65536 partials (64 per thread), two levels beyond
int sum_scratch(int n) { return n <= 65536 ? 0 : (n + 8191) / 8192; }

hipError_t launch_sum_partials(const double* partials, int n, double* out, hipStream_t s, int* ctr)
{
    const int nb = sum_scratch(n);
    if (nb == 0) {
        k_sum_n<<<1, 1024, 0, s>>>(partials, n, out, ctr);
    } else {
        // two fixed-order levels; the first level's sums go right after the partials
        double* mid = const_cast<double*>(partials) + n;
        k_sum_chunks<<<nb, 1024, 0, s>>>(partials, n, 8192, mid);
        k_sum_n<<<1, 1024, 0, s>>>(mid, nb, out, ctr);
    }
    return hipGetLastError();
}

}  // namespace mgp
