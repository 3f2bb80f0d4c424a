// mgp_blk.hip — the tiled smoothing phases of small levels (k_blk: one launch per phase, the tile and its halo in
// LDS), their launcher and dynamic-LDS attributes.  Two consecutive 2D levels in one launch: mgp_blk2.hip.
#include "mgp_cell.h"

namespace mgp {
namespace {

// ---- 3D-tiled smoothing phases of small levels (k_blk) ----------------------------------------
//
// Below ~128^3 a launch costs more than its work (≈5 us per kernel, most of it the kernel
// boundary), so a smoothing phase of nu RB-GS sweeps runs as ONE launch instead of 2 nu + 1:
//   PRE : nu sweeps of src, then residual + restriction   (smooth(l, nu1) + residual_restrict(l))
//   POST: src + P V, then nu sweeps                        (prolong_correct(l) + smooth(l, nu2))
// A workgroup owns a tx x ty x tz tile, loads it with a halo of E = 2 nu + 1 (PRE) / 2 nu (POST)
// cells (x halo rounded up to even so the LDS rows keep the global red/black packing) into LDS,
// and runs the half-sweeps there on a region that shrinks by one cell per half-sweep (the halo is
// recomputed redundantly by the neighbouring tiles with the same arithmetic), one barrier each.
// Only black cells of the input are read (Gauss-Seidel never reads the value it replaces: the red
// half-sweep overwrites the red ones); cells outside the box are 0 in LDS and never written.
// Every expression is half_item's / resrestrict_item's / prolong_value's, so the result is
// bit-identical to the launch-per-piece path and to the oracle.  src == nullptr: u = 0 (a fresh
// coarse guess, cpu.lua:138, without the memset).  src and dst are different buffers.

// 3D: 16 waves (the levels are small, so a workgroup is most of a CU); 2D tiles are 32 x 32
template <int DIM>
constexpr int blk_threads() { return DIM == 3 ? 1024 : 256; }

// Compile-time shape of a phase: owned B^DIM tile, halo E (y, z) and HX (x, even), NS sweeps.  FW (PRE):
// the full-weighting restriction reads the residuals of a one-cell ring around the tile, so the swept
// region ends one cell wider.
template <int DIM, bool PRE, int B, int NS, bool FW = false>
struct BlkShape {
    static constexpr int E = PRE ? 2 * NS + 1 + (FW ? 1 : 0) : 2 * NS;
    static constexpr int HX = (E + 1) & ~1;
    static constexpr int EX = B + 2 * HX, EY = B + 2 * E, EZ = DIM == 3 ? B + 2 * E : 1, EH = EX / 2;
    static constexpr int BZ = DIM == 3 ? B : 1;  // owned planes
    static constexpr int cells = EX * EY * EZ;
    static constexpr int owned = B * B * BZ;
    static constexpr int RB = FW ? B + 2 : B, RBZ = DIM == 3 ? RB : 1;  // residual region edge (PRE)
    static constexpr int rcells = RB * RB * RBZ;
    // POST: coarse cells x0/2 - 1 .. of the extended tile's parents and their neighbours
    static constexpr int CX = EX / 2 + 2, CY = EY / 2 + 3, CZ = DIM == 3 ? EZ / 2 + 3 : 1;
    static constexpr int ccells = CX * CY * CZ;
    static constexpr int lidx(int lz, int ly, int c, int mm) { return ((lz * EY + ly) * 2 + c) * EH + mm; }
};

// PRE: LINEAR selects the restriction (0: the 2^DIM average, 1: full weighting with face weight 3 - clc)
template <typename T, int DIM, bool PRE, int LINEAR, int B, int NS>
__global__ __launch_bounds__(blk_threads<DIM>()) void k_blk(const T* __restrict__ src, const T* __restrict__ f,
                                                            T* __restrict__ dst, T* __restrict__ R,
                                                            const T* __restrict__ V, Geo g, Geo gc, Op<T, DIM> op,
                                                            T clc)
{
    constexpr bool FW = PRE && LINEAR == 1;
    using S = BlkShape<DIM, PRE, B, NS, FW>;
    constexpr int E = S::E, HX = S::HX, EY = S::EY, EZ = S::EZ, EH = S::EH, BZ = S::BZ;
    constexpr int EZH = DIM == 3 ? E : 0;  // z halo
    constexpr int NT = blk_threads<DIM>();
    extern __shared__ __align__(16) unsigned char blk_smem[];
    T* const U = reinterpret_cast<T*>(blk_smem);
    T* const F = U + S::cells;
    T* const RS = F + S::cells;  // PRE: residuals of the owned cells (x fastest)
    T* const VC = F + S::cells;  // POST: the staged coarse region
    const int tid = threadIdx.x;
    __shared__ Op<T, DIM> sop;  // the operator in LDS: its diagonal table is indexed per cell
    if (tid == 0) sop = op;
    const int ntx = g.nx / B, nty = g.ny / B;
    const int b = blockIdx.x;
    const int X0 = (b % ntx) * B, Y0 = ((b / ntx) % nty) * B, Z0 = (b / (ntx * nty)) * BZ;
    const int xs = X0 - HX, ys = Y0 - E, zs = Z0 - EZH;  // global (local-plane) origin of the LDS box
    const int mxs = xs >> 1;                            // xs is even
    const int nzl = (int)g.nz, gnz = (int)g.gnz, gz0 = (int)g.z0;
    const int p0 = (ys + zs + gz0) & 1;                 // parity of LDS row (0, 0)
    auto faces = [&](int gi, int gj, int gk) {          // box faces of a cell (gk global)
        return (gi == 0) + (gi == g.nx - 1) + (gj == 0) + (gj == g.ny - 1) + (DIM == 3 ? (gk == 0) + (gk == gnz - 1) : 0);
    };

    // load: every LDS slot of both colours (u: black cells in the box, 0 elsewhere; f: cells in the
    // box), all of a thread's global loads in flight at once.  POST: the coarse region the tile's
    // prolongation reads is staged in LDS (VC, unpacked) with the same loads, and P V of the black
    // slots is evaluated from there (prolong_eval: prolong_value's arithmetic) after one barrier.
    {
        constexpr int n = EZ * EY * 2 * EH;
        constexpr int NB = (n + NT - 1) / NT;
        constexpr int CX = S::CX, CY = S::CY, NCB = (S::ccells + NT - 1) / NT;
        const int cx0 = (xs >> 1) - 1, cy0 = (ys >> 1) - 1, cz0 = DIM == 3 ? (zs >> 1) - 1 : 0;
        T uv[NB], fv[NB], cv[PRE ? 1 : NCB];
        if (!PRE) {
#pragma unroll
            for (int q = 0; q < NCB; ++q) {
                const int t = tid + q * NT;
                const int a = t % CX, bb = (t / CX) % CY, cc = t / (CX * CY);
                const int I = cx0 + a, J = cy0 + bb, K = cz0 + cc;
                const bool in = t < S::ccells && I >= 0 && I < gc.nx && J >= 0 && J < gc.ny && K >= 0 &&
                                (DIM == 2 || K < (int)gc.nz);
                cv[q] = in ? V[pidx(gc, I, J, (int64_t)K)] : (T)0;
            }
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int it = tid + q * NT;
            const int row = it / (2 * EH), rest = it % (2 * EH);
            const int lz = row / EY, ly = row % EY;
            const int c = rest >= EH, mm = rest - c * EH;
            const int gm = mxs + mm, gj = ys + ly, gk = zs + lz;
            const bool in = it < n && gm >= 0 && gm < g.hw && gj >= 0 && gj < g.ny && gk >= 0 && gk < nzl;
            const int64_t gi = (int64_t)gk * g.P + c * g.H + (int64_t)gj * g.hw + gm;
            fv[q] = in ? f[gi] : (T)0;
            uv[q] = in && c == 1 && src ? src[gi] : (T)0;
        }
        if (!PRE) {
#pragma unroll
            for (int q = 0; q < NCB; ++q) {
                const int t = tid + q * NT;
                if (t < S::ccells) VC[t] = cv[q];
            }
            __syncthreads();
            auto get = [&](int I, int J, int64_t K) { return VC[(((int)K - cz0) * CY + (J - cy0)) * CX + (I - cx0)]; };
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int it = tid + q * NT;
                const int row = it / (2 * EH), rest = it % (2 * EH);
                const int lz = row / EY, ly = row % EY;
                const int c = rest >= EH, mm = rest - c * EH;
                const int gm = mxs + mm, gj = ys + ly, gk = zs + lz;
                const bool in = it < n && gm >= 0 && gm < g.hw && gj >= 0 && gj < g.ny && gk >= 0 && gk < nzl;
                if (in && c == 1) {
                    const int i = 2 * gm + (1 ^ ((ly + lz + p0) & 1));
                    uv[q] = uv[q] + prolong_eval<T, DIM, LINEAR>(get, gc, clc, i, gj, (int64_t)gk);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int it = tid + q * NT;
            if (it < n) {
                U[it] = uv[q];
                F[it] = fv[q];
            }
        }
    }
    __syncthreads();

    // in-plane and z neighbour sum of LDS cell (lx, ly, lz) of colour c: half_item's order
    auto nbsum = [&](int lx, int ly, int lz, int c) {
        const int mm = lx >> 1, o = lx & 1;
        const int oth = S::lidx(lz, ly, c ^ 1, mm);
        T sum = U[oth - 1 + o] + U[oth + o];
        sum = sum + U[oth - 2 * EH];
        sum = sum + U[oth + 2 * EH];
        if (DIM == 3) {
            sum = sum + U[oth - 2 * EH * EY];
            sum = sum + U[oth + 2 * EH * EY];
        }
        return sum;
    };

    // half-sweeps: colour s & 1 (red first) on the tile extended by e = E - 1 - s cells (cells
    // outside the box are skipped: they stay 0)
#pragma unroll
    for (int s = 0; s < 2 * NS; ++s) {
        const int c = s & 1, e = E - 1 - s;
        const int xlo = HX - e, xhi = HX + B - 1 + e;
        const int mlo = xlo >> 1, nm = (xhi >> 1) - mlo + 1;
        const int ny = B + 2 * e, nz = DIM == 3 ? B + 2 * e : 1, n = nz * ny * nm;
        const int lz0 = DIM == 3 ? E - e : 0;
#pragma unroll
        for (int q = 0; q < (n + NT - 1) / NT; ++q) {
            const int it = tid + q * NT;
            const int row = it / nm, mm = mlo + it % nm;
            const int ly = E - e + row % ny, lz = lz0 + row / ny;
            const int o = c ^ ((ly + lz + p0) & 1);
            const int lx = 2 * mm + o;
            const int gi = xs + lx, gj = ys + ly, gkl = zs + lz;
            if (it < n && lx >= xlo && lx <= xhi && gi >= 0 && gi < g.nx && gj >= 0 && gj < g.ny && gkl >= 0 &&
                gkl < nzl) {
                const T sum = nbsum(lx, ly, lz, c);
                const int own = S::lidx(lz, ly, c, mm);
                U[own] = sop.relax_idx(sum, F[own], faces(gi, gj, gz0 + gkl));
            }
        }
        __syncthreads();
    }

    if (FW) {
        // residual of the owned cells and a one-cell ring (0 outside the box) into RS ...
        constexpr int RB = S::RB;
#pragma unroll
        for (int q = 0; q < (S::rcells + NT - 1) / NT; ++q) {
            const int it = tid + q * NT;
            if (it < S::rcells) {
                const int x = it % RB - 1, y = (it / RB) % RB - 1, z = DIM == 3 ? it / (RB * RB) - 1 : 0;
                const int gi = X0 + x, gj = Y0 + y, gk = Z0 + z;  // gk local
                T v = (T)0;
                if (gi >= 0 && gi < g.nx && gj >= 0 && gj < g.ny && (DIM == 2 || (gk >= 0 && gk < nzl))) {
                    const int lx = HX + x, ly = E + y, lz = EZH + z;
                    const int c = (lx & 1) ^ ((ly + lz + p0) & 1);
                    const int own = S::lidx(lz, ly, c, lx >> 1);
                    v = sop.residual_idx(nbsum(lx, ly, lz, c), F[own], U[own], faces(gi, gj, gz0 + gk));
                }
                RS[it] = v;
            }
        }
        __syncthreads();
        // ... then one coarse cell per thread by full weighting (fw_eval's order)
        constexpr int C = B / 2, CZ = DIM == 3 ? C : 1;
        const T wf = (T)3 - clc;
        for (int it = tid; it < C * C * CZ; it += NT) {
            const int I = it % C, J = (it / C) % C, K = it / (C * C);
            const int gI = (X0 >> 1) + I, gJ = (Y0 >> 1) + J, gK = (Z0 >> 1) + K;
            // RS holds fine local cell x at x + 1: coarse I reads RS columns 2I .. 2I + 3
            auto get = [&](int i, int j, int64_t k) {
                return RS[((DIM == 3 ? (int)k - Z0 + 1 : 0) * RB + (j - Y0 + 1)) * RB + (i - X0 + 1)];
            };
            R[pidx(gc, gI, gJ, (int64_t)gK)] = fw_eval<T, DIM>(get, g, gc, wf, gI, gJ, (int64_t)gK);
        }
    } else if (PRE) {
        // residual of every owned cell into RS (residual_at's expressions) ...
#pragma unroll
        for (int q = 0; q < (S::owned + NT - 1) / NT; ++q) {
            const int it = tid + q * NT;
            if (it < S::owned) {
                const int x = it % B, y = (it / B) % B, z = it / (B * B);
                const int lx = HX + x, ly = E + y, lz = EZH + z;
                const int c = (lx & 1) ^ ((ly + lz + p0) & 1);
                const int own = S::lidx(lz, ly, c, lx >> 1);
                const T sum = nbsum(lx, ly, lz, c);
                RS[it] = sop.residual_idx(sum, F[own], U[own], faces(X0 + x, Y0 + y, gz0 + Z0 + z));
            }
        }
        __syncthreads();
        // ... then one coarse cell per thread, children summed in resrestrict_item's order
        constexpr int C = B / 2, CZ = DIM == 3 ? C : 1;
        for (int it = tid; it < C * C * CZ; it += NT) {
            const int I = it % C, J = (it / C) % C, K = it / (C * C);
            const int r0 = (2 * K * B + 2 * J) * B + 2 * I;
            T sm = RS[r0] + RS[r0 + 1];
            sm = sm + RS[r0 + B];
            sm = sm + RS[r0 + B + 1];
            if (DIM == 3) {
                sm = sm + RS[r0 + B * B];
                sm = sm + RS[r0 + B * B + 1];
                sm = sm + RS[r0 + B * B + B];
                sm = sm + RS[r0 + B * B + B + 1];
            }
            R[pidx(gc, (X0 >> 1) + I, (Y0 >> 1) + J, (int64_t)((Z0 >> 1) + K))] = (DIM == 3 ? (T)0.125 : (T)0.25) * sm;
        }
    }
    // the owned cells to dst: both colours after POST; only the black ones after PRE (its output is read
    // only by POST, which loads black cells and whose first red half-sweep replaces the red ones)
    {
        constexpr int NC = PRE ? 1 : 2;  // colours stored
        constexpr int H2 = B / 2, n = BZ * B * NC * H2;
#pragma unroll
        for (int q = 0; q < (n + NT - 1) / NT; ++q) {
            const int it = tid + q * NT;
            if (it < n) {
                const int mm = it % H2, c = PRE ? 1 : (it / H2) & 1, ly = (it / (NC * H2)) % B, lz = it / (NC * H2 * B);
                dst[(int64_t)(Z0 + lz) * g.P + c * g.H + (int64_t)(Y0 + ly) * g.hw + (X0 >> 1) + mm] =
                    U[S::lidx(lz + EZH, ly + E, c, (HX >> 1) + mm)];
            }
        }
    }
}

}  // namespace

// ---- 3D-tiled phases of small levels ----

template <int DIM>
constexpr int blk_tile() { return DIM == 3 ? kBlkTile : kBlkTile2D; }

template <typename T, int DIM, bool PRE, int NS, bool FW = false>
constexpr size_t blk_lds()
{
    using S = BlkShape<DIM, PRE, blk_tile<DIM>(), NS, FW>;
    return (2 * (size_t)S::cells + (PRE ? (size_t)S::rcells : (size_t)S::ccells)) * sizeof(T);
}

// the owned tile edge B divides every axis of the level (3D: B^3 tiles, 2D: B^2)
bool block_supported(int rb, int dim, int ns, const Geo& g)
{
    if ((dim != 2 && dim != 3) || ns < 1 || ns > kBlkMaxSweeps) return false;
    const int B = dim == 3 ? kBlkTile : kBlkTile2D;
    if (g.nx < B || g.ny < B || (dim == 3 && g.nz < B) || g.z0 != 0 || g.gnz != g.nz) return false;
    const size_t lds = rb == 8 ? (dim == 3 ? blk_lds<double, 3, true, kBlkMaxSweeps, true>() : blk_lds<double, 2, true, kBlkMaxSweeps, true>())
                               : (dim == 3 ? blk_lds<float, 3, true, kBlkMaxSweeps, true>() : blk_lds<float, 2, true, kBlkMaxSweeps, true>());
    return lds <= kTailMaxLds;
}

template <typename T, int D, int NS>
static hipError_t blk_attr_ns()
{
    constexpr int B = blk_tile<D>();
    const auto A = hipFuncAttributeMaxDynamicSharedMemorySize;
    const int pre = (int)blk_lds<T, D, true, NS>(), post = (int)blk_lds<T, D, false, NS>();
    const int pre_fw = (int)blk_lds<T, D, true, NS, true>();
    hipError_t e = hipFuncSetAttribute((const void*)k_blk<T, D, true, 0, B, NS>, A, pre);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_blk<T, D, true, 1, B, NS>, A, pre_fw);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_blk<T, D, false, 0, B, NS>, A, post);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_blk<T, D, false, 1, B, NS>, A, post);
    return e;
}

template <typename T>
static hipError_t blk_attr()
{
    hipError_t e = blk_attr_ns<T, 3, 1>();
    if (e == hipSuccess) e = blk_attr_ns<T, 3, 2>();
    if (e == hipSuccess) e = blk_attr_ns<T, 2, 1>();
    if (e == hipSuccess) e = blk_attr_ns<T, 2, 2>();
    return e;
}

template <typename T, int D, int NS>
static hipError_t blk_t(const BlockArgs& a, hipStream_t s)
{
    constexpr int B = blk_tile<D>();
    constexpr int NT = blk_threads<D>();
    const Op<T, D> op = make_op<T, D>(a.h, a.cl);
    const unsigned nb = (unsigned)((a.g.nx / B) * (a.g.ny / B) * (D == 3 ? a.g.nz / B : 1));
    const T* src = (const T*)a.src;
    if (a.pre && a.linear)  // PRE: linear = full-weighting restriction
        k_blk<T, D, true, 1, B, NS><<<nb, NT, blk_lds<T, D, true, NS, true>(), s>>>(
            src, (const T*)a.f, (T*)a.dst, (T*)a.R, (const T*)a.V, a.g, a.gc, op, (T)a.clc);
    else if (a.pre)
        k_blk<T, D, true, 0, B, NS><<<nb, NT, blk_lds<T, D, true, NS>(), s>>>(
            src, (const T*)a.f, (T*)a.dst, (T*)a.R, (const T*)a.V, a.g, a.gc, op, (T)a.clc);
    else if (a.linear)
        k_blk<T, D, false, 1, B, NS><<<nb, NT, blk_lds<T, D, false, NS>(), s>>>(
            src, (const T*)a.f, (T*)a.dst, (T*)a.R, (const T*)a.V, a.g, a.gc, op, (T)a.clc);
    else
        k_blk<T, D, false, 0, B, NS><<<nb, NT, blk_lds<T, D, false, NS>(), s>>>(
            src, (const T*)a.f, (T*)a.dst, (T*)a.R, (const T*)a.V, a.g, a.gc, op, (T)a.clc);
    return hipGetLastError();
}

hipError_t launch_block(int rb, int dim, const BlockArgs& a, hipStream_t s)
{
    if (!block_supported(rb, dim, a.ns, a.g)) return hipErrorInvalidValue;
    if (rb == 8) {
        if (dim == 3) return a.ns == 1 ? blk_t<double, 3, 1>(a, s) : blk_t<double, 3, 2>(a, s);
        return a.ns == 1 ? blk_t<double, 2, 1>(a, s) : blk_t<double, 2, 2>(a, s);
    }
    if (dim == 3) return a.ns == 1 ? blk_t<float, 3, 1>(a, s) : blk_t<float, 3, 2>(a, s);
    return a.ns == 1 ? blk_t<float, 2, 1>(a, s) : blk_t<float, 2, 2>(a, s);
}

hipError_t blk_attr(int rb) { return rb == 4 ? blk_attr<float>() : blk_attr<double>(); }

}  // namespace mgp
