// mgp_mean.hip — removing the mean of a level's field (mgp_remove_mean, mgp_group_remove_mean,
// mgp_refine_remove_mean): Neumann boxes determine psi up to a constant and need sum f = 0.
//   k_mean_sum  S = sum of the field's cells in fp64 in a fixed order: per thread (grid-stride), per wave (butterfly),
//               the 4 wave sums of a workgroup in order, then launch_sum_partials.  One read of the field.
//   k_mean_div  m = S / N (after the all-reduce of S on a distributed level)
//   k_mean_sub  every cell becomes RN_T((double)x - m).  One read and one write of the field.
// Both passes walk the level's own slots, 2 H per plane, under the plane stride g.P: the pad slots of a padded layout
// (MGP_PLANE_PAD), the ghost planes and the empty slots of nx = 1 rows are neither summed nor written (they stay 0).
// Where rows allow it (nx >= 2, 16-byte aligned planes) an item is one 16-byte vector of consecutive slots.
#include "mgp_device.h"

#include <algorithm>

namespace mgp {
namespace {

template <typename T>
struct MeanVec {
    static constexpr int N = VN<T>::n, LN = sizeof(T) == 4 ? 2 : 1;  // reals per item and its log2
};

// offset of vector item `it` (N consecutive own slots; 2 H / N items per plane)
template <typename T>
__device__ __forceinline__ int64_t mean_item(int64_t it, const Geo& g)
{
    const int lpv = g.lhw + g.ly + 1 - MeanVec<T>::LN;
    return (it >> lpv) * g.P + ((it & (((int64_t)1 << lpv) - 1)) << MeanVec<T>::LN);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_mean_sum(const T* __restrict__ in, Geo g, double* __restrict__ partials)
{
    constexpr int N = MeanVec<T>::N;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    double s = 0.0;
    if (VEC) {
        const int64_t items = (2 * g.H * g.nz) >> MeanVec<T>::LN;
        for (int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x; it < items; it += step) {
            const Vec<T, N> v = vload<T, N>(in + mean_item<T>(it, g));
#pragma unroll
            for (int e = 0; e < N; ++e) s += (double)v.v[e];
        }
    } else {
        const int64_t n = 2 * g.H * g.nz;
        for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n; c += step) {
            const int64_t x = level_slot(c, g.lhw + g.ly + 1, g.P);
            int i, j;
            int64_t k;
            if (slot_cell(x, g, i, j, k)) s += (double)in[x];
        }
    }
    s = wave_sum(s);
    __shared__ double ws[kBlock / 64];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = ws[0];
        for (int w = 1; w < kBlock / 64; ++w) a += ws[w];
        partials[blockIdx.x] = a;
    }
}

__global__ void k_mean_div(double* __restrict__ out, double cells) { out[1] = out[0] / cells; }

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_mean_sub(T* __restrict__ x, Geo g, const double* __restrict__ out)
{
    constexpr int N = MeanVec<T>::N;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    const double m = out[1];
    if (VEC) {
        const int64_t items = (2 * g.H * g.nz) >> MeanVec<T>::LN;
        for (int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x; it < items; it += step) {
            T* const p = x + mean_item<T>(it, g);
            Vec<T, N> v = vload<T, N>(p);
#pragma unroll
            for (int e = 0; e < N; ++e) v.v[e] = (T)((double)v.v[e] - m);
            vstore<T, N>(p, v);
        }
    } else {
        const int64_t n = 2 * g.H * g.nz;
        for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n; c += step) {
            const int64_t o = level_slot(c, g.lhw + g.ly + 1, g.P);
            int i, j;
            int64_t k;
            if (slot_cell(o, g, i, j, k)) x[o] = (T)((double)x[o] - m);
        }
    }
}

// every own slot holds a cell, and every item is a 16-byte aligned vector inside one plane's own slots
template <typename T>
bool mean_vec(const void* p, const Geo& g)
{
    constexpr int N = MeanVec<T>::N;
    return g.nx >= 2 && 2 * g.H >= N && g.P % N == 0 && (uintptr_t)p % 16 == 0;
}

template <typename T>
unsigned mean_blocks(const Geo& g, bool vec)
{
    const int64_t items = vec ? (2 * g.H * g.nz) / MeanVec<T>::N : 2 * g.H * g.nz;
    return (unsigned)std::min<int64_t>(kSumBlocks, std::max<int64_t>(1, (items + kBlock - 1) / kBlock));
}

template <typename T>
void mean_sum_t(const void* p, const Geo& g, double* partials, unsigned* nb, hipStream_t s)
{
    const bool vec = mean_vec<T>(p, g);
    *nb = mean_blocks<T>(g, vec);
    if (vec) k_mean_sum<T, true><<<*nb, kBlock, 0, s>>>((const T*)p, g, partials);
    else k_mean_sum<T, false><<<*nb, kBlock, 0, s>>>((const T*)p, g, partials);
}

template <typename T>
void mean_sub_t(void* p, const Geo& g, const double* out, hipStream_t s)
{
    const bool vec = mean_vec<T>(p, g);
    const unsigned nb = nblk_gs(vec ? (2 * g.H * g.nz) / MeanVec<T>::N : 2 * g.H * g.nz);
    if (vec) k_mean_sub<T, true><<<nb, kBlock, 0, s>>>((T*)p, g, out);
    else k_mean_sub<T, false><<<nb, kBlock, 0, s>>>((T*)p, g, out);
}

}  // namespace

hipError_t launch_mean_sum(int rb, const void* p, Geo g, double* partials, double* out, hipStream_t s)
{
    unsigned nb = 1;
    MGP_REAL(rb, (mean_sum_t<T>(p, g, partials, &nb, s)));
    (void)launch_sum_partials(partials, (int)nb, out, s);
    return hipGetLastError();
}

hipError_t launch_mean_sub(int rb, void* p, Geo g, double cells, double* out, hipStream_t s)
{
    k_mean_div<<<1, 1, 0, s>>>(out, cells);
    MGP_REAL(rb, (mean_sub_t<T>(p, g, out, s)));
    return hipGetLastError();
}

}  // namespace mgp
