// mgp_fmg_dev.h — the device helpers of the cubic prolongation P3 shared by mgp_fmg.hip (the ordinary context's
// passes and the batched vector form) and mgp_batch.hip (fmg_prolong_part: the batch's scalar form, in global memory
// and in LDS).  mgp_fmg.hip's header has the definition of P3.  Internal to each translation unit.
#pragma once
#include "mgp_device.h"

namespace mgp {
namespace {

template <typename T>
struct W3 {
    static constexpr T wp = (T)(105.0 / 128.0), wn = (T)(35.0 / 128.0), wq = (T)(-7.0 / 128.0), wr = (T)(-5.0 / 128.0);
};

// ((wp a + wn b) + wq c) + wr d
template <typename T>
__device__ __forceinline__ T cub(T a, T b, T c, T d)
{
    T s = W3<T>::wp * a + W3<T>::wn * b;
    s = s + W3<T>::wq * c;
    s = s + W3<T>::wr * d;
    return s;
}

// sample q in [-2, m + 1] of the extended line: the in-box sample it comes from, and how many times mc multiplies it
__device__ __forceinline__ int ext_src(int q, int m, int& nmul)
{
    nmul = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (q < 0) {
            q = -1 - q;
            ++nmul;
        } else if (q >= m) {
            q = 2 * m - 1 - q;
            ++nmul;
        }
    }
    return q;
}

template <typename T>
__device__ __forceinline__ T ext_scale(T v, int nmul, T mc)
{
    if (nmul >= 1) v = mc * v;
    if (nmul >= 2) v = mc * v;
    return v;
}

}  // namespace
}  // namespace mgp
