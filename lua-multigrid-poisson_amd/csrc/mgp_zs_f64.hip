// mgp_zs_f64.hip — k_zs's fp64 instantiations (mgp_zs.h): their dispatch and dynamic-LDS attributes, for launch_fused
// and prepare_kernels (mgp_zs.hip, which holds the fp32 ones).
#include "mgp_zs.h"

namespace mgp {

hipError_t zs_attr_f64()
{
    const hipError_t e = fused_attr<double, true>();
    return e == hipSuccess ? fused_attr<double, false>() : e;
}

hipError_t launch_fused_f64(const FusedArgs& a, hipStream_t s)
{
    return a.cl == 0.0 ? fused_dispatch<double, true>(a, s) : fused_dispatch<double, false>(a, s);
}

}  // namespace mgp
