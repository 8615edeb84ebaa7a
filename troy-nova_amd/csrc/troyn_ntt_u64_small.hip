// kernel instantiations of the ArithU64 policy, N <= 8192 (ntt_launch.inl)
#include "ntt_launch.inl"

namespace troyn {

template struct NttUnit<ArithU64, 1>;

void launch_ntt_generic(const NttArgs& a, unsigned log_n, bool inverse, size_t limb_polys, const LaunchCtx& lc) {
    hipLaunchKernelGGL(ntt_generic_kernel, dim3((unsigned)limb_polys), dim3(256), 0, lc.s, a, log_n, inverse ? 1 : 0);
}

}  // namespace troyn
