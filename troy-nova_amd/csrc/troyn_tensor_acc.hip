// kernel instantiations of tensor_accumulate_kernel (ntt_launch.inl): the FP64 policy; the integer policy's spill and are not built
#include "ntt_launch.inl"

namespace troyn {

bool launch_tensor_accumulate(unsigned log_n, bool f64, const NttArgs& fa, const TensorAccPtrs& terms, unsigned count, const NttArgs& id, size_t batch, const LaunchCtx& lc) {
    return f64 && launch_tensor_accumulate_class<ArithF64>(log_n, fa, terms, count, id, batch, lc);
}

}  // namespace troyn
