// kernel instantiations of the ArithF64 policy, N <= 8192 (ntt_launch.inl)
#include "ntt_launch.inl"

namespace troyn {

template struct NttUnit<ArithF64, 1>;

}  // namespace troyn
