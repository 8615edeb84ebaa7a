// kernel instantiations of the ArithF64 policy, N >= 16384 (ntt_launch.inl)
#include "ntt_launch.inl"

namespace troyn {

template struct NttUnit<ArithF64, 2>;

}  // namespace troyn
