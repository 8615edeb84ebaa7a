// kernel instantiations of the ArithU64 policy, N >= 16384 (ntt_launch.inl)
#include "ntt_launch.inl"

namespace troyn {

template struct NttUnit<ArithU64, 2>;

}  // namespace troyn
