// troyn_mulpair_half.hip -- step (1) of the fused multiply -> relinearize -> rescale chain, digits = INTT(a1 (.) b1), on half-limb tiles:
// two 256-thread workgroups per CU (mulpair_half_kernels.hpp).  N = 16384, all-FP64 chains, the batches that fill the chip -- the class
// mrr_tail_kernel serves (troyn_mrr_tail.hip); everything else keeps ntt_pass_kernel's NTT_FUSED_MULPAIR form.
#include "launch.hpp"
#include "mulpair_half_kernels.hpp"

namespace troyn {

bool launch_mulpair_half(unsigned log_n, size_t batch, const MulpairHalfArgs& a, hipStream_t s) {
    if (log_n != 14 || batch * a.L == 0 || batch * a.L > 0x7fffffffull) return false;
    hipLaunchKernelGGL(mulpair_half_kernel<MPH_LOAD_WINDOW>, dim3((unsigned)(batch * a.L)), dim3(KSM_THREADS), 0, s, a);
    return true;
}

}  // namespace troyn
