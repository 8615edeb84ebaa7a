// troyn_raise.hip -- the instantiations and the launch of the CKKS ModRaise kernel (raise_kernels.hpp); troyn.hip (the C-ABI) only calls this.
#include "raise_kernels.hpp"
#include "launch.hpp"

namespace troyn {

template <int LM>
static void mod_raise_launch(const ModRaiseArgs& a, unsigned chunks, const dim3& grid, hipStream_t s) {
    hipLaunchKernelGGL(ckks_mod_raise_kernel<LM>, grid, dim3(RAISE_BLOCK), 0, s, chunks, a.in, a.low, a.low_stride, a.out, a.out_stride, a.mods, a.garner, a.radix,
                       a.half_digits, a.q_mod, a.K, a.L, a.LO, a.n);
}

// items = batch * pcount rows of (item, polynomial); the caller has checked items * chunks against the grid limit
bool launch_ckks_mod_raise(const ModRaiseArgs& a, size_t items, unsigned chunks, hipStream_t s) {
    const dim3 grid((unsigned)(items * chunks));
    if (a.L == 1) mod_raise_launch<1>(a, chunks, grid, s);
    else if (a.L == 2) mod_raise_launch<2>(a, chunks, grid, s);
    else if (a.L <= 4) mod_raise_launch<4>(a, chunks, grid, s);
    else if (a.L <= 8) mod_raise_launch<8>(a, chunks, grid, s);
    else if (a.L <= (unsigned)CKKS_MAX_L) mod_raise_launch<CKKS_MAX_L>(a, chunks, grid, s);
    else return false;
    return true;
}

}  // namespace troyn
