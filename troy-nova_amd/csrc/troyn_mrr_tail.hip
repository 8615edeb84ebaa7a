// troyn_mrr_tail.hip -- the tail of the fused multiply -> relinearize -> rescale chain as ONE launch on whole-limb tiles, N = 16384 (round 7).
//
// After the inner product the chain ran three whole-limb launches (troyn.hip mrr_chain steps (3)-(5)): INTT of the special rows -> T_s,
// LAST_LIMB (INTT of Q_{L-1}, reads T_s) -> T_l, TAIL_RESCALE (one forward transform per output limb, reads T_s and T_l).  For one item and
// one polynomial all of them work on the same coefficient positions, and the last inverse round leaves a thread exactly the 16 words
// {t + R 1024} the first forward round starts from.  Here one 1024-thread workgroup per (item, polynomial) runs the two inverse transforms,
// keeps both results in 2 x 16 registers per thread and loops over the L - 1 output limbs: the rows T_s / T_l are neither written nor read
// (2 x 2 x 128 KB stored and (2 + 2 (L - 1)) x 128 KB loaded per item before), and three launch ramps and tails become one.
// What mrr_quartet_kernel (troyn_mrr_small.hip) does for the two-pass form of a small launch, for the batches that fill the chip.
// Arithmetic: ntt_pass_body itself (REGIO 3 / 4) -- ArithF64's butterflies in the order of the three separate kernels.  The two rows are handed
// over as centred representatives c(s) in [-(qk-1)/2, (qk-1)/2] and c(l) in [-(ql-1)/2, (ql-1)/2] (ArithF64::centred: the rows T = (x + aux/2) mod aux
// of the separate launches, minus aux/2), which every output limb uses as its rounding fix without a constant or a reduction of its own; every
// value is an exact integer in a double, congruent to the one the separate kernels hold, and the canonical outputs are the same words.
// Magnitudes: |c| < 2^49; held_tail_in gives |x| <= 0.6875 p + 2^49, a 4-layer forward block from there stays below 7.7 x 2^50 < 2^53 (ntt_kernels.hpp).
// Reference: evaluator_keyswitching_core.cu:570-658 (ski_util6/7), utils/rns_tool.cu:523-627 (divide_and_round_q_last_ntt).
#include "launch.hpp"

#ifndef TROYN_MRR_TAIL_PARK
#define TROYN_MRR_TAIL_PARK 3
#endif

namespace troyn {

// sp: the special rows (in = row K-1 of poly_prod, inverse tables, NTT_FLAG_STORE_ROUND_HALF); la: step (4)'s arguments; ta: step (5)'s.
// grid = batch * 2, workgroup g = (item g / 2, polynomial g % 2); none of the three uses the XCD co-location (xcd_groups = 0): no row is shared.
template <int LOGN, int EB>
__global__ __launch_bounds__(1 << (LOGN - EB), 1) void mrr_tail_kernel(NttArgs sp, NttArgs la, NttArgs ta) {
    using A = ArithF64;
    constexpr int E = 1 << EB, THREADS = 1 << (LOGN - EB), PARK = TROYN_MRR_TAIL_PARK;
    static_assert(PARK >= 0 && PARK <= E && (ntt_lds_words(LOGN) + PARK * THREADS) * 8 <= 160 * 1024, "tile + parked words: the 160 KB of a CU");
    __shared__ u64 lds[ntt_lds_words(LOGN)];
    __shared__ double park[PARK > 0 ? PARK * THREADS : 1];
    const unsigned g = blockIdx.x;
    double th[2 * E];      // c(s), c(l) at the words {t + R 2^(LOGN-EB)}
    ntt_pass_body<A, LOGN, 0, LOGN, LOGN, EB, true, true, true, false, 0, 3>(sp, nullptr, lds, g, threadIdx.x, th);
    __syncthreads();       // the next transform's first exchange overwrites words other waves read in this one's last round
    ntt_pass_body<A, LOGN, 0, LOGN, LOGN, EB, true, true, true, false, NTT_FUSED_LAST_LIMB, 3>(la, nullptr, lds, g, threadIdx.x, th);
    // the forward transform takes 66 registers on its own, 2 more than 128 - 64: the last PARK words of c(l) wait in the part of the CU's LDS the
    // tile leaves free (PARK x 8 KB, word i of thread t at park[i][t]: no bank conflicts) and are read back where held_tail_in consumes them
    if constexpr (PARK > 0) static_for<0, PARK>([&](auto ic) { constexpr int i = decltype(ic)::value; park[i * THREADS + threadIdx.x] = th[2 * E - PARK + i]; });
    for (unsigned j = 0; j < ta.ncomp; ++j) {
        unsigned t = threadIdx.x;
        asm volatile("" : "+v"(t));      // neither the LDS addresses nor the parked words depend on the limb: keep them from being hoisted out of the loop into registers
        __syncthreads();
        if constexpr (PARK > 0) static_for<0, PARK>([&](auto ic) { constexpr int i = decltype(ic)::value; th[2 * E - PARK + i] = park[i * THREADS + t]; });
        ntt_pass_body<A, LOGN, 0, LOGN, LOGN, EB, false, true, true, false, NTT_FUSED_TAIL_RESCALE, 4>(ta, nullptr, lds, g * ta.ncomp + j, t, th);
    }
}

void launch_mrr_tail(unsigned log_n, size_t batch, const NttArgs& sp, const NttArgs& la, const NttArgs& ta, hipStream_t s) {
    if (log_n != 14) return;
    hipLaunchKernelGGL((mrr_tail_kernel<14, 4>), dim3((unsigned)(batch * 2)), dim3(1024), 0, s, sp, la, ta);
}

}  // namespace troyn
