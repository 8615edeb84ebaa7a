// ntt_launch.inl -- launch code of the NTT-family kernels (ntt_kernels.hpp), templated on the arithmetic policy and on the part of the
// sizes a translation unit holds.  Included by troyn_ntt_{f64,u64}_{small,large}.hip, which instantiate NttUnit (launch.hpp) for one policy
// and one part each, and by troyn_tensor_acc.hip, so that the five sets of kernels compile in parallel; troyn.hip calls the entry points
// of launch.hpp.  Every tile size comes from ntt_sizes.hpp.
#pragma once
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <hip/hip_runtime.h>
#include "ntt_kernels.hpp"
#include "launch.hpp"

namespace troyn {

// IOM: compile-time variant of the kernel (0 plain, 1 key-switch tail, 2 rescale, 3..5 fused chain).  Whole-limb N = 16384 tiles of the
// FP64 policy can run with half-word LDS tiles (two workgroups per CU, ntt_pass_body HALF); they pay off where the kernel fits 64
// registers: the plain forward transform (+18 %, 3.8 -> 4.5 TB/s), the fused tail + rescale (+2 % on the headline) and, measured in round 3
// through the three-call path, the key-switch tail and the rescale (relinearize N = 16384 +2 %, multiply + relinearize + rescale as three calls
// +4 %).  The inverse variants need 76-82 registers; the plain one fits since the per-lane twiddles of its first round are loaded in three
// steps (ntt_pass_body: an opaque zero derived from the previous layer's result enters the table index, so the loads cannot be hoisted;
// scratch 68 -> 12 bytes, NTT + dyadic + INTT +2 %) and is on by default (mask 0x0127); the fused chain's MULPAIR / LAST_LIMB variants still
// spill 64 / 108 bytes in their loaders and stay on full-word tiles.  TROYN_NTT_HALF=<mask> (bit (INV ? 8 : 0) + IOM) selects variants for A/B runs.
template <class A, int LOGN, int LO, int G, int TB, int EB, bool INV, bool FIRST, bool LAST, int IOM>
static void launch_variant(const NttArgs& a, dim3 grid, dim3 block, const LaunchCtx& lc) {
    if constexpr (std::is_same<A, ArithF64>::value && LOGN == 14 && TB == 14 && LO == 0) {
        // bit (INV ? 8 : 0) + IOM selects the variant (plan option TROYN_NTT_HALF, -1: the default below)
        // half-word tiles buy a second workgroup per CU at the price of three barriers per exchange: with no more workgroups than CUs there is
        // nobody to share the CU with and the full-word tile is the faster one (a single ciphertext: three calls 174 -> 154 us per op); an
        // explicit TROYN_NTT_HALF is obeyed at every size
        const int half = lc.half_mask >= 0 ? lc.half_mask : (grid.x > device_cu_count() ? 0x0167 : 0);     // (bit 6: NTT_FUSED_TAIL_RESCALE_W follows bit 5)
        constexpr int half_bit = IOM == NTT_IOM_CENTRALIZE ? 0 : (INV ? 8 : 0) + IOM;                     // (the centralising loader follows the plain forward kernel)
        if ((half >> half_bit) & 1) { hipLaunchKernelGGL((ntt_pass_kernel<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, IOM, true>), grid, block, 0, lc.s, a); return; }
    }
    hipLaunchKernelGGL((ntt_pass_kernel<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, IOM, false>), grid, block, 0, lc.s, a);
}

template <class A, int LOGN, int LO, int G, int TB, int EB, bool INV, bool FIRST, bool LAST>
static void launch_pass(const NttArgs& a, size_t limb_polys, const LaunchCtx& lc) {
    const unsigned tiles = 1u << (LOGN - TB);
    dim3 grid((unsigned)(limb_polys * tiles)), block(1u << (TB - EB));
    // the fused prologue / epilogue is a compile-time variant of the forward kernels (no runtime branches per word)
    const unsigned lm = FIRST ? a.load_mode : 0u, sm = LAST ? a.store_mode : 0u;
    if constexpr (LOGN >= 13 && LOGN <= 15) {
        // kernels of the fused multiply -> relinearize -> rescale chain (NttFused): whole-limb at N <= 16384, both passes at N = 32768; both
        // policies since round 5 (chains with moduli of 2^50 and more run the chain per modulus class); the _W variants are FP64 kernels
        if constexpr (INV) {
            if (a.fused_mode == NTT_FUSED_MULPAIR) { launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, NTT_FUSED_MULPAIR>(a, grid, block, lc); return; }
            if (a.fused_mode == NTT_FUSED_LAST_LIMB) { launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, NTT_FUSED_LAST_LIMB>(a, grid, block, lc); return; }
            if constexpr (std::is_same<A, ArithF64>::value)
                if (a.fused_mode == NTT_FUSED_LAST_LIMB_W) { launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, NTT_FUSED_LAST_LIMB_W>(a, grid, block, lc); return; }
        } else {
            if (a.fused_mode == NTT_FUSED_TAIL_RESCALE) { launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, NTT_FUSED_TAIL_RESCALE>(a, grid, block, lc); return; }
            if constexpr (std::is_same<A, ArithF64>::value)
                if (a.fused_mode == NTT_FUSED_TAIL_RESCALE_W) { launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, NTT_FUSED_TAIL_RESCALE_W>(a, grid, block, lc); return; }
        }
    }
    if constexpr (INV && LAST) {
        if (sm == NTT_STORE_KS_FINISH) {   // coefficient-form key-switch tail: the finish runs in the inverse transform's epilogue
            launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, 1>(a, grid, block, lc);
            return;
        }
    }
    if constexpr (!INV && FIRST) {
        if (lm == NTT_LOAD_CENTRALIZE) {     // plaintext -> NTT form in one launch (troyn_plain_centralize_ntt)
            launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, NTT_IOM_CENTRALIZE>(a, grid, block, lc);
            return;
        }
    }
    if constexpr (!INV) {
        if (lm == NTT_LOAD_KS_ROUND || sm == NTT_STORE_KS_FINISH) {
            launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, 1>(a, grid, block, lc);
            return;
        }
        if (lm == NTT_LOAD_RESCALE || sm == NTT_STORE_RESCALE) {
            launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, 2>(a, grid, block, lc);
            return;
        }
    }
    launch_variant<A, LOGN, LO, G, TB, EB, INV, FIRST, LAST, 0>(a, grid, block, lc);
}

// single pass: whole limb in one tile
template <class A, int LOGN, int EB>
static void launch_single(const NttArgs& a, size_t lp, bool inv, const LaunchCtx& lc) {
    if (inv) launch_pass<A, LOGN, 0, LOGN, LOGN, EB, true, true, true>(a, lp, lc);
    else launch_pass<A, LOGN, 0, LOGN, LOGN, EB, false, true, true>(a, lp, lc);
}

// two passes: G1 strided layers (columns of 2^(TB-G1) consecutive words), then contiguous 2^TB chunks.
// The pass between them lives in `scratch` ([limb-polynomial][N], contiguous) when one is given, else in `out`: a fused
// epilogue that READS the old destination (key-switch tail with AddInplace / OverwriteExceptFirst) must not find the first
// pass's intermediate words there.
template <class A, int LOGN, int TB, int EB>
static void launch_two_pass(const NttArgs& a, size_t lp, bool inv, const LaunchCtx& lc, u64* scratch) {
    constexpr int G1 = LOGN - TB;
    NttArgs first = a, second = a;
    if (scratch) {
        first.out = scratch;
        first.out_cstride = (long long)1 << LOGN;
        first.out_pstride = (long long)a.ncomp << LOGN;
        first.out_bstride = (long long)a.pcount * a.ncomp << LOGN;
    }
    second.in = first.out;
    second.in_bstride = first.out_bstride; second.in_pstride = first.out_pstride; second.in_cstride = first.out_cstride;
    second.reduce_input = 0;
    if (!inv) {
        launch_pass<A, LOGN, 0, G1, TB, EB, false, true, false>(first, lp, lc);
        launch_pass<A, LOGN, G1, TB, TB, EB, false, false, true>(second, lp, lc);
    } else {
        launch_pass<A, LOGN, G1, TB, TB, EB, true, true, false>(first, lp, lc);
        launch_pass<A, LOGN, 0, G1, TB, EB, true, false, true>(second, lp, lc);
    }
}

// the transform form of one tile: whole limb in one pass, or two passes
template <class A, int LOGN, int TB, int EB>
static void launch_form(const NttArgs& a, size_t lp, bool inv, const LaunchCtx& lc, u64* scratch) {
    if constexpr (TB == LOGN) launch_single<A, LOGN, EB>(a, lp, inv, lc);
    else launch_two_pass<A, LOGN, TB, EB>(a, lp, inv, lc, scratch);
}

template <class A, int PART>
bool NttUnit<A, PART>::transform(unsigned log_n, const NttArgs& a, size_t lp, bool inverse, const LaunchCtx& lc, u64* scratch) {
    return for_ntt_size<PART>(log_n, [&](auto n) {
        constexpr int LOGN = decltype(n)::value;
        constexpr NttSize S = ntt_size(LOGN);
        // TROYN_NTT_SMALL_TWO_PASS=0 keeps the form that fills the chip (A/B runs, tests).  Results are the same words.
        if constexpr (S.small.tb != 0)
            if (is_small_launch(lp) && !lc.small_two_pass_off) { launch_form<A, LOGN, S.small.tb, S.small.eb>(a, lp, inverse, lc, scratch); return true; }
        launch_form<A, LOGN, S.full.tb, S.full.eb>(a, lp, inverse, lc, scratch);
        return true;
    });
}

// the two passes of launch_two_pass<A, LOGN, T.tb, T.eb>, T = ntt_merged_tail_tile(LOGN), one at a time
template <class A, int PART>
bool NttUnit<A, PART>::small_pass(unsigned log_n, int which, const NttArgs& a, size_t lp, const LaunchCtx& lc) {
    return for_ntt_size<PART>(log_n, [&](auto n) {
        constexpr int LOGN = decltype(n)::value;
        if constexpr (ntt_size(LOGN).merged_tail) {
            constexpr NttTile T = ntt_merged_tail_tile(LOGN);
            if (which == 0) launch_pass<A, LOGN, LOGN - T.tb, T.tb, T.tb, T.eb, true, true, false>(a, lp, lc);
            else launch_pass<A, LOGN, LOGN - T.tb, T.tb, T.tb, T.eb, false, false, true>(a, lp, lc);
            return true;
        } else return false;
    });
}

template <class A, int PART>
bool NttUnit<A, PART>::ks_mac(unsigned log_n, const NttArgs& a, const KeyPtrs& kp, size_t blocks, const LaunchCtx& lc) {
    return for_ntt_size<PART>(log_n, [&](auto n) {
        constexpr int LOGN = decltype(n)::value, EB = ntt_size(LOGN).ks_mac_eb;
        if constexpr (EB != 0) {
            hipLaunchKernelGGL((ks_mac_kernel<A, LOGN, EB>), dim3((unsigned)blocks), dim3(1u << (LOGN - EB)), 0, lc.s, a, kp);
            return true;
        } else return false;
    });
}

template <class A, int LOGN, int TB, int EB>
static void tensor_stage_t(int stage, const NttArgs& a, const NttArgs& b, const NttArgs& d, size_t batch, const LaunchCtx& lc) {
    constexpr int G1 = LOGN - TB;
    if constexpr (G1 > 0) {
        if (stage == 0) { launch_pass<A, LOGN, 0, G1, TB, EB, false, true, false>(a, batch * a.pcount * a.ncomp, lc); return; }
        if (stage == 2) { launch_pass<A, LOGN, 0, G1, TB, EB, true, false, true>(a, batch * a.pcount * a.ncomp, lc); return; }
    }
    if (stage != 1) return;
    const dim3 grid((unsigned)((batch * a.ncomp) << G1)), block(1u << (TB - EB));
    if constexpr (G1 > 0) {
        // three polynomials are held in registers next to the transform in flight.  Default: 512-thread workgroups x 8 coefficients
        // (100-111 registers, no spills, two workgroups = 16 waves per CU).  TROYN_TENSOR_WGS=3 / 2: 256 threads x 16 coefficients with
        // three (168 registers, 11-28 spilled) / two (no spills) workgroups per CU -- measured 1.8 % / 3 % slower at N = 32768 L = 10.
        const int wgs = lc.tensor_wgs;
        if (wgs == 8) {   // 512-thread workgroups x 8 coefficients: 100-111 registers, no spills, two workgroups (16 waves) per CU
            hipLaunchKernelGGL((tensor_core_kernel<A, LOGN, TB, 3, 2>), grid, dim3(1u << (TB - 3)), 0, lc.s, a, b, d);
        } else if (wgs == 3) hipLaunchKernelGGL((tensor_core_kernel<A, LOGN, TB, EB, 3>), grid, block, 0, lc.s, a, b, d);
        else hipLaunchKernelGGL((tensor_core_kernel<A, LOGN, TB, EB, 2>), grid, block, 0, lc.s, a, b, d);
    } else hipLaunchKernelGGL((tensor_core_kernel<A, LOGN, TB, EB, 1>), grid, block, 0, lc.s, a, b, d);
}

template <class A, int PART>
bool NttUnit<A, PART>::tensor(unsigned log_n, int stage, const NttArgs& a, const NttArgs& b, const NttArgs& d, size_t batch, const LaunchCtx& lc) {
    return for_ntt_size<PART>(log_n, [&](auto n) {
        constexpr int LOGN = decltype(n)::value;
        constexpr NttTile T = ntt_size(LOGN).tensor;
        if constexpr (T.tb != 0) {
            tensor_stage_t<A, LOGN, T.tb, T.eb>(stage, a, b, d, batch, lc);
            return true;
        } else return false;
    });
}

// sum of tensor products at the two-pass sizes (tensor_accumulate_kernel), one tensor tile per workgroup: 256 threads x 16 coefficients.
// Six arrays of 16 words stay in registers next to the transform in flight: one wave per SIMD and its 512 registers (FP64 class: 256 + 75
// used, no scratch; two workgroups per CU would leave 256 and spill 101).
template <class A>
static bool launch_tensor_accumulate_class(unsigned log_n, const NttArgs& fa, const TensorAccPtrs& terms, unsigned count, const NttArgs& id, size_t batch, const LaunchCtx& lc) {
    if (count == 0 || count > (unsigned)TENSOR_ACC_MAX_TERMS) return false;
    return for_ntt_size<0>(log_n, [&](auto n) {
        constexpr int LOGN = decltype(n)::value;
        constexpr NttTile T = ntt_size(LOGN).tensor;
        if constexpr (ntt_size(LOGN).tensor_acc) {
            hipLaunchKernelGGL((tensor_accumulate_kernel<A, LOGN, T.tb, T.eb, 1>), dim3((unsigned)((batch * fa.ncomp) << (LOGN - T.tb))), dim3(1u << (T.tb - T.eb)), 0, lc.s, fa, terms, count, id);
            return true;
        } else return false;
    });
}

}  // namespace troyn
