// ntt_sizes.hpp -- the tile geometry of every ring size the NTT-family kernels are built for.  One row per log_n; the launch code
// (ntt_launch.inl), the merged tails (troyn_mrr_small.hip) and the routing between the translation units (launch.hpp) read it.
#pragma once
#include <type_traits>

#ifndef TROYN_SMALL_EB
#define TROYN_SMALL_EB 3      // small launches at N = 16384 (two-pass form): 512 threads x 8 coefficients (single fused op 82 -> 78 us; 4: 82, 2: 81)
#endif

namespace troyn {

// a workgroup works on 2^tb words with 2^eb coefficients per thread (2^(tb - eb) threads).  tb == log_n: the whole limb in one tile, one
// pass.  tb < log_n: two passes -- log_n - tb strided layers (columns of 2^(2 tb - log_n) consecutive words), then contiguous 2^tb chunks;
// 2^(log_n - tb) workgroups per limb and pass.  tb == 0: no such form at this size.
struct NttTile { int tb, eb; };

struct NttSize {
    int log_n;
    NttTile full;        // transform that fills the chip
    NttTile small;       // transform of a small launch (is_small_launch, launch.hpp), where it differs: always two passes
    NttTile tensor;      // tensor_core_kernel (stage 1; stages 0 / 2 are the strided passes of this tile) and tensor_accumulate_kernel
    int ks_mac_eb;       // first-generation ks_mac_kernel (0: not built -- N >= 8192 takes ksmac2_kernel / ksmaci_kernel)
    bool tensor_acc;     // tensor_accumulate_kernel is built
    bool merged_tail;    // mrr_quartet_kernel / mrr_quartet_load_kernel are built: single passes of the two-pass form can be launched alone
    NttTile fft;         // FP64 complex FFT of the CKKS encoder (ckks_kernels.hpp): a point is 16 bytes, so a whole transform fits one workgroup's LDS up to N = 8192
};

// N = 4096 / 8192: 8 coefficients per thread (EB = 3) doubles the waves per tile, so a CU holds 32 waves instead of 16; measured 5-14 %
// faster than EB = 4 despite the extra LDS exchange.  N = 16384 needs EB = 4 to fit one workgroup (1024 threads x 16 coefficients).
// N = 8192 / 16384, small launches: a whole-limb tile puts a transform on ONE CU (15-23 us at N = 16384 however few limbs the launch
// has); launches that leave most of the chip idle take the two-pass form of the larger rings -- 4 workgroups per limb and pass, ~3x shorter.
constexpr int NTT_LOG_N_MIN = 10, NTT_LOG_N_MAX = 17;
constexpr NttSize NTT_SIZES[] = {
    // log_n  full      small                  tensor    ks_mac  acc    merged tail  fft
    {10,      {10, 4},  {0, 0},                {10, 4},  4,      false, false,     {10, 3}},
    {11,      {11, 4},  {0, 0},                {11, 4},  4,      false, false,     {11, 3}},
    {12,      {12, 3},  {0, 0},                {12, 3},  4,      false, false,     {12, 3}},
    {13,      {13, 3},  {11, TROYN_SMALL_EB},  {13, 3},  0,      false, true,      {13, 3}},
    {14,      {14, 4},  {12, TROYN_SMALL_EB},  {14, 4},  0,      false, true,      {12, 3}},
    {15,      {12, 4},  {0, 0},                {12, 4},  0,      true,  true,      {12, 3}},
    {16,      {12, 4},  {0, 0},                {12, 4},  0,      true,  false,     {12, 3}},
    {17,      {12, 4},  {0, 0},                {0, 0},   0,      false, false,     {12, 3}},
};
constexpr const NttSize& ntt_size(int log_n) { return NTT_SIZES[log_n - NTT_LOG_N_MIN]; }
static_assert(ntt_size(NTT_LOG_N_MIN).log_n == NTT_LOG_N_MIN && ntt_size(13).log_n == 13 && ntt_size(NTT_LOG_N_MAX).log_n == NTT_LOG_N_MAX, "row i holds log_n = NTT_LOG_N_MIN + i");
// the two-pass form whose passes the merged tails launch one at a time: the small form, or the only form where every launch is two-pass
constexpr NttTile ntt_merged_tail_tile(int log_n) { return ntt_size(log_n).small.tb ? ntt_size(log_n).small : ntt_size(log_n).full; }

// the transforms of one arithmetic class are instantiated in two translation units so that they compile in parallel: part 1 holds
// N <= 8192, part 2 N >= 16384 (part 0: every size)
constexpr int ntt_part_of(unsigned log_n) { return log_n <= 13 ? 1 : 2; }
constexpr bool ntt_part_holds(int part, int log_n) { return part == 0 || part == ntt_part_of((unsigned)log_n); }


// The one switch from a runtime log_n to a compile-time one: f(std::integral_constant<int, log_n>{}) for the sizes of part PART (f is
// instantiated for these alone), false for every other log_n.  f returns whether it found a kernel.
template <int PART, int LOGN, class F>
inline bool at_ntt_size(F& f) {
    if constexpr (ntt_part_holds(PART, LOGN)) return f(std::integral_constant<int, LOGN>{});
    else return false;
}
template <int PART, class F>
inline bool for_ntt_size(unsigned log_n, F&& f) {
    static_assert(NTT_LOG_N_MIN == 10 && NTT_LOG_N_MAX == 17 && sizeof(NTT_SIZES) / sizeof(NTT_SIZES[0]) == 8, "one case per row of NTT_SIZES");
    switch (log_n) {
        case 10: return at_ntt_size<PART, 10>(f);
        case 11: return at_ntt_size<PART, 11>(f);
        case 12: return at_ntt_size<PART, 12>(f);
        case 13: return at_ntt_size<PART, 13>(f);
        case 14: return at_ntt_size<PART, 14>(f);
        case 15: return at_ntt_size<PART, 15>(f);
        case 16: return at_ntt_size<PART, 16>(f);
        case 17: return at_ntt_size<PART, 17>(f);
        default: return false;
    }
}

}  // namespace troyn
