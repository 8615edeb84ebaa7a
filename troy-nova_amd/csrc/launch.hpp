// launch.hpp -- entry points of the translation units that hold the kernel instantiations (one per kernel family / arithmetic
// policy, so that they compile in parallel).  troyn.hip (the C-ABI) only calls these.
#pragma once
#include <hip/hip_runtime.h>
#include "ntt_kernels.hpp"
#include "ntt_sizes.hpp"
#include "ksmac_kernels.hpp"
#include "behz2_kernels.hpp"

#ifndef TROYN_SMALL_LP_FACTOR
#define TROYN_SMALL_LP_FACTOR 2      // measured 8 | 2 | 1: eight ciphertexts at N = 16384, fused chain 100 | 75 | 75 us; 128: 473 | 469 | 481
#endif

namespace troyn {

// CUs of the current device (cached per host thread)
inline unsigned device_cu_count() {
    static thread_local int cached_dev = -1;
    static thread_local unsigned cached = 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev != cached_dev) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        cached = (unsigned)cus; cached_dev = dev;
    }
    return cached;
}
// a launch of at most CUs / TROYN_SMALL_LP_FACTOR limb-polynomials counts as small (two-pass transforms at N = 8192 / 16384, merged tails, no split by class)
inline bool is_small_launch(size_t limb_polys) { return limb_polys * TROYN_SMALL_LP_FACTOR <= device_cu_count(); }

// what a launch of the NTT family needs besides its arguments: the stream and the plan's A/B options that select kernel variants
// (read once when the plan is created, troyn.hip TroynOptions -- no environment access on the launch path)
struct LaunchCtx {
    hipStream_t s;
    int half_mask;             // TROYN_NTT_HALF: half-word LDS tile variants of the whole-limb N = 16384 FP64 transforms; -1 = default
    bool small_two_pass_off;   // TROYN_NTT_SMALL_TWO_PASS=0
    int tensor_wgs;            // TROYN_TENSOR_WGS (8 = default)
};

// The NTT-family launches of one arithmetic class and one part of the sizes (ntt_sizes.hpp: ntt_part_of): defined in ntt_launch.inl,
// instantiated once in each of troyn_ntt_{f64,u64}_{small,large}.hip.  All return false where no kernel exists for the size.
template <class A, int PART>
struct NttUnit {
    static bool transform(unsigned log_n, const NttArgs& a, size_t limb_polys, bool inverse, const LaunchCtx& lc, u64* scratch);
    static bool small_pass(unsigned log_n, int which, const NttArgs& a, size_t limb_polys, const LaunchCtx& lc);
    static bool ks_mac(unsigned log_n, const NttArgs& a, const KeyPtrs& kp, size_t blocks, const LaunchCtx& lc);
    static bool tensor(unsigned log_n, int stage, const NttArgs& a, const NttArgs& b, const NttArgs& d, size_t batch, const LaunchCtx& lc);
};
extern template struct NttUnit<ArithF64, 1>;
extern template struct NttUnit<ArithF64, 2>;
extern template struct NttUnit<ArithU64, 1>;
extern template struct NttUnit<ArithU64, 2>;
// f(the unit that holds log_n under the FP64 (f64) or the integer policy)
template <class F>
inline bool in_ntt_unit(unsigned log_n, bool f64, F&& f) {
    if (ntt_part_of(log_n) == 1) return f64 ? f(NttUnit<ArithF64, 1>{}) : f(NttUnit<ArithU64, 1>{});
    return f64 ? f(NttUnit<ArithF64, 2>{}) : f(NttUnit<ArithU64, 2>{});
}

// optimised transform (false: no kernel for this size -> launch_ntt_generic)
inline bool launch_transform(unsigned log_n, bool f64, const NttArgs& a, size_t limb_polys, bool inverse, const LaunchCtx& lc, u64* scratch) {
    return in_ntt_unit(log_n, f64, [&](auto u) { return decltype(u)::transform(log_n, a, limb_polys, inverse, lc, scratch); });
}
void launch_ntt_generic(const NttArgs& a, unsigned log_n, bool inverse, size_t limb_polys, const LaunchCtx& lc);
// single objects through the fused chain at N = 8192 .. 32768: one pass of the two-pass transform a small launch takes (troyn_mrr_small.hip
// runs the strided passes between them itself).  which = 0: first inverse pass (the layers inside the contiguous chunks), 1: last forward
// pass (the same layers + the fused epilogue a.fused_mode selects)
inline bool launch_small_pass(unsigned log_n, bool f64, int which, const NttArgs& a, size_t limb_polys, const LaunchCtx& lc) {
    return in_ntt_unit(log_n, f64, [&](auto u) { return decltype(u)::small_pass(log_n, which, a, limb_polys, lc); });
}
// ... and the strided passes of the chain's tail (special rows, dropped limb, output limbs) as one launch
void launch_mrr_quartet(unsigned log_n, size_t batch, const NttArgs& sp, const NttArgs& la, const NttArgs& ta, hipStream_t s, bool limb_parallel);
void launch_mrr_quartet_load(unsigned log_n, size_t groups, const NttArgs& iv, const NttArgs& fw, hipStream_t s, bool f64);
// the same tail on whole-limb tiles for the batches that fill the chip (troyn_mrr_tail.hip; log_n = 14, all-FP64 chains): one launch for steps (3)-(5)
void launch_mrr_tail(unsigned log_n, size_t batch, const NttArgs& sp, const NttArgs& la, const NttArgs& ta, hipStream_t s);
// step (1) of the same chain for the same class on half-limb tiles, two workgroups per CU (troyn_mulpair_half.hip; log_n = 14, all-FP64 chains);
// false: no kernel for this size
struct MulpairHalfArgs;
bool launch_mulpair_half(unsigned log_n, size_t batch, const MulpairHalfArgs& a, hipStream_t s);
// first-generation fused key-switch inner product (ks_mac_kernel)
inline bool launch_ks_mac(unsigned log_n, bool f64, const NttArgs& a, const KeyPtrs& kp, size_t blocks, const LaunchCtx& lc) {
    return in_ntt_unit(log_n, f64, [&](auto u) { return decltype(u)::ks_mac(log_n, a, kp, blocks, lc); });
}
// tensor product fused with the transforms (tensor_core_kernel); stage 0 / 2: the strided passes of the two-pass sizes
inline bool launch_tensor(unsigned log_n, bool f64, int stage, const NttArgs& a, const NttArgs& b, const NttArgs& d, size_t batch, const LaunchCtx& lc) {
    return in_ntt_unit(log_n, f64, [&](auto u) { return decltype(u)::tensor(log_n, stage, a, b, d, batch, lc); });
}
// sum of tensor products fused with the transforms (tensor_accumulate_kernel, troyn_tensor_acc.hip; log_n = 15 / 16, at most
// TENSOR_ACC_MAX_TERMS terms).  FP64 class only: false for the integer class (its instantiations spill and are not built) and where no
// kernel exists for the size
bool launch_tensor_accumulate(unsigned log_n, bool f64, const NttArgs& fa, const TensorAccPtrs& terms, unsigned count, const NttArgs& id, size_t batch, const LaunchCtx& lc);
// second-generation key-switch inner product (ksmac2_kernel, log_n = 13 / 14 / 15) and its key preparation
// digits_f64: the digit rows hold doubles (fused chain: NTT_FLAG_STORE_F64) instead of u64 words; wide_digits: some digit limb is 2^50 or
// wider (mixed chains, a.row_mask selects the rows of moduli < 2^50): digits are reduced with integer arithmetic while loading
void launch_ksmac2(unsigned log_n, size_t batch, unsigned rows, const KsMacArgs& a, hipStream_t s, bool digits_f64 = false, bool wide_digits = false);
void launch_ksmac2_split(unsigned log_n, size_t batch, const KsMacArgs& a, hipStream_t s, bool digits_f64, int epi);
// scale (optional): Shoup pairs of the factor the rows r < scale_rows of every key component are multiplied by (fused chain: qk^-1 mod q_r)
void launch_ksmac_prepare_keys(const KeyPtrs& kp, unsigned L, unsigned polys, unsigned n, double* out, unsigned blocks, hipStream_t s,
                               const ulonglong2* scale = nullptr, const DevModulus* mods = nullptr, unsigned scale_rows = 0,
                               double* diag_out = nullptr);   // diag_out: [j][2][N], block (key j, modulus j) in natural order
// integer inner product for the rows of moduli >= 2^50 (ksmaci_kernel, log_n = 13 / 14 / 15) and its key preparation; a.row_mask = those rows
struct KsMacIArgs;
void launch_ksmaci(unsigned log_n, size_t batch, const KsMacIArgs& a, hipStream_t s, int epi);
void launch_ksmaci_prepare_keys(const KeyPtrs& kp, unsigned L, unsigned K, unsigned n, unsigned long long row_mask, ulonglong2* out, unsigned blocks, hipStream_t s,
                                const ulonglong2* scale, const DevModulus* mods, unsigned scale_rows, ulonglong2* diag_out);
// second-generation BEHZ conversions (L = 1 .. 16)
// aux50: the auxiliary base holds primes below 2^50 (Behz2Dev::NB > L of them) instead of the reference's 61-bit primes
void launch_behz2_lift(unsigned L, bool smallq, unsigned grid, hipStream_t s, unsigned chunks, const Behz2Dev& c, const u64* src, u64* dst, bool aux50 = false);
bool launch_behz2_lift_pass1(unsigned L, size_t items, hipStream_t s, const Behz2Dev& c, const u64* src, u64* dst_q, u64* dst_bsk,
                             const double* tw_q, const double* tw_aux, const DevModulus* q_mods, const DevModulus* aux_mods);
bool launch_behz2_floor_pass2(unsigned L, size_t items, hipStream_t s, const Behz2Dev& c, const u64* in_q, const u64* in_bsk, u64* out,
                              const double* tw_q, const double* tw_aux, const DevModulus* q_mods, const DevModulus* aux_mods);
void launch_behz2_floor(unsigned L, bool smallq, unsigned grid, hipStream_t s, unsigned chunks, const Behz2Dev& c, const u64* in_q, const u64* in_bsk, u64* out, bool aux50 = false);

// CKKS encoder (troyn_ckks.hip, ckks_kernels.hpp): the FP64 canonical-embedding FFT with its fused first loads / last stores (every pass of the
// size's form, ntt_sizes.hpp column fft), the coefficient-wise encoding, and the CRT composition of a decoded plaintext (L <= CKKS_MAX_L)
struct CkksFftArgs;
struct CkksComposeArgs;
struct CkksDftFactorArgs;
struct CkksDftFactorSparseArgs;
struct CkksDftFactorPackedArgs;
bool ckks_fft_two_pass(unsigned log_n);
bool launch_ckks_fft(unsigned log_n, bool decode, const CkksFftArgs& a, size_t batch, hipStream_t s);
bool launch_ckks_fft_diagonals(unsigned log_n, bool matrix, const CkksFftArgs& a, size_t batch, hipStream_t s);
void launch_ckks_encode_polynomial(const double* coeffs, unsigned count, double scale, unsigned n, const DevModulus* mods, unsigned L, u64* residues,
                                   unsigned* too_large, size_t batch, hipStream_t s);
bool launch_ckks_compose(const CkksComposeArgs& a, size_t batch, hipStream_t s);
void launch_ckks_dft_factor(const CkksDftFactorArgs& a, hipStream_t s);
void launch_ckks_dft_factor_sparse(const CkksDftFactorSparseArgs& a, hipStream_t s);
void launch_ckks_dft_factor_packed(const CkksDftFactorPackedArgs& a, hipStream_t s);
// CKKS ModRaise (troyn_raise.hip, raise_kernels.hpp): the centred base extension of items = batch * pcount polynomials in coefficient form, `chunks`
// workgroups per polynomial (L <= CKKS_MAX_L; false above)
struct ModRaiseArgs;
bool launch_ckks_mod_raise(const ModRaiseArgs& a, size_t items, unsigned chunks, hipStream_t s);

}  // namespace troyn
