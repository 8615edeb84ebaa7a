// troyn_ckks.hip -- the instantiations and launches of the CKKS encoder kernels (ckks_kernels.hpp); troyn.hip (the C-ABI) only calls these.
#include "ckks_kernels.hpp"
#include "launch.hpp"

namespace troyn {

bool ckks_fft_two_pass(unsigned log_n) {
    return log_n >= (unsigned)NTT_LOG_N_MIN && log_n <= (unsigned)NTT_LOG_N_MAX && ntt_size((int)log_n).fft.tb < (int)log_n;
}

template <int LOGN, bool DEC, int SRC = CKKS_SRC_VALUES>
static void ckks_fft_passes(const CkksFftArgs& a, size_t batch, hipStream_t s) {
    constexpr int TB = ntt_size(LOGN).fft.tb;
    static_assert(ntt_size(LOGN).fft.eb == 3, "ckks_fft_kernel holds 8 points per thread");
    const dim3 grid((unsigned)(batch << (LOGN - TB))), block(1u << (TB - 3));
    if constexpr (TB == LOGN) {
        hipLaunchKernelGGL((ckks_fft_kernel<LOGN, TB, DEC, false, SRC>), grid, block, 0, s, a);
    } else if constexpr (DEC) {          // gap N/2 downwards: the strided layers first
        hipLaunchKernelGGL((ckks_fft_kernel<LOGN, TB, true, true>), grid, block, 0, s, a);
        hipLaunchKernelGGL((ckks_fft_kernel<LOGN, TB, true, false>), grid, block, 0, s, a);
    } else {                             // gap 1 upwards: the contiguous tiles first
        hipLaunchKernelGGL((ckks_fft_kernel<LOGN, TB, false, false, SRC>), grid, block, 0, s, a);
        hipLaunchKernelGGL((ckks_fft_kernel<LOGN, TB, false, true>), grid, block, 0, s, a);
    }
}

bool launch_ckks_fft(unsigned log_n, bool decode, const CkksFftArgs& a, size_t batch, hipStream_t s) {
    return for_ntt_size<0>(log_n, [&](auto size) {
        constexpr int LOGN = decltype(size)::value;
        if (decode) ckks_fft_passes<LOGN, true>(a, batch, s);
        else ckks_fft_passes<LOGN, false>(a, batch, s);
        return true;
    });
}

// the encoder with the load of its first pass reading pre-rotated matrix diagonals (a.table, a.pairs); the second pass at the two-pass sizes is
// the values source's
bool launch_ckks_fft_diagonals(unsigned log_n, bool matrix, const CkksFftArgs& a, size_t batch, hipStream_t s) {
    return for_ntt_size<0>(log_n, [&](auto size) {
        constexpr int LOGN = decltype(size)::value;
        if (matrix) ckks_fft_passes<LOGN, false, CKKS_SRC_MATRIX>(a, batch, s);
        else ckks_fft_passes<LOGN, false, CKKS_SRC_DIAGONALS>(a, batch, s);
        return true;
    });
}

void launch_ckks_encode_polynomial(const double* coeffs, unsigned count, double scale, unsigned n, const DevModulus* mods, unsigned L, u64* residues,
                                   unsigned* too_large, size_t batch, hipStream_t s) {
    hipLaunchKernelGGL(ckks_encode_polynomial_kernel, dim3((unsigned)(batch * (n / 256))), dim3(256), 0, s, coeffs, count, scale, n, mods, L, residues, too_large);
}

bool launch_ckks_compose(const CkksComposeArgs& a, size_t batch, hipStream_t s) {
    const dim3 grid((unsigned)(batch * (a.n / 256))), block(256);
    if (a.L <= 2) hipLaunchKernelGGL(ckks_compose_kernel<2>, grid, block, 0, s, a);
    else if (a.L <= 4) hipLaunchKernelGGL(ckks_compose_kernel<4>, grid, block, 0, s, a);
    else if (a.L <= 8) hipLaunchKernelGGL(ckks_compose_kernel<8>, grid, block, 0, s, a);
    else if (a.L <= (unsigned)CKKS_MAX_L) hipLaunchKernelGGL(ckks_compose_kernel<CKKS_MAX_L>, grid, block, 0, s, a);
    else return false;
    return true;
}

// one thread per (diagonal, slot): 256 slots per workgroup along x, the diagonal along y
void launch_ckks_dft_factor(const CkksDftFactorArgs& a, hipStream_t s) {
    const unsigned n = 1u << (a.log_n - 1);
    hipLaunchKernelGGL(ckks_dft_factor_kernel, dim3((n + 255) / 256, a.nd), dim3(256), 0, s, a);
}

// the sub-ring table: 256 rows of the n per workgroup along x, the diagonal along y
void launch_ckks_dft_factor_sparse(const CkksDftFactorSparseArgs& a, hipStream_t s) {
    const unsigned n = 1u << a.log_slots;
    hipLaunchKernelGGL(ckks_dft_factor_sparse_kernel, dim3((n + 255) / 256, a.nd), dim3(256), 0, s, a);
}

// the packed table: 256 rows of the 2n per workgroup along x, the diagonal along y
void launch_ckks_dft_factor_packed(const CkksDftFactorPackedArgs& a, hipStream_t s) {
    const unsigned rows = 1u << a.log_rows;
    hipLaunchKernelGGL(ckks_dft_factor_packed_kernel, dim3((rows + 255) / 256, a.nd), dim3(256), 0, s, a);
}

}  // namespace troyn
