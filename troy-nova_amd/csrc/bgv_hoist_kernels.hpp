// bgv_hoist_kernels.hpp -- the tail of the hoisted BGV entries (troyn_bgv_apply_galois_many / _sum / _weighted_sums / _sum_each and
// troyn_bgv_linear_transform_bsgs, additions to the reference's surface; include/troyn.h).  Everything before the division is shared with
// the BFV/CKKS entries (hoist_kernels.hpp); what differs is how X_c is divided by the special prime qk (ski_util5):
//   s        INTT of X_c's special row, canonical mod qk
//   k        = -(s mod t) qk^-1 mod t
//   dk_j(s)  = [k]_{q_j} qk + [s]_{q_j}  mod q_j
//   result_j = (X_j - NTT_j(dk_j(s))) qk^-1  mod q_j
// dk depends on the special row alone, and the unkeyed contributions are injected as (qk mod q_j) y on the data rows only, so
// ((X + qk y) - dk) qk^-1 = (X - dk) qk^-1 + y holds as it does for the rounded division of BFV/CKKS.
//
// Both kernels are streaming kernels of poly_kernels.hpp's geometry: 256 threads, a thread owns two adjacent coefficients, 16-byte loads
// and stores, wave-uniform modulus constants, no LDS, no scratch.  The rows of every slot and item go in one launch.  troyn_bgv_switch_key,
// troyn_bgv_relinearize and the fused chain keep bgv_delta_kernel / bgv_finish_kernel.
#pragma once
#include "bgv_chain_kernels.hpp"

namespace troyn {

// delta [r][L][N] = dk_j(s) for the L data limbs of one (item, component) row r.  A thread reads its two words of s once and forms the two
// mod-t multipliers once (bgv_delta_kernel re-reads the row and recomputes the multiplier once per limb).
//   spec [rows][N], the special rows in coefficient form;  qk the special prime
__global__ __launch_bounds__(POLY_BLOCK) void bgv_hoist_delta_kernel(unsigned chunks, const DevModulus* __restrict__ mods, unsigned L, unsigned n,
                                                                     DevModulus t, u64 inv_k_mod_t, u64 qk, const u64* __restrict__ spec,
                                                                     u64* __restrict__ delta) {
    const size_t r = blk_row(chunks);                  // item * 2 + component
    const u64* sp = spec + r * n;
    u64* dp = delta + r * L * (size_t)n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 s = ld2(sp + i);
        const u64 ka = bgv_mod_t_multiplier(s.a, t, inv_k_mod_t), kb = bgv_mod_t_multiplier(s.b, t, inv_k_mod_t);
        for (unsigned j = 0; j < L; ++j) {
            const DevModulus qj = mods[j];
            st2(dp + (size_t)j * n + i, bgv_delta_word(ka, s.a, qk, qj), bgv_delta_word(kb, s.b, qk, qj));
        }
    }
}

// dest_j (op)= (X_j - D_j) qk^-1 mod q_j for one (item, component, limb) row, D = NTT(delta).  ADD_FIRST (TROYN_ASSIGN_OVERWRITE_EXCEPT_FIRST):
// component 0 adds into the destination, which holds the permuted c0; component 1, and both under TROYN_ASSIGN_OVERWRITE, overwrite.
// X and D canonical, so is every stored word.
//   prod [items][2][L+1][N] (rows 0 .. L-1 used), dntt and dest [items][2][L][N];  inv_k [j] = qk^-1 mod q_j (operand, quotient)
template <bool ADD_FIRST>
__global__ __launch_bounds__(POLY_BLOCK) void bgv_hoist_finish_kernel(unsigned chunks, const DevModulus* __restrict__ mods, unsigned L, unsigned n,
                                                                      const u64* __restrict__ prod, const u64* __restrict__ dntt,
                                                                      const ulonglong2* __restrict__ inv_k, u64* __restrict__ dest) {
    const unsigned j = blk_row(chunks) % L;
    const size_t r = blk_row(chunks) / L;              // item * 2 + component
    const DevModulus md = mods[j];
    const ulonglong2 w = inv_k[j];
    const bool add = ADD_FIRST && (r & 1) == 0;        // wave-uniform
    const u64* pp = prod + (r * (L + 1) + j) * (size_t)n;
    const u64* dl = dntt + (r * L + j) * (size_t)n;
    u64* op = dest + (r * L + j) * (size_t)n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 X = ld2(pp + i), D = ld2(dl + i);
        u64 r0 = shoup_mul(sub_mod(X.a, D.a, md.q), w.x, w.y, md.q);
        u64 r1 = shoup_mul(sub_mod(X.b, D.b, md.q), w.x, w.y, md.q);
        if (add) { const u64x2 o = ld2(op + i); r0 = add_mod(o.a, r0, md.q); r1 = add_mod(o.b, r1, md.q); }
        st2(op + i, r0, r1);
    }
}

}  // namespace troyn
