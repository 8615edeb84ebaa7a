// bgv_chain_kernels.hpp -- the element-wise steps of the fused BGV multiply -> relinearize -> mod-switch chain
// (troyn_bgv_multiply_relinearize_mod_switch, an addition to the reference's surface).  The transforms, the digit decomposition and the
// key-switch inner product are the library's own launches; what is new sits between them.
//
// Derivation (the CKKS chain's, ntt_kernels.hpp, with both corrections of the mod-t kind).  Level L, data primes q_0 .. q_{L-1}, special
// prime qk, dropped prime ql = q_{L-1}; c = a (x) b the three-polynomial tensor product; for each of the two output components:
//   P        the key-switch inner product of c_2 = a1 . b1 (NTT form, rows 0 .. L-1 and the special row)
//   s        INTT of P's special row, canonical mod qk
//   dk_j(s)  = [-s qk^-1 mod t]_{q_j} qk + [s]_{q_j}          the key switch's correction (bgv_delta_kernel on the special row)
//   Q_j      = P_j qk^-1 + c_j                                 so that relinearize gives R_j = Q_j - NTT_j(dk_j(s)) qk^-1
//   l        = INTT(Q_{L-1}) - dk_{L-1}(s) qk^-1 mod q_{L-1}   = INTT(R_{L-1}) by linearity of the transform, canonical
//   dl_j(l)  = [-l ql^-1 mod t]_{q_j} ql + [l]_{q_j}          the modulus switch's correction (bgv_delta_kernel on the dropped limb)
//   out_j    = (R_j - NTT_j(dl_j(l))) ql^-1 = (Q_j - NTT_j(dk_j(s) qk^-1 + dl_j(l))) ql^-1 mod q_j,   j < L-1
// so ONE forward transform per output limb carries both corrections, added in coefficient form.  Everything is exact integer arithmetic
// modulo q_j and every stored word is canonical, hence the words equal those of troyn_dyadic_convolute + troyn_bgv_relinearize +
// troyn_bgv_mod_t_and_divide_q_last_ntt.
//
// All four kernels are streaming kernels of poly_kernels.hpp's geometry: 256 threads, a thread owns two adjacent coefficients, 16-byte
// loads and stores, wave-uniform modulus constants, no LDS, no scratch.
#pragma once
#include "poly_kernels.hpp"

namespace troyn {

// c_2 = a1 . b1, the key switch's target: a, b [batch][2][L][N] -> c2 [batch][L][N] (the word dyadic_convolute_kernel<2, 2> stores)
__global__ __launch_bounds__(POLY_BLOCK) void bgv_chain_c2_kernel(unsigned chunks, const DevModulus* __restrict__ mods, unsigned L, unsigned n,
                                                                  const u64* __restrict__ a, const u64* __restrict__ b, u64* __restrict__ c2) {
    const unsigned j = blk_row(chunks) % L;
    const size_t item = blk_row(chunks) / L;
    const DevModulus md = mods[j];
    const size_t in_off = (item * 2 + 1) * (size_t)L * n + (size_t)j * n;
    u64* op = c2 + (item * L + j) * (size_t)n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 va = ld2(a + in_off + i), vb = ld2(b + in_off + i);
        st2(op + i, mul_mod(va.a, vb.a, md), mul_mod(va.b, vb.b, md));
    }
}

// the 128-bit sum P w + c_comp of one coefficient, reduced ONCE: P, w < 2^64 and 2^61, a, b canonical below 2^61, so at most three
// products below 2^125 meet one word below 2^61
__device__ __forceinline__ u64 bgv_chain_q_word(u64 P, u64 w, u64 a0, u64 a1, u64 b0, u64 b1, bool comp1, u64 extra, const DevModulus& md) {
    u64 lo, hi;
    mul128(P, w, lo, hi);
    if (comp1) { mac128(lo, hi, a0, b1); mac128(lo, hi, a1, b0); }
    else mac128(lo, hi, a0, b0);
    const u128 acc = (((u128)hi << 64) | lo) + extra;
    return barrett128((u64)acc, (u64)(acc >> 64), md.q, md.ratio_lo, md.ratio_hi);
}

// Last-limb row: Q_{L-1} = P_{L-1} qk^-1 + c_{L-1} of both components, the input of the INTT that yields l.
//   prod [batch][2][L+1][N] (the inner product), a, b [batch][2][L][N], inv_k [j] = qk^-1 mod q_j (operand, quotient), q_last [batch][2][N]
__global__ __launch_bounds__(POLY_BLOCK) void bgv_chain_last_row_kernel(unsigned chunks, const DevModulus* __restrict__ mods, unsigned L, unsigned n,
                                                                        const u64* __restrict__ prod, const u64* __restrict__ a, const u64* __restrict__ b,
                                                                        const ulonglong2* __restrict__ inv_k, u64* __restrict__ q_last) {
    const size_t r = blk_row(chunks);                  // item * 2 + component
    const size_t item = r >> 1;
    const bool comp1 = (r & 1) != 0;
    const DevModulus md = mods[L - 1];
    const u64 w = inv_k[L - 1].x;
    const size_t pc = (size_t)L * n;
    const u64* ap = a + item * 2 * pc + (size_t)(L - 1) * n;
    const u64* bp = b + item * 2 * pc + (size_t)(L - 1) * n;
    const u64* pp = prod + (r * (L + 1) + (L - 1)) * (size_t)n;
    u64* op = q_last + r * n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 P = ld2(pp + i), a0 = ld2(ap + i), b0 = ld2(bp + i);
        u64x2 a1{0, 0}, b1{0, 0};
        if (comp1) { a1 = ld2(ap + pc + i); b1 = ld2(bp + pc + i); }      // wave-uniform
        st2(op + i, bgv_chain_q_word(P.a, w, a0.a, a1.a, b0.a, b1.a, comp1, 0, md), bgv_chain_q_word(P.b, w, a0.b, a1.b, b0.b, b1.b, comp1, 0, md));
    }
}

// -(c mod t) * inv mod t: the multiplier of bgv_delta_kernel (inv == 1: t = 2 and the like, no multiply)
__device__ __forceinline__ u64 bgv_mod_t_multiplier(u64 c, const DevModulus& t, u64 inv) {
    u64 k = neg_mod(barrett64(c, t.q, t.ratio_hi), t.q);
    if (inv != 1) k = mul_mod(k, inv, t);
    return k;
}
// [k]_{q} big + [c]_{q}: the correction of one limb from its multiplier
__device__ __forceinline__ u64 bgv_delta_word(u64 k, u64 c, u64 big, const DevModulus& qj) {
    return add_mod(mul_mod(barrett64(k, qj.q, qj.ratio_hi), big, qj), barrett64(c, qj.q, qj.ratio_hi), qj.q);
}

// Combined delta: d_j = dk_j(s) qk^-1 + dl_j(l) mod q_j for the L-1 output limbs of one (item, component).  A thread reads its two words of
// s and of INTT(Q_{L-1}) once, forms l and the two mod-t multipliers once, then loops over the limbs (bgv_delta_kernel re-reads the row
// and recomputes the multiplier once per limb).
//   spec, q_last_intt [batch][2][N];  inv_k as above;  delta [batch][2][L-1][N]
struct BgvChainDeltaArgs {
    const DevModulus* mods; const ulonglong2* inv_k;
    DevModulus t;
    u64 inv_k_mod_t, inv_l_mod_t, qk, ql;
    unsigned L, n;
};

__global__ __launch_bounds__(POLY_BLOCK) void bgv_chain_delta_kernel(unsigned chunks, BgvChainDeltaArgs g, const u64* __restrict__ spec,
                                                                     const u64* __restrict__ q_last_intt, u64* __restrict__ delta) {
    const size_t r = blk_row(chunks);                  // item * 2 + component
    const unsigned L = g.L, n = g.n;
    const DevModulus ml = g.mods[L - 1];
    const ulonglong2 wl = g.inv_k[L - 1];
    u64* dp = delta + r * (L - 1) * (size_t)n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 s = ld2(spec + r * n + i), v = ld2(q_last_intt + r * n + i);
        const u64 k1a = bgv_mod_t_multiplier(s.a, g.t, g.inv_k_mod_t), k1b = bgv_mod_t_multiplier(s.b, g.t, g.inv_k_mod_t);
        const u64 la = sub_mod(v.a, shoup_mul(bgv_delta_word(k1a, s.a, g.qk, ml), wl.x, wl.y, ml.q), ml.q);
        const u64 lb = sub_mod(v.b, shoup_mul(bgv_delta_word(k1b, s.b, g.qk, ml), wl.x, wl.y, ml.q), ml.q);
        const u64 k2a = bgv_mod_t_multiplier(la, g.t, g.inv_l_mod_t), k2b = bgv_mod_t_multiplier(lb, g.t, g.inv_l_mod_t);
        for (unsigned j = 0; j + 1 < L; ++j) {
            const DevModulus qj = g.mods[j];
            const ulonglong2 w = g.inv_k[j];
            const u64 da = add_mod(shoup_mul(bgv_delta_word(k1a, s.a, g.qk, qj), w.x, w.y, qj.q), bgv_delta_word(k2a, la, g.ql, qj), qj.q);
            const u64 db = add_mod(shoup_mul(bgv_delta_word(k1b, s.b, g.qk, qj), w.x, w.y, qj.q), bgv_delta_word(k2b, lb, g.ql, qj), qj.q);
            st2(dp + (size_t)j * n + i, da, db);
        }
    }
}

// Finish: out_j = (P_j qk^-1 + c_j - D_j) ql^-1 mod q_j for both components of one (item, limb) row, D = NTT(delta).  c_0 = a0 . b0 and
// c_1 = a0 . b1 + a1 . b0 are formed while loading a and b; the sum P_j qk^-1 + c_j + (q_j - D_j) is kept in 128 bits and reduced once
// (bgv_chain_q_word), then takes the Shoup multiply by ql^-1.  Geometry of multiply_affine_kernel.
//   prod [batch][2][L+1][N], dntt and out [batch][2][L-1][N];  inv_l [j] = ql^-1 mod q_j
__global__ __launch_bounds__(POLY_BLOCK) void bgv_chain_finish_kernel(unsigned chunks, const DevModulus* __restrict__ mods, unsigned L, unsigned n,
                                                                      const u64* __restrict__ prod, const u64* __restrict__ a, const u64* __restrict__ b,
                                                                      const u64* __restrict__ dntt, const ulonglong2* __restrict__ inv_k,
                                                                      const ulonglong2* __restrict__ inv_l, u64* __restrict__ out) {
    const unsigned j = blk_row(chunks) % (L - 1);
    const size_t item = blk_row(chunks) / (L - 1);
    const DevModulus md = mods[j];
    const u64 wk = inv_k[j].x;
    const ulonglong2 wl = inv_l[j];
    const size_t pc = (size_t)L * n, ppc = (size_t)(L + 1) * n, opc = (size_t)(L - 1) * n;
    const u64* ap = a + item * 2 * pc + (size_t)j * n;
    const u64* bp = b + item * 2 * pc + (size_t)j * n;
    const u64* pp = prod + item * 2 * ppc + (size_t)j * n;
    const u64* dp = dntt + item * 2 * opc + (size_t)j * n;
    u64* op = out + item * 2 * opc + (size_t)j * n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 a0 = ld2(ap + i), a1 = ld2(ap + pc + i), b0 = ld2(bp + i), b1 = ld2(bp + pc + i);
        const u64x2 P0 = ld2(pp + i), P1 = ld2(pp + ppc + i), D0 = ld2(dp + i), D1 = ld2(dp + opc + i);
        u64 r0 = bgv_chain_q_word(P0.a, wk, a0.a, 0, b0.a, 0, false, md.q - D0.a, md);
        u64 r1 = bgv_chain_q_word(P0.b, wk, a0.b, 0, b0.b, 0, false, md.q - D0.b, md);
        st2(op + i, shoup_mul(r0, wl.x, wl.y, md.q), shoup_mul(r1, wl.x, wl.y, md.q));
        r0 = bgv_chain_q_word(P1.a, wk, a0.a, a1.a, b0.a, b1.a, true, md.q - D1.a, md);
        r1 = bgv_chain_q_word(P1.b, wk, a0.b, a1.b, b0.b, b1.b, true, md.q - D1.b, md);
        st2(op + opc + i, shoup_mul(r0, wl.x, wl.y, md.q), shoup_mul(r1, wl.x, wl.y, md.q));
    }
}

}  // namespace troyn
