// hoist_kernels.hpp -- hoisted rotations (an ADDITION to the reference's kernels: troyn_apply_galois_many / troyn_apply_galois_sum).
//
// A key switch decomposes its target ONCE into the transformed digits D[item][L+1][L][N] (row k = the L digits under key modulus m_k,
// the forward transform with TROYN_IDX_KS_SET_PRODUCTS and reduce_input).  The automorphism X -> X^g commutes with the decomposition,
// and in NTT form it is the index permutation of galois_kernel (crypto_kernels.hpp):
//     pi_g(i) = brev_logN(((g * brev_{logN+1}(i + N)) >> 1) mod N)
// so the digits of sigma_g(c1) under every key modulus are D read at pi_g(i): `terms` Galois keys share one decomposition.
//
// Block property of pi_g (g odd): i + 1 for even i adds N to the (logN+1)-bit reversal, g * N / 2 = N / 2 (mod N) flips the top bit of
// the raw index, which the final reversal turns into the lowest bit: pi_g(i + 1) = pi_g(i) ^ 1.  By the same argument every aligned
// block of 2^b consecutive outputs reads ONE aligned block of 2^b sources.  A thread owns two adjacent outputs: its two digit words are
// one aligned 16-byte pair (swapped when pi_g(i) is odd), and a wave's 128 outputs gather from exactly one 1 KiB block of the digit row
// -- every fetched line is used in full, no LDS staging.
//
// hoist_mac_kernel: poly_prod[slot][item][c][k][i] = SUM_{t in S(slot)} SUM_j D[item][k][j][pi_t(i)] * key_{t,j}[c][k][i]  mod m_k
//   many form: S(slot) = {slot};  sum form: one slot, S = every term.
//   The keys are the HBM stream (16 L K N bytes per term): 16-byte loads per lane, coalesced; a workgroup carries IB items of the batch
//   through the same key registers.  Integer arithmetic for every modulus: 64 x 64 -> 128 products in a 128-bit accumulator, L <= 63
//   products of residues below 2^61 per term, ONE Barrett-128 reduction per term and output word, then an addition modulo m_k -- the
//   accumulator never runs across terms.  Every output word is written once.
// hoist_c0_kernel: dest[slot][item][0][l] = SUM_{t in S(slot)} sigma_{g_t}(c0[item][l])  mod q_l, a gather in either form (coefficient
//   form: the source of output o is i = o * g^-1 mod N, negated when (i * g) & N -- the sign rule of galois_kernel).
//
// hoist_weighted_kernel (troyn_apply_galois_weighted_sums): the same rows, pairs and gather with a plaintext weight between the per-term
//   Barrett reduction and the addition across terms,
//     poly_prod[slot][item][c][k][i] = SUM_{t in T(slot)} w_{slot,t}[m_k][i] * ( SUM_j D[item][k][j][pi_t(i)] * key_{t,j}[c][k][i]          (g_t != 1)
//                                                                            + (q_special mod q_k) * u_{t,c}[item][k][pi_t(i)] )  mod m_k   (k < L)
//   u_{t,0} = the NTT-form limbs of c0, u_{t,1} = those of c1 for the identity terms and nothing otherwise: the unkeyed contributions enter
//   BEFORE the division by the special prime, scaled by q_special on the data rows and absent from the special row, so the tail's
//   (X - r) * q_special^-1 returns them unscaled and r is untouched (include/troyn.h states the argument).  The slot is a grid dimension;
//   a term whose weight pointer is null in this slot is skipped without touching its keys; the keys of an identity term are never read.
//   One 16-byte weight load per thread and term serves the IB items.
#pragma once
#include "poly_kernels.hpp"

namespace troyn {

struct HoistArgs {
    const DevModulus* mods;
    unsigned K, L, log_n, batch;
    unsigned groups;               // ceil(batch / IB) (hoist_mac_kernel)
    unsigned terms_per_slot;       // many: 1, sum: terms
    int is_ntt_form;
    const u64* ct;                 // [batch][2][L][N]
    const u64* digits_ntt;         // D [batch][L+1][L][N]
    int diag_from_ct;              // NTT form with the diagonal blocks of D not produced (skip_diag): digit k of row k < L is c1's limb k itself
    const u64* const* keys;        // device table [terms][L] -> u64[2][K][N]
    const u64* elements;           // device table [terms]
    const u64* inv_elements;       // device table [terms]: g^-1 mod 2N (coefficient form)
    u64* poly_prod;                // [slots][batch][2][L+1][N]
    u64* dest;                     // [slots][batch][2][L][N]
};

__device__ __forceinline__ unsigned hoist_ntt_source(unsigned i, unsigned g, unsigned log_n) {
    const unsigned n = 1u << log_n;
    const unsigned reversed = __brev(i + n) >> (31 - log_n);                   // (log_n + 1)-bit reversal
    const unsigned index_raw = (unsigned)(((u64)g * reversed) >> 1) & (n - 1);
    return __brev(index_raw) >> (32 - log_n);
}

template <int IB>
__global__ __launch_bounds__(POLY_BLOCK) void hoist_mac_kernel(unsigned chunks, HoistArgs a) {
    const unsigned L = a.L, K = a.K, n = 1u << a.log_n;
    const unsigned row = blk_row(chunks);
    const unsigned k = row % (L + 1);
    const unsigned grp = (row / (L + 1)) % a.groups;
    const unsigned slot = row / (L + 1) / a.groups;
    const unsigned key_index = (k == L) ? K - 1 : k;
    const DevModulus md = a.mods[key_index];
    const size_t key_poly = (size_t)K * n;
    // items past the batch's end recompute the last item and store nothing
    size_t item[IB];
    const u64* dp[IB];
#pragma unroll
    for (int b = 0; b < IB; ++b) {
        const unsigned it = grp * IB + b;
        item[b] = it < a.batch ? it : a.batch - 1;
        dp[b] = a.digits_ntt + (item[b] * (L + 1) + k) * (size_t)L * n;
    }
    const bool diag = a.diag_from_ct && k < L;
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        u64 r[IB][2][2];
#pragma unroll
        for (int b = 0; b < IB; ++b) r[b][0][0] = r[b][0][1] = r[b][1][0] = r[b][1][1] = 0;
        for (unsigned u = 0; u < a.terms_per_slot; ++u) {
            const size_t t = (size_t)slot * a.terms_per_slot + u;
            const unsigned src = hoist_ntt_source(x, (unsigned)a.elements[t], a.log_n);
            const unsigned pair = src & ~1u;
            const bool swap = src & 1u;
            u64 lo[IB][2][2], hi[IB][2][2];
#pragma unroll
            for (int b = 0; b < IB; ++b)
#pragma unroll
                for (int c = 0; c < 2; ++c) lo[b][c][0] = lo[b][c][1] = hi[b][c][0] = hi[b][c][1] = 0;
            for (unsigned j = 0; j < L; ++j) {
                const u64* kj = a.keys[t * L + j] + (size_t)key_index * n + x;
                const u64x2 k0 = ld2(kj), k1 = ld2(kj + key_poly);
#pragma unroll
                for (int b = 0; b < IB; ++b) {
                    const u64* drow = (diag && j == k) ? a.ct + (item[b] * 2 + 1) * (size_t)L * n + (size_t)j * n : dp[b] + (size_t)j * n;
                    const u64x2 v = ld2(drow + pair);
                    const u64 d0 = swap ? v.b : v.a, d1 = swap ? v.a : v.b;
                    mac128(lo[b][0][0], hi[b][0][0], d0, k0.a); mac128(lo[b][0][1], hi[b][0][1], d1, k0.b);
                    mac128(lo[b][1][0], hi[b][1][0], d0, k1.a); mac128(lo[b][1][1], hi[b][1][1], d1, k1.b);
                }
            }
#pragma unroll
            for (int b = 0; b < IB; ++b)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    r[b][c][0] = add_mod(r[b][c][0], barrett128(lo[b][c][0], hi[b][c][0], md.q, md.ratio_lo, md.ratio_hi), md.q);
                    r[b][c][1] = add_mod(r[b][c][1], barrett128(lo[b][c][1], hi[b][c][1], md.q, md.ratio_lo, md.ratio_hi), md.q);
                }
        }
#pragma unroll
        for (int b = 0; b < IB; ++b) {
            if (grp * IB + b >= a.batch) break;
            u64* pp = a.poly_prod + ((size_t)slot * a.batch + item[b]) * 2 * (size_t)(L + 1) * n + (size_t)k * n + x;
            st2(pp, r[b][0][0], r[b][0][1]);
            st2(pp + (size_t)(L + 1) * n, r[b][1][0], r[b][1][1]);
        }
    }
}

// one thread per coefficient of (slot, item, limb); rows = slots * batch * L
__global__ __launch_bounds__(POLY_BLOCK) void hoist_c0_kernel(unsigned chunks, HoistArgs a) {
    const unsigned L = a.L, n = 1u << a.log_n, mask = n - 1;
    const unsigned row = blk_row(chunks);
    const unsigned l = row % L;
    const size_t item = (row / L) % a.batch;
    const size_t slot = row / L / a.batch;
    const u64 q = a.mods[l].q;
    const u64* ip = a.ct + (item * 2 * L + l) * (size_t)n;
    u64* op = a.dest + ((slot * a.batch + item) * 2 * L + l) * (size_t)n;
    for (unsigned x = blk_col(chunks); x < n; x += chunks * blockDim.x) {
        u64 sum = 0;
        for (unsigned u = 0; u < a.terms_per_slot; ++u) {
            const size_t t = slot * a.terms_per_slot + u;
            const unsigned g = (unsigned)a.elements[t];
            u64 v;
            if (a.is_ntt_form) {
                v = ip[hoist_ntt_source(x, g, a.log_n)];
            } else {
                const unsigned i = (unsigned)((u64)x * a.inv_elements[t]) & mask;
                v = ip[i];
                if ((((u64)i * g) >> a.log_n) & 1) v = neg_mod(v, q);
            }
            sum = add_mod(sum, v, q);
        }
        op[x] = sum;
    }
}

struct HoistWeightedArgs {
    const DevModulus* mods;
    unsigned K, L, log_n, batch;
    unsigned groups;               // ceil(batch / IB)
    unsigned terms;
    const u64* digits_ntt;         // D [batch][L+1][L][N]
    const u64* c0_ntt;             // NTT-form limbs of c0: item b, limb l at c0_ntt + b * c0_bstride + l * N
    size_t c0_bstride;
    const u64* c1_ntt;             // NTT-form limb l of c1 at c1_ntt + b * c1_bstride + l * c1_lstride (the ciphertext, or the diagonal block D[l][l])
    size_t c1_bstride, c1_lstride;
    int diag_from_c1;              // skip_diag: digit k of row k < L was not produced, it is c1's NTT-form limb k
    const u64* const* keys;        // device table [terms][L] -> u64[2][K][N]; the entries of an identity term are not read
    const u64* elements;           // device table [terms]
    const u64* const* weights;     // device table [slots][terms] -> u64[K][N], null = the term is absent from the slot
    const u64* special_mod;        // device table [L]: q_special mod q_l
    u64* poly_prod;                // [slots][batch][2][L+1][N]
};

template <int IB>
__global__ __launch_bounds__(POLY_BLOCK) void hoist_weighted_kernel(unsigned chunks, HoistWeightedArgs a) {
    const unsigned L = a.L, K = a.K, n = 1u << a.log_n;
    const unsigned row = blk_row(chunks);
    const unsigned k = row % (L + 1);
    const unsigned grp = (row / (L + 1)) % a.groups;
    const unsigned slot = row / (L + 1) / a.groups;
    const unsigned key_index = (k == L) ? K - 1 : k;
    const DevModulus md = a.mods[key_index];
    const size_t key_poly = (size_t)K * n;
    const bool data_row = k < L;
    const u64 special = data_row ? a.special_mod[k] : 0;
    // items past the batch's end recompute the last item and store nothing
    size_t item[IB];
    const u64 *dp[IB], *c0p[IB], *c1p[IB];
#pragma unroll
    for (int b = 0; b < IB; ++b) {
        const unsigned it = grp * IB + b;
        item[b] = it < a.batch ? it : a.batch - 1;
        dp[b] = a.digits_ntt + (item[b] * (L + 1) + k) * (size_t)L * n;
        c0p[b] = a.c0_ntt + item[b] * a.c0_bstride + (size_t)(data_row ? k : 0) * n;
        c1p[b] = a.c1_ntt + item[b] * a.c1_bstride + (size_t)(data_row ? k : 0) * a.c1_lstride;
    }
    const bool diag = a.diag_from_c1 && data_row;
    const u64* const* wrow = a.weights + (size_t)slot * a.terms;
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        u64 r[IB][2][2];
#pragma unroll
        for (int b = 0; b < IB; ++b) r[b][0][0] = r[b][0][1] = r[b][1][0] = r[b][1][1] = 0;
        for (unsigned t = 0; t < a.terms; ++t) {
            const u64* w = wrow[t];
            if (!w) continue;                                           // uniform over the grid row: the term is absent from this slot
            const u64x2 wv = ld2(w + (size_t)key_index * n + x);
            const unsigned g = (unsigned)a.elements[t];
            const unsigned src = hoist_ntt_source(x, g, a.log_n);
            const unsigned pair = src & ~1u;
            const bool swap = src & 1u;
            if (g != 1) {
                u64 lo[IB][2][2], hi[IB][2][2];
#pragma unroll
                for (int b = 0; b < IB; ++b)
#pragma unroll
                    for (int c = 0; c < 2; ++c) lo[b][c][0] = lo[b][c][1] = hi[b][c][0] = hi[b][c][1] = 0;
                for (unsigned j = 0; j < L; ++j) {
                    const u64* kj = a.keys[(size_t)t * L + j] + (size_t)key_index * n + x;
                    const u64x2 k0 = ld2(kj), k1 = ld2(kj + key_poly);
#pragma unroll
                    for (int b = 0; b < IB; ++b) {
                        const u64* drow = (diag && j == k) ? c1p[b] : dp[b] + (size_t)j * n;
                        const u64x2 v = ld2(drow + pair);
                        const u64 d0 = swap ? v.b : v.a, d1 = swap ? v.a : v.b;
                        mac128(lo[b][0][0], hi[b][0][0], d0, k0.a); mac128(lo[b][0][1], hi[b][0][1], d1, k0.b);
                        mac128(lo[b][1][0], hi[b][1][0], d0, k1.a); mac128(lo[b][1][1], hi[b][1][1], d1, k1.b);
                    }
                }
#pragma unroll
                for (int b = 0; b < IB; ++b)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const u64 p0 = barrett128(lo[b][c][0], hi[b][c][0], md.q, md.ratio_lo, md.ratio_hi);
                        const u64 p1 = barrett128(lo[b][c][1], hi[b][c][1], md.q, md.ratio_lo, md.ratio_hi);
                        r[b][c][0] = add_mod(r[b][c][0], mul_mod(p0, wv.a, md), md.q);
                        r[b][c][1] = add_mod(r[b][c][1], mul_mod(p1, wv.b, md), md.q);
                    }
            }
            if (data_row) {
                // the unkeyed contributions, scaled by q_special: c0 under every term, c1 under the identity
                const u64 ws0 = mul_mod(wv.a, special, md), ws1 = mul_mod(wv.b, special, md);
#pragma unroll
                for (int b = 0; b < IB; ++b) {
                    const u64x2 v = ld2(c0p[b] + pair);
                    r[b][0][0] = add_mod(r[b][0][0], mul_mod(swap ? v.b : v.a, ws0, md), md.q);
                    r[b][0][1] = add_mod(r[b][0][1], mul_mod(swap ? v.a : v.b, ws1, md), md.q);
                    if (g == 1) {
                        const u64x2 v1 = ld2(c1p[b] + x);
                        r[b][1][0] = add_mod(r[b][1][0], mul_mod(v1.a, ws0, md), md.q);
                        r[b][1][1] = add_mod(r[b][1][1], mul_mod(v1.b, ws1, md), md.q);
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < IB; ++b) {
            if (grp * IB + b >= a.batch) break;
            u64* pp = a.poly_prod + ((size_t)slot * a.batch + item[b]) * 2 * (size_t)(L + 1) * n + (size_t)k * n + x;
            st2(pp, r[b][0][0], r[b][0][1]);
            st2(pp + (size_t)(L + 1) * n, r[b][1][0], r[b][1][1]);
        }
    }
}

// hoist_each_kernel (troyn_apply_galois_sum_each): the rows, pairs and gather of hoist_mac_kernel with ONE CIPHERTEXT PER TERM,
//     poly_prod[item][c][k][i] (+)= SUM_t ( SUM_j D[t][item][k][j][pi_t(i)] * key_{t,j}[c][k][i]                                  (g_t != 1)
//                                         + (q_special mod q_k) * u_{t,c}[item][k][pi_t(i)] )  mod m_k                            (k < L)
//   u_{t,0} = the NTT-form limbs of c0 of term t, u_{t,1} = those of c1 of an identity term and nothing otherwise, injected as
//   hoist_weighted_kernel injects them.  The digit row pointer depends on the term: every term streams its own digits, 8 L (L+1) N bytes
//   per item and term next to 16 L (L+1) N bytes of keys per term -- at IB = 4 about twice the key stream.  The 128-bit accumulator runs
//   over the L digits of a term, one Barrett-128 per term and word, then an addition modulo m_k.  The host resides the digits of at most
//   TROYN_HOIST_EACH_GROUP terms at once; `accumulate` makes a later group add into poly_prod modulo m_k (modular addition is associative:
//   the words do not depend on the grouping).  The keys of an identity term are never read.  No LDS, no scratch.
struct HoistEachArgs {
    const DevModulus* mods;
    unsigned K, L, log_n, batch;
    unsigned groups;               // ceil(batch / IB)
    unsigned terms;                // the terms of this launch (one group)
    int accumulate;                // a later group: add into poly_prod
    const u64* digits_ntt;         // D [terms][batch][L+1][L][N]
    const u64* c0_ntt;             // NTT-form limbs of c0: term t, item b, limb l at c0_ntt + (t * batch + b) * c0_bstride + l * N
    size_t c0_bstride;
    const u64* c1_ntt;             // NTT-form limb l of c1 at c1_ntt + (t * batch + b) * c1_bstride + l * c1_lstride (the ciphertext, or D[l][l])
    size_t c1_bstride, c1_lstride;
    int diag_from_c1;              // skip_diag: digit k of row k < L was not produced, it is c1's NTT-form limb k
    const u64* const* keys;        // device table [terms][L] -> u64[2][K][N]; the entries of an identity term are not read
    const u64* elements;           // device table [terms]
    const u64* special_mod;        // device table [L]: q_special mod q_l
    u64* poly_prod;                // [batch][2][L+1][N]
};

template <int IB>
__global__ __launch_bounds__(POLY_BLOCK) void hoist_each_kernel(unsigned chunks, HoistEachArgs a) {
    const unsigned L = a.L, K = a.K, n = 1u << a.log_n;
    const unsigned row = blk_row(chunks);
    const unsigned k = row % (L + 1);
    const unsigned grp = row / (L + 1);
    const unsigned key_index = (k == L) ? K - 1 : k;
    const DevModulus md = a.mods[key_index];
    const size_t key_poly = (size_t)K * n;
    const size_t digit_item = (size_t)(L + 1) * L * n;
    const bool data_row = k < L;
    const u64 special = data_row ? a.special_mod[k] : 0;
    const bool diag = a.diag_from_c1 && data_row;
    // items past the batch's end recompute the last item and store nothing
    size_t item[IB];
#pragma unroll
    for (int b = 0; b < IB; ++b) {
        const unsigned it = grp * IB + b;
        item[b] = it < a.batch ? it : a.batch - 1;
    }
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        u64 r[IB][2][2];
#pragma unroll
        for (int b = 0; b < IB; ++b) {
            if (a.accumulate) {
                const u64* pp = a.poly_prod + item[b] * 2 * (size_t)(L + 1) * n + (size_t)k * n + x;
                const u64x2 p0 = ld2(pp), p1 = ld2(pp + (size_t)(L + 1) * n);
                r[b][0][0] = p0.a; r[b][0][1] = p0.b; r[b][1][0] = p1.a; r[b][1][1] = p1.b;
            } else r[b][0][0] = r[b][0][1] = r[b][1][0] = r[b][1][1] = 0;
        }
        for (unsigned t = 0; t < a.terms; ++t) {
            const unsigned g = (unsigned)a.elements[t];
            const unsigned src = hoist_ntt_source(x, g, a.log_n);
            const unsigned pair = src & ~1u;
            const bool swap = src & 1u;
            const size_t first = (size_t)t * a.batch;      // the term's first ciphertext
            if (g != 1) {
                u64 lo[IB][2][2], hi[IB][2][2];
#pragma unroll
                for (int b = 0; b < IB; ++b)
#pragma unroll
                    for (int c = 0; c < 2; ++c) lo[b][c][0] = lo[b][c][1] = hi[b][c][0] = hi[b][c][1] = 0;
                for (unsigned j = 0; j < L; ++j) {
                    const u64* kj = a.keys[(size_t)t * L + j] + (size_t)key_index * n + x;
                    const u64x2 k0 = ld2(kj), k1 = ld2(kj + key_poly);
#pragma unroll
                    for (int b = 0; b < IB; ++b) {
                        const u64* drow = (diag && j == k) ? a.c1_ntt + (first + item[b]) * a.c1_bstride + (size_t)k * a.c1_lstride
                                                           : a.digits_ntt + (first + item[b]) * digit_item + ((size_t)k * L + j) * n;
                        const u64x2 v = ld2(drow + pair);
                        const u64 d0 = swap ? v.b : v.a, d1 = swap ? v.a : v.b;
                        mac128(lo[b][0][0], hi[b][0][0], d0, k0.a); mac128(lo[b][0][1], hi[b][0][1], d1, k0.b);
                        mac128(lo[b][1][0], hi[b][1][0], d0, k1.a); mac128(lo[b][1][1], hi[b][1][1], d1, k1.b);
                    }
                }
#pragma unroll
                for (int b = 0; b < IB; ++b)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        r[b][c][0] = add_mod(r[b][c][0], barrett128(lo[b][c][0], hi[b][c][0], md.q, md.ratio_lo, md.ratio_hi), md.q);
                        r[b][c][1] = add_mod(r[b][c][1], barrett128(lo[b][c][1], hi[b][c][1], md.q, md.ratio_lo, md.ratio_hi), md.q);
                    }
            }
            if (data_row) {
                // the unkeyed contributions, scaled by q_special: c0 under every term, c1 under the identity
#pragma unroll
                for (int b = 0; b < IB; ++b) {
                    const u64x2 v = ld2(a.c0_ntt + (first + item[b]) * a.c0_bstride + (size_t)k * n + pair);
                    r[b][0][0] = add_mod(r[b][0][0], mul_mod(swap ? v.b : v.a, special, md), md.q);
                    r[b][0][1] = add_mod(r[b][0][1], mul_mod(swap ? v.a : v.b, special, md), md.q);
                    if (g == 1) {
                        const u64x2 v1 = ld2(a.c1_ntt + (first + item[b]) * a.c1_bstride + (size_t)k * a.c1_lstride + x);
                        r[b][1][0] = add_mod(r[b][1][0], mul_mod(v1.a, special, md), md.q);
                        r[b][1][1] = add_mod(r[b][1][1], mul_mod(v1.b, special, md), md.q);
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < IB; ++b) {
            if (grp * IB + b >= a.batch) break;
            u64* pp = a.poly_prod + item[b] * 2 * (size_t)(L + 1) * n + (size_t)k * n + x;
            st2(pp, r[b][0][0], r[b][0][1]);
            st2(pp + (size_t)(L + 1) * n, r[b][1][0], r[b][1][1]);
        }
    }
}

// hoist_double_kernel (troyn_linear_transform_bsgs_double_hoisted): the rows, item groups, gather and term groups of hoist_each_kernel for
// the outer stage of the double-hoisted BSGS transform.  Term t is a giant step; x_ntt holds the inner stage's extended-basis sums
// X^(t)[item][c][k] in NTT form (hoist_weighted_kernel's output, unkeyed contributions already injected), digits_ntt the transformed digits
// of v^(t), the divided component 1 of X^(t):
//     poly_prod[item][c][k][i] (+)= SUM_t ( SUM_j D[t][item][k][j][pi_t(i)] * key_{t,j}[c][k][i]  +  [c = 0] X^(t)[item][0][k][pi_t(i)] )    (g_t != 1)
//                                         X^(t)[item][c][k][i]                                                                                (g_t  = 1)
//   mod m_k on EVERY row k = 0 .. L, the special row included: component 0 stays on the extended basis, so nothing is scaled by q_special
//   here and no c0 is transformed -- the gather of X_0 replaces hoist_each_kernel's injection.  An identity term reads no digits and no
//   keys.  Per item and non-identity term a row streams 8 L N bytes of digits and 8 N bytes of X_0 next to the 16 L N bytes of keys the
//   items share.  No LDS, no scratch.
struct HoistDoubleArgs {
    const DevModulus* mods;
    unsigned K, L, log_n, batch;
    unsigned groups;               // ceil(batch / IB)
    unsigned terms;                // the giant steps of this launch (one group)
    int accumulate;                // a later group: add into poly_prod
    const u64* digits_ntt;         // D [terms][batch][L+1][L][N]; the blocks of an identity term are not read
    const u64* v_ntt;              // NTT-form limb l of v^(t) of item b at v_ntt + ((t * batch + b) * L + l) * N (read when diag_from_v)
    int diag_from_v;               // skip_diag: digit k of row k < L was not produced, it is v's NTT-form limb k
    const u64* x_ntt;              // X [terms][batch][2][L+1][N]
    const u64* const* keys;        // device table [terms][L] -> u64[2][K][N]; the entries of an identity term are not read
    const u64* elements;           // device table [terms]
    u64* poly_prod;                // [batch][2][L+1][N]
};

template <int IB>
__global__ __launch_bounds__(POLY_BLOCK) void hoist_double_kernel(unsigned chunks, HoistDoubleArgs a) {
    const unsigned L = a.L, K = a.K, n = 1u << a.log_n;
    const unsigned row = blk_row(chunks);
    const unsigned k = row % (L + 1);
    const unsigned grp = row / (L + 1);
    const unsigned key_index = (k == L) ? K - 1 : k;
    const DevModulus md = a.mods[key_index];
    const size_t key_poly = (size_t)K * n;
    const size_t digit_item = (size_t)(L + 1) * L * n;
    const size_t comp = (size_t)(L + 1) * n;
    const bool diag = a.diag_from_v && k < L;
    // items past the batch's end recompute the last item and store nothing
    size_t item[IB];
#pragma unroll
    for (int b = 0; b < IB; ++b) {
        const unsigned it = grp * IB + b;
        item[b] = it < a.batch ? it : a.batch - 1;
    }
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        u64 r[IB][2][2];
#pragma unroll
        for (int b = 0; b < IB; ++b) {
            if (a.accumulate) {
                const u64* pp = a.poly_prod + item[b] * 2 * comp + (size_t)k * n + x;
                const u64x2 p0 = ld2(pp), p1 = ld2(pp + comp);
                r[b][0][0] = p0.a; r[b][0][1] = p0.b; r[b][1][0] = p1.a; r[b][1][1] = p1.b;
            } else r[b][0][0] = r[b][0][1] = r[b][1][0] = r[b][1][1] = 0;
        }
        for (unsigned t = 0; t < a.terms; ++t) {
            const unsigned g = (unsigned)a.elements[t];
            const size_t first = (size_t)t * a.batch;      // the term's first item
            if (g != 1) {
                const unsigned src = hoist_ntt_source(x, g, a.log_n);
                const unsigned pair = src & ~1u;
                const bool swap = src & 1u;
                u64 lo[IB][2][2], hi[IB][2][2];
#pragma unroll
                for (int b = 0; b < IB; ++b)
#pragma unroll
                    for (int c = 0; c < 2; ++c) lo[b][c][0] = lo[b][c][1] = hi[b][c][0] = hi[b][c][1] = 0;
                for (unsigned j = 0; j < L; ++j) {
                    const u64* kj = a.keys[(size_t)t * L + j] + (size_t)key_index * n + x;
                    const u64x2 k0 = ld2(kj), k1 = ld2(kj + key_poly);
#pragma unroll
                    for (int b = 0; b < IB; ++b) {
                        const u64* drow = (diag && j == k) ? a.v_ntt + ((first + item[b]) * L + k) * (size_t)n
                                                           : a.digits_ntt + (first + item[b]) * digit_item + ((size_t)k * L + j) * n;
                        const u64x2 v = ld2(drow + pair);
                        const u64 d0 = swap ? v.b : v.a, d1 = swap ? v.a : v.b;
                        mac128(lo[b][0][0], hi[b][0][0], d0, k0.a); mac128(lo[b][0][1], hi[b][0][1], d1, k0.b);
                        mac128(lo[b][1][0], hi[b][1][0], d0, k1.a); mac128(lo[b][1][1], hi[b][1][1], d1, k1.b);
                    }
                }
#pragma unroll
                for (int b = 0; b < IB; ++b) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        r[b][c][0] = add_mod(r[b][c][0], barrett128(lo[b][c][0], hi[b][c][0], md.q, md.ratio_lo, md.ratio_hi), md.q);
                        r[b][c][1] = add_mod(r[b][c][1], barrett128(lo[b][c][1], hi[b][c][1], md.q, md.ratio_lo, md.ratio_hi), md.q);
                    }
                    // sigma_g of row k of X_0, the special row included: the permutation of the NTT-form words
                    const u64x2 v = ld2(a.x_ntt + (first + item[b]) * 2 * comp + (size_t)k * n + pair);
                    r[b][0][0] = add_mod(r[b][0][0], swap ? v.b : v.a, md.q);
                    r[b][0][1] = add_mod(r[b][0][1], swap ? v.a : v.b, md.q);
                }
            } else {
                // the identity giant step: both components as they are, no division and no key
#pragma unroll
                for (int b = 0; b < IB; ++b) {
                    const u64* xp = a.x_ntt + (first + item[b]) * 2 * comp + (size_t)k * n + x;
                    const u64x2 v0 = ld2(xp), v1 = ld2(xp + comp);
                    r[b][0][0] = add_mod(r[b][0][0], v0.a, md.q); r[b][0][1] = add_mod(r[b][0][1], v0.b, md.q);
                    r[b][1][0] = add_mod(r[b][1][0], v1.a, md.q); r[b][1][1] = add_mod(r[b][1][1], v1.b, md.q);
                }
            }
        }
#pragma unroll
        for (int b = 0; b < IB; ++b) {
            if (grp * IB + b >= a.batch) break;
            u64* pp = a.poly_prod + item[b] * 2 * comp + (size_t)k * n + x;
            st2(pp, r[b][0][0], r[b][0][1]);
            st2(pp + comp, r[b][1][0], r[b][1][1]);
        }
    }
}

}  // namespace troyn
