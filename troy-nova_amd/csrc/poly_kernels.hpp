// poly_kernels.hpp -- streaming (HBM-bound) RNS polynomial kernels: element-wise ops, dyadic
// tensor products, the key-switch inner product and the mod-switch / rescale element steps.
//
// All of them are pure streaming kernels: one thread owns TWO adjacent coefficients so every
// lane issues 16-byte (dwordx4) loads/stores, consecutive lanes touch consecutive addresses,
// and the modulus constants of a limb are wave-uniform.  Grids are sized by the data
// (>> 256 workgroups for any batch worth timing).
#pragma once
#include "dev_math.hpp"
#include "ntt_kernels.hpp"   // KeyPtrs

namespace troyn {

constexpr int POLY_BLOCK = 256;

// 1-D launch geometry shared by every streaming kernel: block = (row, chunk), `chunks` blocks per
// row of N coefficients (grid.y is limited to 65535, a batched launch can exceed that).
__device__ __forceinline__ unsigned blk_row(unsigned chunks) { return blockIdx.x / chunks; }
__device__ __forceinline__ unsigned blk_col(unsigned chunks) { return (blockIdx.x % chunks) * blockDim.x + threadIdx.x; }

struct u64x2 { u64 a, b; };
__device__ __forceinline__ u64x2 ld2(const u64* p) { ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p); return u64x2{v.x, v.y}; }
__device__ __forceinline__ void st2(u64* p, u64 a, u64 b) { *reinterpret_cast<ulonglong2*>(p) = make_ulonglong2(a, b); }

enum { EW_ADD = 0, EW_SUB = 1, EW_NEG = 2, EW_MULS = 3, EW_MUL = 4, EW_MOD = 5, EW_MULOP = 6 };

// data [count][nmod][N]; grid.x covers N/2 pairs, grid.y = count*nmod limb-polynomials
// (utils/poly_small_mod.cu kernel_add_ps / kernel_sub_ps / kernel_negate_ps /
//  kernel_multiply_scalar_ps / kernel_dyadic_product_ps / kernel_modulo_ps / kernel_multiply_uint64operand_ps)
// EW_MOD: Modulus::reduce of ANY 64-bit word; EW_MULOP: b holds one (operand, quotient) pair per limb of the slice
// (MultiplyUint64Operand, utils/uint_small_mod.h:92-139), the input may be any 64-bit word, the result is canonical.
template <int OP>
__global__ __launch_bounds__(POLY_BLOCK) void elementwise_kernel(unsigned chunks, const DevModulus* mods, unsigned mod_start, unsigned nmod,
                                                                 unsigned n, const u64* a, const u64* b, u64 scalar, u64* out) {
    const unsigned limb = blk_row(chunks);
    const DevModulus md = mods[mod_start + limb % nmod];
    const size_t base = (size_t)limb * n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 va = ld2(a + base + i);
        u64 r0, r1;
        if constexpr (OP == EW_ADD) { const u64x2 vb = ld2(b + base + i); r0 = add_mod(va.a, vb.a, md.q); r1 = add_mod(va.b, vb.b, md.q); }
        else if constexpr (OP == EW_SUB) { const u64x2 vb = ld2(b + base + i); r0 = sub_mod(va.a, vb.a, md.q); r1 = sub_mod(va.b, vb.b, md.q); }
        else if constexpr (OP == EW_NEG) { r0 = neg_mod(va.a, md.q); r1 = neg_mod(va.b, md.q); }
        else if constexpr (OP == EW_MULS) { r0 = mul_mod(va.a, scalar, md); r1 = mul_mod(va.b, scalar, md); }
        else if constexpr (OP == EW_MOD) { r0 = barrett64(va.a, md.q, md.ratio_hi); r1 = barrett64(va.b, md.q, md.ratio_hi); }
        else if constexpr (OP == EW_MULOP) {
            const u64x2 w = ld2(b + 2 * (limb % nmod));     // wave-uniform (operand, quotient)
            r0 = shoup_mul(va.a, w.a, w.b, md.q); r1 = shoup_mul(va.b, w.a, w.b, md.q);
        }
        else { const u64x2 vb = ld2(b + base + i); r0 = mul_mod(va.a, vb.a, md); r1 = mul_mod(va.b, vb.b, md); }
        st2(out + base + i, r0, r1);
    }
}

// fgk/dyadic_convolute.cu:6-41 kernel_dyadic_convolute, restructured: one thread computes ALL
// pa+pb-1 outputs of its two coefficients, so each input word is read from HBM exactly once
// (the reference re-reads a_i, b_j once per output polynomial).  PA, PB compile-time (2,2 / 3,2..).
template <int PA, int PB>
__global__ __launch_bounds__(POLY_BLOCK) void dyadic_convolute_kernel(unsigned chunks, const DevModulus* mods, unsigned mod_start, unsigned nmod,
                                                                      unsigned n, const u64* a, const u64* b, u64* out) {
    constexpr int PO = PA + PB - 1;
    const unsigned limb = blk_row(chunks) % nmod;
    const size_t item = blk_row(chunks) / nmod;
    const DevModulus md = mods[mod_start + limb];
    const size_t pc = (size_t)nmod * n;
    const u64* ap = a + item * PA * pc + (size_t)limb * n;
    const u64* bp = b + item * PB * pc + (size_t)limb * n;
    u64* op = out + item * PO * pc + (size_t)limb * n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        u64x2 va[PA], vb[PB];
#pragma unroll
        for (int p = 0; p < PA; ++p) va[p] = ld2(ap + p * pc + i);
#pragma unroll
        for (int p = 0; p < PB; ++p) vb[p] = ld2(bp + p * pc + i);
#pragma unroll
        for (int o = 0; o < PO; ++o) {
            u64 acc0 = 0, acc1 = 0;
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                const int r = o - p;
                if (r >= 0 && r < PB) {
                    acc0 = add_mod(acc0, mul_mod(va[p].a, vb[r].a, md), md.q);
                    acc1 = add_mod(acc1, mul_mod(va[p].b, vb[r].b, md), md.q);
                }
            }
            st2(op + o * pc + i, acc0, acc1);
        }
    }
}

// Sum of `terms` two-by-two tensor products (an addition to the reference's kernels: lazy relinearization of a dot product,
// troyn_dyadic_convolute_accumulate): out[i] (+)= SUM_t a[t][i] (x) b[t][i], a[t], b[t] -> [batch][2][nmod][N], out [batch][3][nmod][N].
// Geometry of dyadic_convolute_kernel<2, 2>: a thread owns two adjacent coefficients of one (item, limb) row, every input word is read once and
// every output word written once per launch.  The three outputs are accumulated in 128 bits (mac128, as ks_accumulate_kernel) and reduced ONCE per
// launch; the sum modulo q in canonical form is the value the per-term reductions of dyadic_convolute + add give.
// Bound: plan moduli are < 2^61, so 64 products plus one canonical carry-in stay below 2^128: 64 (2^61 - 1)^2 + 2^61 < 2^128.  The middle output
// takes TWO products per term, hence at most CONV_ACC_MAX_TERMS = 32 terms per launch; the driver cuts longer sums into launches that carry `out`.
// The pointer tables travel in the kernel arguments (GatherPtrs' pattern); the term loop is wave-uniform and unrolled by UNROLL terms with all
// 4 * UNROLL 16-byte loads issued before the multiplies (the table entries sit in SGPRs, the loads take scalar bases).
constexpr unsigned CONV_ACC_MAX_TERMS = 32;
struct ConvAccPtrs { const u64* a[CONV_ACC_MAX_TERMS]; const u64* b[CONV_ACC_MAX_TERMS]; };

struct ConvAcc128 {
    u64 lo0a = 0, hi0a = 0, lo0b = 0, hi0b = 0;   // output 0, coefficients a / b of the pair
    u64 lo1a = 0, hi1a = 0, lo1b = 0, hi1b = 0;
    u64 lo2a = 0, hi2a = 0, lo2b = 0, hi2b = 0;
    __device__ __forceinline__ void term(const u64x2& a0, const u64x2& a1, const u64x2& b0, const u64x2& b1) {
        mac128(lo0a, hi0a, a0.a, b0.a); mac128(lo0b, hi0b, a0.b, b0.b);
        mac128(lo1a, hi1a, a0.a, b1.a); mac128(lo1b, hi1b, a0.b, b1.b);
        mac128(lo1a, hi1a, a1.a, b0.a); mac128(lo1b, hi1b, a1.b, b0.b);
        mac128(lo2a, hi2a, a1.a, b1.a); mac128(lo2b, hi2b, a1.b, b1.b);
    }
};

template <int UNROLL>
__global__ __launch_bounds__(POLY_BLOCK) void dyadic_convolute_accumulate_kernel(unsigned chunks, const DevModulus* mods, unsigned mod_start, unsigned nmod,
                                                                                 unsigned n, ConvAccPtrs ptrs, unsigned terms, u64* out, int accumulate) {
    const unsigned limb = blk_row(chunks) % nmod;
    const size_t item = blk_row(chunks) / nmod;
    const DevModulus md = mods[mod_start + limb];
    const size_t pc = (size_t)nmod * n;
    const size_t in_off = item * 2 * pc + (size_t)limb * n;
    u64* op = out + item * 3 * pc + (size_t)limb * n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        ConvAcc128 acc;
        if (accumulate) {    // canonical carry-in (the earlier launches of a long sum, or the caller's own `out`)
            const u64x2 c0 = ld2(op + i), c1 = ld2(op + pc + i), c2 = ld2(op + 2 * pc + i);
            acc.lo0a = c0.a; acc.lo0b = c0.b; acc.lo1a = c1.a; acc.lo1b = c1.b; acc.lo2a = c2.a; acc.lo2b = c2.b;
        }
        unsigned t = 0;
        for (; t + UNROLL <= terms; t += UNROLL) {
            u64x2 a0[UNROLL], a1[UNROLL], b0[UNROLL], b1[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const u64* ap = ptrs.a[t + u] + in_off + i;
                const u64* bp = ptrs.b[t + u] + in_off + i;
                a0[u] = ld2(ap); a1[u] = ld2(ap + pc); b0[u] = ld2(bp); b1[u] = ld2(bp + pc);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) acc.term(a0[u], a1[u], b0[u], b1[u]);
        }
        for (; t < terms; ++t) {
            const u64* ap = ptrs.a[t] + in_off + i;
            const u64* bp = ptrs.b[t] + in_off + i;
            const u64x2 a0 = ld2(ap), a1 = ld2(ap + pc), b0 = ld2(bp), b1 = ld2(bp + pc);
            acc.term(a0, a1, b0, b1);
        }
        st2(op + i, barrett128(acc.lo0a, acc.hi0a, md.q, md.ratio_lo, md.ratio_hi), barrett128(acc.lo0b, acc.hi0b, md.q, md.ratio_lo, md.ratio_hi));
        st2(op + pc + i, barrett128(acc.lo1a, acc.hi1a, md.q, md.ratio_lo, md.ratio_hi), barrett128(acc.lo1b, acc.hi1b, md.q, md.ratio_lo, md.ratio_hi));
        st2(op + 2 * pc + i, barrett128(acc.lo2a, acc.hi2a, md.q, md.ratio_lo, md.ratio_hi), barrett128(acc.lo2b, acc.hi2b, md.q, md.ratio_lo, md.ratio_hi));
    }
}

// Scalar-weighted sums of ciphertexts (an addition to the reference's kernels, troyn_scalar_weighted_sums): a small dense matrix of residues
// times a vector of ciphertexts, out[s] = SUM_t scalars[s][t] * in[t] (+ constants[s]), in[t] -> [batch][pcount][in_nmod[t]][N] of which only the
// first nmod limbs are read, out [slots][batch][pcount][nmod][N].
// Geometry of dyadic_convolute_accumulate_kernel: a thread owns two adjacent coefficients of one (item, polynomial, limb) row.  New is the SLOT
// TILE: the thread keeps the 128-bit accumulators of TS slots (8 * TS VGPRs), an input word loaded once is multiplied into all of them, so
// the inputs are read ceil(slots / TS) times in total (grid = tiles x rows x chunks) and every output word is written once, after ONE
// barrett128.  The last tile may be partial: `live` is wave-uniform, a dead slot costs neither a multiply nor a store.
// Bound: plan moduli are < 2^61, so 64 products plus one canonical carry-in stay below 2^128 (64 (2^61 - 1)^2 + 2^61 < 2^128); an
// accumulator takes ONE product per term, hence at most SSUM_MAX_TERMS = 64 terms per launch.  The driver cuts longer sums into launches
// that carry `out`; the constant is added after the reduction of the last launch (add_mod), so it does not count against the bound.
// The pointer table travels in the kernel arguments; the scalars come from a table the driver lays out as [tile][limb][term][TS], so the
// TS residues of a (tile, limb, term) are one wave-uniform run that the compiler fetches with scalar loads into SGPRs.  The term loop is
// wave-uniform and unrolled by UNROLL terms with all UNROLL 16-byte loads issued before the multiplies.  No LDS, no scratch.
constexpr unsigned SSUM_MAX_TERMS = 64;
struct ScalarSumPtrs { const u64* in[SSUM_MAX_TERMS]; unsigned in_nmod[SSUM_MAX_TERMS]; };

template <int TS, int UNROLL>
__global__ __launch_bounds__(POLY_BLOCK) void scalar_weighted_sums_kernel(unsigned chunks, const DevModulus* __restrict__ mods, unsigned mod_start, unsigned nmod,
                                                                          unsigned n, ScalarSumPtrs ptrs, unsigned terms,
                                                                          const u64* __restrict__ scal, unsigned scal_terms, unsigned term0,
                                                                          const u64* __restrict__ consts, int constant_at_index0, unsigned pcount,
                                                                          unsigned rows, unsigned slots, u64* __restrict__ out, int carry) {
    const unsigned tile = blk_row(chunks) / rows;
    const unsigned r = blk_row(chunks) % rows;      // (item * pcount + c) * nmod + limb
    const unsigned limb = r % nmod;
    const size_t pi = r / nmod;
    const DevModulus md = mods[mod_start + limb];
    const unsigned slot0 = tile * TS;
    const unsigned live = slots - slot0 < (unsigned)TS ? slots - slot0 : (unsigned)TS;
    const u64* w = scal + (((size_t)tile * nmod + limb) * scal_terms + term0) * TS;
    u64* op = out + ((size_t)slot0 * rows + r) * n;
    const size_t slot_stride = (size_t)rows * n;
    const bool with_const = consts && pi % pcount == 0;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        u64 loa[TS], hia[TS], lob[TS], hib[TS];
#pragma unroll
        for (int s = 0; s < TS; ++s) {
            loa[s] = hia[s] = lob[s] = hib[s] = 0;
            if (carry && s < (int)live) {    // canonical carry-in: the earlier launches of a long sum
                const u64x2 c = ld2(op + s * slot_stride + i);
                loa[s] = c.a; lob[s] = c.b;
            }
        }
        unsigned t = 0;
        for (; t + UNROLL <= terms; t += UNROLL) {
            u64x2 v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) v[u] = ld2(ptrs.in[t + u] + (pi * ptrs.in_nmod[t + u] + limb) * n + i);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
                for (int s = 0; s < TS; ++s) {
                    if (s < (int)live) {
                        const u64 k = w[(size_t)(t + u) * TS + s];
                        mac128(loa[s], hia[s], v[u].a, k); mac128(lob[s], hib[s], v[u].b, k);
                    }
                }
            }
        }
        for (; t < terms; ++t) {
            const u64x2 v = ld2(ptrs.in[t] + (pi * ptrs.in_nmod[t] + limb) * n + i);
#pragma unroll
            for (int s = 0; s < TS; ++s) {
                if (s < (int)live) {
                    const u64 k = w[(size_t)t * TS + s];
                    mac128(loa[s], hia[s], v.a, k); mac128(lob[s], hib[s], v.b, k);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < TS; ++s) {
            if (s < (int)live) {
                u64 r0 = barrett128(loa[s], hia[s], md.q, md.ratio_lo, md.ratio_hi), r1 = barrett128(lob[s], hib[s], md.q, md.ratio_lo, md.ratio_hi);
                if (with_const) {
                    const u64 c = consts[(size_t)(slot0 + s) * nmod + limb];
                    if (!constant_at_index0) { r0 = add_mod(r0, c, md.q); r1 = add_mod(r1, c, md.q); }
                    else if (i == 0) r0 = add_mod(r0, c, md.q);
                }
                st2(op + s * slot_stride + i, r0, r1);
            }
        }
    }
}

// Tensor product plus affine part (an addition to the reference's kernels, troyn_ckks_multiply_affine_relinearize_rescale): the Chebyshev
// step 2 T_a T_b - T_c and the double angle 2 x^2 - 1 before their ONE relinearize and rescale.  Per item of the batch
//   P_0 = alpha (a0 . b0) + w c0 + k,   P_1 = alpha (a0 . b1 + a1 . b0) + w c1,   P_2 = alpha (a1 . b1)
// a[i], b[i] -> [2][nmod][N], c[i] -> [2][c_nmod[i]][N] (only the first nmod limbs are read) or null (no addend), out [items][3][nmod][N].
// Geometry of dyadic_convolute_accumulate_kernel: a thread owns two adjacent coefficients of one (item, limb) row; every word of a, b and c is read
// ONCE with a 16-byte load and every word of P written once.  Headroom: plan moduli are < 2^61, so a0 b1 + a1 b0 < 2^123 is reduced (barrett128)
// BEFORE it meets alpha; then t alpha + w c + k < 2^123 + 2^61 takes the one final reduction of the word.  The sum modulo q in canonical form is
// the value that multiply_scalar, add and the constant give step by step.
// The item pointers travel in the kernel arguments, at most MAFF_MAX_ITEMS items per launch; the per-(item, limb) scalars come from a table
// [item][limb][4] = (alpha, w, k, 0), one wave-uniform 32-byte run that the compiler fetches with a scalar load.  The "has an addend" branch is
// wave-uniform and taken OUTSIDE the coefficient loop (a select per load would serialise the loads).  No LDS, no scratch.
constexpr unsigned MAFF_MAX_ITEMS = 32;
struct MulAffinePtrs { const u64* a[MAFF_MAX_ITEMS]; const u64* b[MAFF_MAX_ITEMS]; const u64* c[MAFF_MAX_ITEMS]; unsigned c_nmod[MAFF_MAX_ITEMS]; };

__device__ __forceinline__ u64 affine_word(u64 lo, u64 hi, u64 alpha, u64 w, u64 c, u64 k, const DevModulus& md) {
    const u64 t = barrett128(lo, hi, md.q, md.ratio_lo, md.ratio_hi);
    u64 l, h;
    mul128(t, alpha, l, h);
    mac128(l, h, w, c);
    const u128 acc = (((u128)h << 64) | l) + k;
    return barrett128((u64)acc, (u64)(acc >> 64), md.q, md.ratio_lo, md.ratio_hi);
}

template <bool HAS_C>
__device__ __forceinline__ void multiply_affine_row(unsigned chunks, const DevModulus& md, unsigned n, size_t pc, const u64* ap, const u64* bp,
                                                    const u64* cp, size_t c_pc, u64 alpha, u64 w, u64 k, u64* op) {
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 a0 = ld2(ap + i), a1 = ld2(ap + pc + i), b0 = ld2(bp + i), b1 = ld2(bp + pc + i);
        u64x2 c0{0, 0}, c1{0, 0};
        if constexpr (HAS_C) { c0 = ld2(cp + i); c1 = ld2(cp + c_pc + i); }
        const u64 wc = HAS_C ? w : 0;
        u64 lo, hi, r0, r1;
        mul128(a0.a, b0.a, lo, hi); r0 = affine_word(lo, hi, alpha, wc, c0.a, k, md);
        mul128(a0.b, b0.b, lo, hi); r1 = affine_word(lo, hi, alpha, wc, c0.b, k, md);
        st2(op + i, r0, r1);
        mul128(a0.a, b1.a, lo, hi); mac128(lo, hi, a1.a, b0.a); r0 = affine_word(lo, hi, alpha, wc, c1.a, 0, md);
        mul128(a0.b, b1.b, lo, hi); mac128(lo, hi, a1.b, b0.b); r1 = affine_word(lo, hi, alpha, wc, c1.b, 0, md);
        st2(op + pc + i, r0, r1);
        r0 = mul_mod(mul_mod(a1.a, b1.a, md), alpha, md);      // P_2 has no affine part
        r1 = mul_mod(mul_mod(a1.b, b1.b, md), alpha, md);
        st2(op + 2 * pc + i, r0, r1);
    }
}

// scal: the table of the launch's first item; out: P of the launch's first item
__global__ __launch_bounds__(POLY_BLOCK) void multiply_affine_kernel(unsigned chunks, const DevModulus* __restrict__ mods, unsigned nmod, unsigned n,
                                                                     MulAffinePtrs ptrs, const u64* __restrict__ scal, u64* __restrict__ out) {
    const unsigned limb = blk_row(chunks) % nmod;
    const unsigned item = blk_row(chunks) / nmod;      // < MAFF_MAX_ITEMS: the grid is items * nmod * chunks blocks
    const DevModulus md = mods[limb];
    const size_t pc = (size_t)nmod * n;
    const size_t in_off = (size_t)limb * n;
    const u64* s = scal + ((size_t)item * nmod + limb) * 4;
    const u64 alpha = s[0], w = s[1], k = s[2];
    const u64* cp = ptrs.c[item];
    u64* op = out + (size_t)item * 3 * pc + in_off;
    if (cp) multiply_affine_row<true>(chunks, md, n, pc, ptrs.a[item] + in_off, ptrs.b[item] + in_off, cp + in_off, (size_t)ptrs.c_nmod[item] * n, alpha, w, k, op);
    else multiply_affine_row<false>(chunks, md, n, pc, ptrs.a[item] + in_off, ptrs.b[item] + in_off, nullptr, 0, alpha, 0, k, op);
}

// Real and imaginary parts of CKKS slots (additions to the reference's kernels, troyn_ckks_complex_split / troyn_ckks_complex_join): the level-free
// multiplication by i.  mu is the forward transform of the monomial X^(N/2): iota = psi^(N/2), the square root of -1 that the forward twiddle table holds
// at index 1 (bit_reverse(N/2)), on the lower half of a row and q - iota on the upper half -- the first butterfly layer sends the one non-zero
// coefficient N/2 to (+iota, -iota) at distance N/2 and every later layer copies it within its half.
//   split:  s = a + b,  d = mu . (b - a)        join:  out = a + mu . b        all modulo q_l, canonical words in and out
// a, b, s, d, out -> [rows][N], rows = items * 2 * nmod, the limb of a row is row % nmod.  Geometry of multiply_affine_kernel: a thread owns two adjacent
// coefficients of one row, 16-byte loads and stores, every input word read once and every output word written once, no LDS.  (iota, its Shoup quotient)
// is one wave-uniform 16-byte load per workgroup.  The half of the row picks the ORDER of the difference (split) or the sign of b (join) with a
// select, so q - iota is never formed: iota (b - a) below N/2, iota (a - b) above.  x + q - y lies in [1, 2q) and Shoup's product takes any 64-bit
// word, so a word of d costs one product and one conditional subtraction; a word of out one product and the add_mod.
__device__ __forceinline__ u64 split_word(u64 a, u64 b, bool upper, const ulonglong2& iota, u64 q) {
    return shoup_mul((upper ? a : b) + q - (upper ? b : a), iota.x, iota.y, q);
}
__device__ __forceinline__ u64 join_word(u64 a, u64 b, bool upper, const ulonglong2& iota, u64 q) {
    return add_mod(a, shoup_mul(upper ? q - b : b, iota.x, iota.y, q), q);
}

__global__ __launch_bounds__(POLY_BLOCK) void ckks_complex_split_kernel(unsigned chunks, const DevModulus* __restrict__ mods, const ulonglong2* __restrict__ fwd,
                                                                        unsigned nmod, unsigned n, const u64* a, const u64* b, u64* s, u64* d) {
    const unsigned limb = blk_row(chunks) % nmod;
    const u64 q = mods[limb].q;
    const ulonglong2 iota = fwd[(size_t)limb * n + 1];
    const size_t base = (size_t)blk_row(chunks) * n;
    const unsigned half = n / 2;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 va = ld2(a + base + i), vb = ld2(b + base + i);
        st2(s + base + i, add_mod(va.a, vb.a, q), add_mod(va.b, vb.b, q));
        st2(d + base + i, split_word(va.a, vb.a, i >= half, iota, q), split_word(va.b, vb.b, i + 1 >= half, iota, q));
    }
}

__global__ __launch_bounds__(POLY_BLOCK) void ckks_complex_join_kernel(unsigned chunks, const DevModulus* __restrict__ mods, const ulonglong2* __restrict__ fwd,
                                                                       unsigned nmod, unsigned n, const u64* a, const u64* b, u64* out) {
    const unsigned limb = blk_row(chunks) % nmod;
    const u64 q = mods[limb].q;
    const ulonglong2 iota = fwd[(size_t)limb * n + 1];
    const size_t base = (size_t)blk_row(chunks) * n;
    const unsigned half = n / 2;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 va = ld2(a + base + i), vb = ld2(b + base + i);
        st2(out + base + i, join_word(va.a, vb.a, i >= half, iota, q), join_word(va.b, vb.b, i + 1 >= half, iota, q));
    }
}

// generic (any pa, pb) version with the reference's loop structure
__global__ __launch_bounds__(POLY_BLOCK) void dyadic_convolute_generic_kernel(unsigned chunks, const DevModulus* mods, unsigned mod_start, unsigned nmod,
                                                                              unsigned n, const u64* a, unsigned pa, const u64* b, unsigned pb, u64* out) {
    const unsigned po = pa + pb - 1;
    const unsigned limb = blk_row(chunks) % nmod;
    const size_t item = blk_row(chunks) / nmod;
    const DevModulus md = mods[mod_start + limb];
    const size_t pc = (size_t)nmod * n;
    const u64* ap = a + item * pa * pc + (size_t)limb * n;
    const u64* bp = b + item * pb * pc + (size_t)limb * n;
    u64* op = out + item * po * pc + (size_t)limb * n;
    for (unsigned i = blk_col(chunks); i < n; i += chunks * blockDim.x) {
        for (unsigned o = 0; o < po; ++o) {
            const unsigned i_start = (o + 1 > pb) ? (o + 1 - pb) : 0;
            const unsigned i_end = (pa - 1 < o) ? pa - 1 : o;
            u64 acc = 0;
            for (unsigned p = i_start; p <= i_end; ++p)
                acc = add_mod(acc, mul_mod(ap[p * pc + i], bp[(o - p) * pc + i], md), md.q);
            op[o * pc + i] = acc;
        }
    }
}

// fgk/dyadic_convolute.cu:92-114 kernel_dyadic_square
__global__ __launch_bounds__(POLY_BLOCK) void dyadic_square_kernel(unsigned chunks, const DevModulus* mods, unsigned mod_start, unsigned nmod,
                                                                   unsigned n, const u64* a, u64* out) {
    const unsigned limb = blk_row(chunks) % nmod;
    const size_t item = blk_row(chunks) / nmod;
    const DevModulus md = mods[mod_start + limb];
    const size_t pc = (size_t)nmod * n;
    const u64* ap = a + item * 2 * pc + (size_t)limb * n;
    u64* op = out + item * 3 * pc + (size_t)limb * n;
    for (unsigned i = blk_col(chunks) * 2; i < n; i += chunks * blockDim.x * 2) {
        const u64x2 c0 = ld2(ap + i), c1 = ld2(ap + pc + i);
        u64 x0 = mul_mod(c0.a, c1.a, md), x1 = mul_mod(c0.b, c1.b, md);
        st2(op + i, mul_mod(c0.a, c0.a, md), mul_mod(c0.b, c0.b, md));
        st2(op + pc + i, add_mod(x0, x0, md.q), add_mod(x1, x1, md.q));
        st2(op + 2 * pc + i, mul_mod(c1.a, c1.a, md), mul_mod(c1.b, c1.b, md));
    }
}

// ---- key switching ---------------------------------------------------------------------

// KeyPtrs / KS_MAX_KEYS: ntt_kernels.hpp

// fgk/switch_key.cu:83-136 kernel_accumulate_products.
//   temp_ntt [batch][L+1][L][N]   decomposed digits in NTT form (row i under q_key(i))
//   keys[j]  -> [2][K][N]
//   poly_prod [batch][2][L+1][N]
// grid.y = batch*(L+1); a thread owns two coefficients of ONE row i and produces both key
// components from a single pass over its L digits; the <digit, key> sum is accumulated in
// 128 bits and reduced once (a sum of L <= 64 products of 61-bit residues is < 2^128, and the
// reference's per-term Barrett reduction yields the same canonical value).
// diag != nullptr: the digit of row i under its own modulus (j == i < L) is the untouched NTT-form input limb
// (the reference's host path does the same, evaluator_keyswitching_core.cu:851-852), read from diag[item][j].
__global__ __launch_bounds__(POLY_BLOCK) void ks_accumulate_kernel(unsigned chunks, const DevModulus* mods, unsigned K, unsigned L, unsigned n,
                                                                   const u64* temp_ntt, KeyPtrs keys, u64* poly_prod,
                                                                   const u64* diag, size_t diag_bstride) {
    const unsigned i = blk_row(chunks) % (L + 1);
    const size_t item = blk_row(chunks) / (L + 1);
    const unsigned key_index = (i == L) ? K - 1 : i;
    const DevModulus md = mods[key_index];
    const u64* tp = temp_ntt + (item * (L + 1) + i) * (size_t)L * n;
    const size_t key_poly = (size_t)K * n;
    u64* pp = poly_prod + item * 2 * (size_t)(L + 1) * n + (size_t)i * n;
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        u64 lo00 = 0, hi00 = 0, lo01 = 0, hi01 = 0, lo10 = 0, hi10 = 0, lo11 = 0, hi11 = 0;
        for (unsigned j = 0; j < L; ++j) {
            const u64x2 d = (diag && j == i) ? ld2(diag + item * diag_bstride + (size_t)j * n + x) : ld2(tp + (size_t)j * n + x);
            const u64* kj = keys.p[j] + (size_t)key_index * n + x;
            const u64x2 k0 = ld2(kj), k1 = ld2(kj + key_poly);
            mac128(lo00, hi00, d.a, k0.a); mac128(lo01, hi01, d.b, k0.b);
            mac128(lo10, hi10, d.a, k1.a); mac128(lo11, hi11, d.b, k1.b);
        }
        st2(pp + x, barrett128(lo00, hi00, md.q, md.ratio_lo, md.ratio_hi), barrett128(lo01, hi01, md.q, md.ratio_lo, md.ratio_hi));
        st2(pp + (size_t)(L + 1) * n + x, barrett128(lo10, hi10, md.q, md.ratio_lo, md.ratio_hi),
            barrett128(lo11, hi11, md.q, md.ratio_lo, md.ratio_hi));
    }
}

// evaluator_keyswitching_core.cu:570-598 device_ski_util6_merged.
//   last_intt [batch][2][N]       INTT of the special-prime row of poly_prod
//   temp_last [batch][2][L][N]
// grid.y = batch*2*L : thread -> two coefficients of (item, k, j)
__global__ __launch_bounds__(POLY_BLOCK) void ks_util6_kernel(unsigned chunks, const DevModulus* mods, unsigned K, unsigned L, unsigned n,
                                                              const u64* last_intt, size_t last_stride, u64* temp_last) {
    const unsigned j = blk_row(chunks) % L;
    const size_t kb = blk_row(chunks) / L;  // item*2 + k
    const DevModulus qk = mods[K - 1];
    const DevModulus qi = mods[j];
    const u64 qk_half = qk.q >> 1;
    const u64 fix = qi.q - barrett64(qk_half, qi.q, qi.ratio_hi);
    const bool need_reduce = qk.q > qi.q;
    const u64* src = last_intt + kb * last_stride;   // last_stride = N (compact) or (L+1)*N (row L of a full INTT)
    u64* dst = temp_last + (kb * L + j) * (size_t)n;
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        const u64x2 v = ld2(src + x);
        u64 t0 = barrett64(v.a + qk_half, qk.q, qk.ratio_hi), t1 = barrett64(v.b + qk_half, qk.q, qk.ratio_hi);
        if (need_reduce) { t0 = barrett64(t0, qi.q, qi.ratio_hi); t1 = barrett64(t1, qi.q, qi.ratio_hi); }
        st2(dst + x, t0 + fix, t1 + fix);
    }
}

// evaluator_keyswitching_core.cu:625-658 device_ski_util7_merged.
//   prod      [batch][2][prod_rows][N] (rows 0..L-1 used; NTT form: poly_prod, else its INTT)
//   temp_last [batch][2][L][N]
//   dest      [batch][2][L][N]
//   inv_qk    Shoup pairs (operand, quotient) of q_special^-1 mod q_j, j < L (RNSTool::inv_q_last_mod_q of the key level)
__global__ __launch_bounds__(POLY_BLOCK) void ks_util7_kernel(unsigned chunks, const DevModulus* mods, unsigned L, unsigned prod_rows, unsigned n,
                                                              const u64* prod, const u64* temp_last, const ulonglong2* inv_qk,
                                                              int is_ckks, int assign_method, u64* dest,
                                                              const u64* addend, size_t addend_bstride,
                                                              const u64* last_intt = nullptr, size_t last_stride = 0, unsigned K = 0) {
    const unsigned j = blk_row(chunks) % L;
    const size_t kb = blk_row(chunks) / L;   // item*2 + k
    const unsigned k = kb & 1;
    const DevModulus md = mods[j];
    const ulonglong2 f = inv_qk[j];
    // coefficient form: ski_util6's rounding fix is formed here from the special-prime row (last_intt) instead of being read back
    // from temp_last -- the same word sequence as ks_util6_kernel
    const DevModulus qk = mods[last_intt ? K - 1 : j];
    const u64 qk_half = qk.q >> 1;
    const u64 fix = md.q - barrett64(qk_half, md.q, md.ratio_hi);
    const bool need_reduce = qk.q > md.q;
    const u64* ls = last_intt ? last_intt + kb * last_stride : nullptr;
    const u64 lift = is_ckks ? (md.q << 2) : (md.q << 1);
    const bool add_inplace = (assign_method == 0) || (k == 0 && assign_method == 2);
    const u64* pp = prod + (kb * prod_rows + j) * (size_t)n;
    const u64* tl = temp_last + (kb * L + j) * (size_t)n;
    u64* dp = dest + (kb * L + j) * (size_t)n;
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        const u64x2 p = ld2(pp + x);
        u64x2 t;
        if (ls) {
            const u64x2 v = ld2(ls + x);
            u64 t0 = barrett64(v.a + qk_half, qk.q, qk.ratio_hi), t1 = barrett64(v.b + qk_half, qk.q, qk.ratio_hi);
            if (need_reduce) { t0 = barrett64(t0, md.q, md.ratio_hi); t1 = barrett64(t1, md.q, md.ratio_hi); }
            t.a = t0 + fix; t.b = t1 + fix;
        } else t = ld2(tl + x);
        u64 d0 = shoup_mul(p.a + lift - t.a, f.x, f.y, md.q);
        u64 d1 = shoup_mul(p.b + lift - t.b, f.x, f.y, md.q);
        if (add_inplace) {
            const u64x2 o = ld2(dp + x);
            d0 = add_mod(o.a, d0, md.q); d1 = add_mod(o.b, d1, md.q);
        }
        if (addend) {   // relinearize_internal's trailing add_inplace_ps (evaluator_keyswitching.cu:143), fused
            const u64x2 o = ld2(addend + (kb >> 1) * addend_bstride + ((size_t)k * L + j) * n + x);
            d0 = add_mod(d0, o.a, md.q); d1 = add_mod(d1, o.b, md.q);
        }
        st2(dp + x, d0, d1);
    }
}

// ---- modulus switching -------------------------------------------------------------------

// utils/rns_tool.cu:374-402 device_divide_and_round_q_last (BFV, coefficient form).
//   in [items][L][N] -> out [items][L-1][N]; grid.y = items*(L-1)
//   inv_last: Shoup pairs of q_{L-1}^-1 mod q_i for this level
__global__ __launch_bounds__(POLY_BLOCK) void divide_round_q_last_kernel(unsigned chunks, const DevModulus* mods, unsigned L, unsigned n,
                                                                         const u64* in, const ulonglong2* inv_last, u64* out) {
    const unsigned i = blk_row(chunks) % (L - 1);
    const size_t item = blk_row(chunks) / (L - 1);
    const DevModulus md = mods[i];
    const DevModulus ql = mods[L - 1];
    const ulonglong2 f = inv_last[i];
    const u64 half = ql.q >> 1;
    const u64 half_mod = barrett64(half, md.q, md.ratio_hi);
    const u64* last = in + (item * L + (L - 1)) * (size_t)n;
    const u64* src = in + (item * L + i) * (size_t)n;
    u64* dst = out + (item * (L - 1) + i) * (size_t)n;
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        const u64x2 vl = ld2(last + x), vi = ld2(src + x);
        u64 t0 = barrett64(add_mod(vl.a, half, ql.q), md.q, md.ratio_hi);
        u64 t1 = barrett64(add_mod(vl.b, half, ql.q), md.q, md.ratio_hi);
        t0 = sub_mod(t0, half_mod, md.q); t1 = sub_mod(t1, half_mod, md.q);
        st2(dst + x, shoup_mul(sub_mod(vi.a, t0, md.q), f.x, f.y, md.q), shoup_mul(sub_mod(vi.b, t1, md.q), f.x, f.y, md.q));
    }
}

// utils/rns_tool.cu:523-550 device_divide_and_round_q_last_ntt_step1.
//   last_intt [items][N] (INTT of the last limb) -> temp [items][L-1][N]; grid.y = items*(L-1)
__global__ __launch_bounds__(POLY_BLOCK) void rescale_step1_kernel(unsigned chunks, const DevModulus* mods, unsigned L, unsigned n,
                                                                   const u64* last_intt, u64* temp) {
    const unsigned i = blk_row(chunks) % (L - 1);
    const size_t item = blk_row(chunks) / (L - 1);
    const DevModulus md = mods[i];
    const DevModulus ql = mods[L - 1];
    const u64 half = ql.q >> 1;
    const u64 half_mod = barrett64(half, md.q, md.ratio_hi);
    const bool need_reduce = md.q < ql.q;
    const u64* src = last_intt + item * (size_t)n;
    u64* dst = temp + (item * (L - 1) + i) * (size_t)n;
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        const u64x2 v = ld2(src + x);
        u64 t0 = add_mod(v.a, half, ql.q), t1 = add_mod(v.b, half, ql.q);
        if (need_reduce) { t0 = barrett64(t0, md.q, md.ratio_hi); t1 = barrett64(t1, md.q, md.ratio_hi); }
        st2(dst + x, sub_mod(t0, half_mod, md.q), sub_mod(t1, half_mod, md.q));
    }
}

// utils/rns_tool.cu:607-627 device_divide_and_round_q_last_ntt_step2.
//   in [items][L][N], temp [items][L-1][N] (NTT form) -> out [items][L-1][N]
__global__ __launch_bounds__(POLY_BLOCK) void rescale_step2_kernel(unsigned chunks, const DevModulus* mods, unsigned L, unsigned n,
                                                                   const u64* in, const u64* temp, const ulonglong2* inv_last, u64* out) {
    const unsigned i = blk_row(chunks) % (L - 1);
    const size_t item = blk_row(chunks) / (L - 1);
    const DevModulus md = mods[i];
    const ulonglong2 f = inv_last[i];
    const u64 lift = md.q << 2;
    const u64* src = in + (item * L + i) * (size_t)n;
    const u64* tp = temp + (item * (L - 1) + i) * (size_t)n;
    u64* dst = out + (item * (L - 1) + i) * (size_t)n;
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        const u64x2 v = ld2(src + x), t = ld2(tp + x);
        // add_uint64_mod(x, 4q) = x + 3q ; sub_uint64_mod(., t) never borrows ; Shoup multiply canonicalises
        u64 d0 = add_mod(v.a, lift, md.q), d1 = add_mod(v.b, lift, md.q);
        d0 = sub_mod(d0, t.a, md.q); d1 = sub_mod(d1, t.b, md.q);
        st2(dst + x, shoup_mul(d0, f.x, f.y, md.q), shoup_mul(d1, f.x, f.y, md.q));
    }
}

// strided limb copy: evaluator_modswitch.cu:147-171 kernel_mod_switch_drop_to, and the gathers
// the fused pipelines need ([items][L_in][N] -> [items][L_out][N], first L_out limbs, or one limb).
__global__ __launch_bounds__(POLY_BLOCK) void copy_limbs_kernel(unsigned chunks, unsigned n, const u64* in, size_t in_item_stride, unsigned in_first,
                                                                u64* out, size_t out_item_stride, unsigned nlimbs) {
    const unsigned l = blk_row(chunks) % nlimbs;
    const size_t item = blk_row(chunks) / nlimbs;
    const u64* src = in + item * in_item_stride + (size_t)(in_first + l) * n;
    u64* dst = out + item * out_item_stride + (size_t)l * n;
    for (unsigned x = blk_col(chunks) * 2; x < n; x += chunks * blockDim.x * 2) {
        const u64x2 v = ld2(src + x);
        st2(dst + x, v.a, v.b);
    }
}

}  // namespace troyn
