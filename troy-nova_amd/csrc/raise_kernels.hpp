// raise_kernels.hpp -- CKKS ModRaise (troyn_ckks_mod_raise): the exact centred base extension of a ciphertext from the primes q_0 .. q_{L-1}
// to q_0 .. q_{LO-1}.  An addition to the reference's kernels; integer arithmetic only.
//
// Per coefficient (coefficient form): x = the centred representative in (-Q/2, Q/2] of the L input residues, Q = q_0 ... q_{L-1}; row j of
// the result is x mod q_j in [0, q_j).  No multi-word arithmetic:
//   digits   the mixed-radix digits d_0 .. d_{L-1} of X = x mod Q (ckks_mixed_radix_digit, shared with ckks_compose_kernel);
//   centring mixed radix is positional, so X > floor(Q/2) is the lexicographic comparison of d, top digit first, with the mixed-radix digits of
//            floor(Q/2) (half_digits, built on the host);
//   rows     for every new prime q_j a Horner over the digits modulo q_j, r = (r (q_i mod q_j) + d_i) mod q_j from the top digit down, minus
//            Q mod q_j where X was above the half.
// The digits of a coefficient are computed once and every new row is written from registers.
//
// Geometry of scalar_weighted_sums_kernel: 256 threads, a thread owns two adjacent coefficients of one (item, polynomial) and moves them with
// 16-byte loads and stores; a workgroup strides over the row, so a row shorter than 512 coefficients is a partial workgroup.  No LDS.
// LM: the digits held in registers (L <= LM; every digit loop is unrolled, nothing is indexed at run time).  The loop over the new rows is a
// run-time loop: its constants (the modulus, q_i mod q_j, Q mod q_j) depend on j only, so they are wave-uniform scalar loads.
// Traffic per coefficient: 8 L bytes read, 8 (LO - L) written (+ 8 L where the kernel also writes the low rows).
#pragma once
#include "ckks_kernels.hpp"

namespace troyn {

constexpr int RAISE_BLOCK = 256;

struct ModRaiseArgs {
    const u64* in;                        // [items][L][N], coefficient form
    u64* low;                             // null, or [items][..][N] with item stride low_stride: rows 0 .. L-1 are copied there as read
    u64* out;                             // row L of item 0; item stride out_stride, rows L .. LO-1 consecutive
    size_t low_stride, out_stride;        // in words
    const DevModulus* mods;
    const ulonglong2* garner;             // [K][K]: (operand, quotient) of q_j^-1 mod q_i at [i][j], j < i
    const ulonglong2* radix;              // [K][CKKS_MAX_L]: (operand, quotient) of q_i mod q_j at [j][i]
    const u64* half_digits;               // [CKKS_MAX_L]: mixed-radix digits of floor(Q / 2)
    const u64* q_mod;                     // [K]: Q mod q_j
    unsigned K, L, LO, n;
};

// (the pointers travel as separate __restrict__ parameters: the stores then cannot alias the tables, which stay scalar loads inside the row loop)
template <int LM>
__global__ __launch_bounds__(RAISE_BLOCK) void ckks_mod_raise_kernel(unsigned chunks, const u64* __restrict__ in, u64* __restrict__ low, size_t low_stride,
                                                                    u64* __restrict__ out, size_t out_stride, const DevModulus* __restrict__ mods,
                                                                    const ulonglong2* __restrict__ garner, const ulonglong2* __restrict__ radix,
                                                                    const u64* __restrict__ half_digits, const u64* __restrict__ q_mod, unsigned K, unsigned L,
                                                                    unsigned LO, unsigned n) {
    const size_t item = blockIdx.x / chunks;
    const u64* src = in + item * L * n;
    auto ld2 = [](const u64* p) { return *reinterpret_cast<const ulonglong2*>(p); };
    auto st2 = [](u64* p, u64 a, u64 b) { *reinterpret_cast<ulonglong2*>(p) = make_ulonglong2(a, b); };
    for (unsigned x = ((blockIdx.x % chunks) * RAISE_BLOCK + threadIdx.x) * 2; x < n; x += chunks * RAISE_BLOCK * 2) {
        ulonglong2 v[LM];
#pragma unroll
        for (int i = 0; i < LM; i++)
            if ((unsigned)i < L) v[i] = ld2(src + (size_t)i * n + x);
        if (low) {
            u64* dst = low + item * low_stride + x;
#pragma unroll
            for (int i = 0; i < LM; i++)
                if ((unsigned)i < L) st2(dst + (size_t)i * n, v[i].x, v[i].y);
        }
        u64 da[LM], db[LM];
        ckks_static_for<0, LM>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            da[i] = db[i] = 0;
            if ((unsigned)i < L) {
                const DevModulus& m = mods[i];
                const ulonglong2* g = garner + (size_t)i * K;
                da[i] = ckks_mixed_radix_digit<LM>(i, v[i].x, da, m, g);
                db[i] = ckks_mixed_radix_digit<LM>(i, v[i].y, db, m, g);
            }
        });
        // X > floor(Q/2): decided at the highest digit that differs
        bool ga = false, gb = false, ea = true, eb = true;
#pragma unroll
        for (int i = LM - 1; i >= 0; i--) {
            if ((unsigned)i < L) {
                const u64 h = half_digits[i];
                if (ea && da[i] != h) { ga = da[i] > h; ea = false; }
                if (eb && db[i] != h) { gb = db[i] > h; eb = false; }
            }
        }
        u64* dst = out + item * out_stride + x;
        for (unsigned j = L; j < LO; j++, dst += n) {
            const u64 q = mods[j].q, ratio = mods[j].ratio_hi;
            const ulonglong2* w = radix + (size_t)j * CKKS_MAX_L;
            u64 ra = 0, rb = 0;
#pragma unroll
            for (int i = LM - 1; i >= 0; i--) {
                if ((unsigned)i < L) {
                    const u64 ta = barrett64(da[i], q, ratio), tb = barrett64(db[i], q, ratio);
                    if (i == LM - 1) { ra = ta; rb = tb; }          // nothing above the top digit of the instantiation
                    else {
                        const ulonglong2 wi = w[i];
                        ra = add_mod(shoup_mul(ra, wi.x, wi.y, q), ta, q);
                        rb = add_mod(shoup_mul(rb, wi.x, wi.y, q), tb, q);
                    }
                }
            }
            const u64 qm = q_mod[j];
            if (ga) ra = sub_mod(ra, qm, q);
            if (gb) rb = sub_mod(rb, qm, q);
            st2(dst, ra, rb);
        }
    }
}

}  // namespace troyn
