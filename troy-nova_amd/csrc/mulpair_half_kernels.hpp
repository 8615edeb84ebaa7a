// mulpair_half_kernels.hpp -- step (1) of the fused multiply -> relinearize -> rescale chain, digits = INTT(a1 (.) b1), at N = 16384 on
// half-limb tiles in ksmac2's shape (ksmac_kernels.hpp): 256 threads x 32 coefficients, 68 KB of LDS, two free-running workgroups per CU.
//
// Why: the whole-limb form (ntt_pass_kernel<ArithF64, 14, ..., NTT_FUSED_MULPAIR>) runs ONE 1024-thread workgroup per CU on a 132 KB tile, so its
// load, transform and store phases run back to back on a CU with nothing else resident to issue while its loads are in flight.
//
// The first 13 Gentleman-Sande layers of a 2^14-point inverse transform act inside the two contiguous NTT-form halves [0, 8192) and
// [8192, 16384); the last layer pairs word i of one half with word i of the other under ONE twiddle -- the mirror image of the layer 0 ksmac2
// applies while loading.  One workgroup owns one limb-polynomial of one item:
//   half 0:  coalesced 16-byte loads of a1, b1 in a rolling window, product in the loaded layout, transposed through the wave's own slice;
//            round A (tile bits 0..4, lane-interleaved twiddle vectors) -> wave-private exchange -> round B (bits 5..9, a 256-byte vector per
//            wave-half) -> the one workgroup-barrier exchange -> round C (bits 10..12, workgroup-uniform scalar twiddles).
//            This is ksmac2's round 2 / 1 / 0 walked backwards; the result sits in ksmac2's LOAD layout (register b0 | b9<<1 | R3<<2 of tile word
//            b0 | t<<1 | b9<<9 | R3<<10) and stays in 32 registers.
//   half 1:  the same; its first operand loads are requested before half 0's round C (no store has been issued yet: vmcnt counts loads only).
//   last layer in registers (N^-1 folded in as ArithF64::inv_fold does), canonical digits (ArithF64::digit_word), 16-byte coalesced stores.
//
// Magnitudes (dev_math_f64.hpp: a difference output is f64_mulq(u - v, w), |.| <= (0.5 + 1.5 |u - v| 2^-52) p = (0.5 + 0.375 m) p for
// |u - v| = m 2^50; a sum output doubles).  Every block re-centres the SUM outputs of its 2nd and of its 4th layer (f64_corr: -> 0.5 p + 1); in
// multiples of p, for p < 2^50, worst case over the registers:
//   round A  start 0.875 (product of canonical factors, ArithF64::prod_in)
//            L1 1.75 | L2 sums 3.5 -> 0.5, diffs 1.8125 | L3 3.625 | L4 sums 7.25 -> 0.5, diffs 3.21875 | L5 6.4375      (peak 7.25 p < 2^53)
//            exchange: every word re-centred -> 0.5 p + 1
//   round B  L1 1.0 | L2 sums 2.0 -> 0.5, diffs 1.25 | L3 2.5 | L4 sums 5.0 -> 0.5, diffs 2.375 | L5 4.75                  (peak 5 p)
//            exchange: every word re-centred -> 0.5 p + 1
//   round C + last layer (a 3 + 1 block): L1 1.0 | L2 sums 2.0 -> 0.5, diffs 1.25 | L3 2.5 (held) | last layer: u + v and u - v <= 5.0,
//            f64_mulc(u + v, N^-1) and f64_mulq(u - v, w N^-1) <= (0.5 + 0.375 x 5) p = 2.375 p, re-centred by digit_word.
// Every operand of every operation is an exact integer below 2^53 (the 7.25 p of round A is the peak the whole-limb LEAN form reaches too);
// tools/fp64_half_check.cpp replays the sequences against 128-bit integers, tests/test_fp64_bounds_half.py drives it.  All arithmetic is exact
// modulo p, so the canonical digits are the words the whole-limb kernel stores.
#pragma once
#include "ksmac_kernels.hpp"

#ifndef MPH_LOAD_WINDOW
#define MPH_LOAD_WINDOW 8      // register pairs (two 16-byte loads each) in flight per thread
#endif

namespace troyn {

struct MulpairHalfArgs {
    const u64* a1; const u64* b1;     // polynomial 1 of the two input ciphertexts, limb 0: [item][limb][N] words, NTT form
    long long in_bstride;             // words between items (limbs are N apart)
    u64* out; long long out_bstride;  // digits [item][limb][N]: canonical, doubles (store_f64) or words
    const DevModulus* mods;           // limb j uses modulus j
    const double* tw;                 // [K][N] inverse twiddles, reference table order
    const double* tw_r1;              // [K][N/1024][32] round-B vector per value of the index bits above bit 9 (slot (1 << lvl) + g)
    const double* tw_r2;              // [K][N] round-A vectors, lane-interleaved (ksm_perm)
    unsigned L;                       // limbs per item
    unsigned store_f64;               // NTT_FLAG_STORE_F64
};

// Gentleman-Sande butterflies of register bit RB for the twiddle groups [G0, G0 + NG): tw[i] belongs to group G0 + i.  FIX: the sums are re-centred.
template <int RB, int G0, int NG, bool FIX>
__device__ __forceinline__ void mph_layer(double (&x)[32], const double* tw, const F64Mod& fm) {
    static_for<0, NG>([&](auto gc) {
        constexpr int g = G0 + decltype(gc)::value;
        const double w = tw[decltype(gc)::value];
        static_for<0, (1 << RB)>([&](auto oc) {
            constexpr int R0 = (g << (RB + 1)) | decltype(oc)::value, R1 = R0 | (1 << RB);
            const double u = x[R0], v = x[R1];
            x[R0] = FIX ? f64_corr(u + v, fm) : u + v;
            x[R1] = f64_mulq(u - v, w, fm.inv_p, fm.p);
        });
    });
}

// A 5-layer inverse register round (register bit 0 first) whose 31 twiddles sit in a 32-slot vector (slot (1 << lvl) + g, lvl = 4 - register
// bit; slot 0 unused).  ta / tb: slots 16..23 / 24..31, already requested by the caller; ld(q) returns slots 2q, 2q+1.
template <class LD>
__device__ __forceinline__ void mph_round5(double (&x)[32], double (&ta)[8], double (&tb)[8], LD&& ld, const F64Mod& fm) {
    mph_layer<0, 0, 8, false>(x, ta, fm);
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, 4>([&](auto qc) { const double2 v = ld(4 + decltype(qc)::value); ta[2 * decltype(qc)::value] = v.x; ta[2 * decltype(qc)::value + 1] = v.y; });
    mph_layer<0, 8, 8, false>(x, tb, fm);
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, 4>([&](auto qc) { const double2 v = ld(decltype(qc)::value); tb[2 * decltype(qc)::value] = v.x; tb[2 * decltype(qc)::value + 1] = v.y; });
    mph_layer<1, 0, 8, true>(x, ta, fm);
    __builtin_amdgcn_sched_barrier(0);
    mph_layer<2, 0, 4, false>(x, tb + 4, fm);
    mph_layer<3, 0, 2, true>(x, tb + 2, fm);
    mph_layer<4, 0, 1, false>(x, tb + 1, fm);
    __builtin_amdgcn_sched_barrier(0);
}

// grid = batch * L, workgroup g = (item g / L, limb g % L).  W: register pairs of the rolling load window
template <int W>
__global__ __launch_bounds__(KSM_THREADS, 2) void mulpair_half_kernel(MulpairHalfArgs a) {
    constexpr unsigned N = 1u << 14, HW = 1u << KSM_TB;      // words of a half
    static_assert(W >= 1 && W <= 16, "load window: 1..16 register pairs");
    __shared__ __attribute__((aligned(16))) u64 lds[KSM_LDS_WORDS];

    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned j = blockIdx.x % a.L, b = blockIdx.x / a.L;
    const ArithF64::Mod md = ArithF64::make(a.mods[j]);
    const F64Mod fm = md.m;

    typedef const double __attribute__((address_space(4)))* cdp;
    const cdp tws = (cdp)(unsigned long long)(a.tw + (size_t)j * N);       // scalar (workgroup-uniform) twiddle fetches
    const double* r1b = a.tw_r1 + (size_t)j * (N >> 10) * 32;
    const double* r2b = a.tw_r2 + (size_t)j * N;
    const unsigned r1off = (t >> 5) * 256u, slice_off = wave * 16384u + lane * 16u;     // bytes

    // LDS addresses (padded words), ksmac2's: p2 holds tile bits [0,5) per thread, p1 bits [5,10), p0 the load layout, pt the coalesced pairs
    const unsigned p0 = ksm_phys(t << 1);                                      // + ksm_phys(b9<<9 | R3<<10)
    const unsigned p1 = ksm_phys((t & 31u) | ((t >> 5) << 10));                // + 34 * R
    const unsigned p2 = ksm_phys(t << 5);                                      // + R
    const unsigned pt = ksm_phys(wave * 2048u + lane * 2u);                    // + ksm_phys(128 m)

    const u64* ga = a.a1 + (long long)b * a.in_bstride + (size_t)j * N;
    const u64* gb = a.b1 + (long long)b * a.in_bstride + (size_t)j * N;

    ulonglong2 va[16], vb[16];
    auto request = [&](auto hc, auto ic) {
        constexpr int h = decltype(hc)::value, m = decltype(ic)::value;
        va[m] = ksm_gload<ulonglong2>(ksm_uniform(ga + h * HW) + m * 128, slice_off);
        vb[m] = ksm_gload<ulonglong2>(ksm_uniform(gb + h * HW) + m * 128, slice_off);
    };

    // loads (pairs [W, 16) requested as the window moves; [0, W) by the caller), product, rounds A and B, and the exchange in front of round C
    auto front = [&](auto hc, double (&x)[32]) {
        constexpr int h = decltype(hc)::value;
        const double* r1u = ksm_uniform(r1b + h * ((KSM_THREADS >> 5) * 32));
        const double* r2u = ksm_uniform(r2b + h * HW);
        double ta[8], tb[8];
        // round A's first 16 twiddle slots travel behind the operands
        static_for<0, 4>([&](auto qc) { constexpr int q = decltype(qc)::value; const double2 v = ksm_gload<double2>(r2u + 128 * (8 + q), slice_off); ta[2 * q] = v.x; ta[2 * q + 1] = v.y; });
        static_for<0, 4>([&](auto qc) { constexpr int q = decltype(qc)::value; const double2 v = ksm_gload<double2>(r2u + 128 * (12 + q), slice_off); tb[2 * q] = v.x; tb[2 * q + 1] = v.y; });
        static_for<0, 16>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            __builtin_amdgcn_sched_barrier(0);
            // canonical factors below p: |product| <= 0.875 p, the start of round A's bound
            const double2 pr = make_double2(f64_mulq(f64_from_u64(va[m].x), f64_from_u64(vb[m].x), fm.inv_p, fm.p),
                                            f64_mulq(f64_from_u64(va[m].y), f64_from_u64(vb[m].y), fm.inv_p, fm.p));
            *reinterpret_cast<double2*>(&lds[pt + ksm_phys(m * 128u)]) = pr;
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (m + W < 16) request(hc, std::integral_constant<int, m + W>{});
        });
        // the wave reads back the words it wrote itself (LDS executes a wave's accesses in order): no workgroup barrier
        __builtin_amdgcn_wave_barrier();
        static_for<0, 16>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            const double2 v = *reinterpret_cast<const double2*>(&lds[p2 + 2 * m]);
            x[2 * m] = v.x; x[2 * m + 1] = v.y;
        });
        __builtin_amdgcn_sched_barrier(0);
        // ---- round A: tile bits 0..4 = register bits 0..4, lane-interleaved twiddle vectors ------------------------------------------
        mph_round5(x, ta, tb, [&](int q) { return ksm_gload<double2>(r2u + 128 * q, slice_off); }, fm);
        // ---- exchange A -> B: inside groups of 32 consecutive threads (tile bits [10,13) = t >> 5 on both sides), wave-private ---------
        static_for<0, 16>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            *reinterpret_cast<double2*>(&lds[p2 + 2 * m]) = make_double2(f64_corr(x[2 * m], fm), f64_corr(x[2 * m + 1], fm));
        });
        static_for<0, 4>([&](auto qc) { constexpr int q = decltype(qc)::value; const double2 v = ksm_gload<double2>(r1u + 2 * (8 + q), r1off); ta[2 * q] = v.x; ta[2 * q + 1] = v.y; });
        static_for<0, 4>([&](auto qc) { constexpr int q = decltype(qc)::value; const double2 v = ksm_gload<double2>(r1u + 2 * (12 + q), r1off); tb[2 * q] = v.x; tb[2 * q + 1] = v.y; });
        __builtin_amdgcn_wave_barrier();
        static_for<0, 32>([&](auto rc) {
            constexpr int R = decltype(rc)::value;
            x[R] = f64_bits_to_double(lds[p1 + 34 * R]);
        });
        __builtin_amdgcn_sched_barrier(0);
        // ---- round B: tile bits 5..9 = register bits 0..4, one 256-byte twiddle vector per wave-half ---------------------------------
        mph_round5(x, ta, tb, [&](int q) { return ksm_gload<double2>(r1u + 2 * q, r1off); }, fm);
        // ---- exchange B -> C: the one workgroup barrier of the transform ---------------------------------------------------------------
        static_for<0, 32>([&](auto rc) {
            constexpr int R = decltype(rc)::value;
            lds[p1 + 34 * R] = f64_double_to_bits(f64_corr(x[R], fm));
        });
        __syncthreads();
        static_for<0, 16>([&](auto ic) {
            constexpr int i = decltype(ic)::value;      // i = b9 | R3<<1
            constexpr unsigned off = ksm_phys(((i & 1) << 9) | ((i >> 1) << 10));
            const double2 v = *reinterpret_cast<const double2*>(&lds[p0 + off]);
            x[2 * i] = v.x; x[2 * i + 1] = v.y;
        });
        __builtin_amdgcn_sched_barrier(0);
    };
    // ---- round C: tile bits 10, 11, 12 = register bits 2, 3, 4; twiddles are workgroup-uniform ------------------------------------------
    auto round_c = [&](auto hc, double (&x)[32]) {
        constexpr unsigned h = decltype(hc)::value;
        static_for<0, 3>([&](auto lc) {
            constexpr int li = decltype(lc)::value;
            constexpr int bit = 10 + li, rb = bit - 8, l = 13 - bit;     // l: the forward-numbered layer of this bit
            constexpr int NG = 1 << (12 - bit);
            double w[NG];
            static_for<0, NG>([&](auto gc) { constexpr unsigned g = decltype(gc)::value; w[g] = tws[N - (2u << l) + 1u + (h << (12 - bit)) + g]; });
            mph_layer<rb, 0, NG, li == 1>(x, w, fm);
        });
        __builtin_amdgcn_sched_barrier(0);
    };

    double x0[32], x1[32];
    const std::integral_constant<int, 0> H0{};
    const std::integral_constant<int, 1> H1{};
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, W>([&](auto ic) { request(H0, ic); });
    front(H0, x0);
    // half 1's operands travel under half 0's last round
    static_for<0, W>([&](auto ic) { request(H1, ic); });
    __builtin_amdgcn_sched_barrier(0);
    round_c(H0, x0);
    __syncthreads();       // half 1's first LDS writes land on words other waves read in half 0's last exchange
    front(H1, x1);
    round_c(H1, x1);

    // ---- last layer (tile word i of half 0 with word i of half 1, N^-1 folded in) + canonical digits, 16-byte coalesced stores ---------------
    const bool digits_f64 = a.store_f64 != 0;
    const double dg_add = digits_f64 ? 0.0 : F64_TWO52;
    const unsigned dg_mask_hi = digits_f64 ? 0xffffffffu : 0x000fffffu;
    u64* go = ksm_uniform(a.out + (long long)b * a.out_bstride + (size_t)j * N);
    static_for<0, 16>([&](auto ic) {
        constexpr int i = decltype(ic)::value;      // i = b9 | R3<<1
        constexpr unsigned woff = ((i & 1) << 9) + ((i >> 1) << 10);
        double s0 = x0[2 * i], d0 = x1[2 * i], s1 = x0[2 * i + 1], d1 = x1[2 * i + 1];
        ArithF64::inv_fold(s0, d0, md);
        ArithF64::inv_fold(s1, d1, md);
        nt_store2_at(go + woff, t << 4, ArithF64::digit_word(s0, false, dg_add, dg_mask_hi, md), ArithF64::digit_word(s1, false, dg_add, dg_mask_hi, md));
        nt_store2_at(go + HW + woff, t << 4, ArithF64::digit_word(d0, true, dg_add, dg_mask_hi, md), ArithF64::digit_word(d1, true, dg_add, dg_mask_hi, md));
    });
}

}  // namespace troyn
