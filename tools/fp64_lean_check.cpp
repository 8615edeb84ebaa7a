// Host-side exactness check of the lean FP64 transform body (csrc/ntt_kernels.hpp, ArithF64: centred / held_c / held_last / held_tail_in,
// to_lds_raw in front of the first inverse round of a1 (.) b1 and in front of TAIL_RESCALE's epilogue, digit_word; N = 16384 only).  A host build of the REAL
// csrc/dev_math_f64.hpp (f64_corr, f64_mulq, f64_mulc, f64_from_u64, f64_to_u64); the sequences below are the ones ArithF64 applies, in its order.
// Every result is compared with 128-bit integer arithmetic / the CPU oracle's transforms, every intermediate is checked against 2^53, and the
// maxima reached are printed.  Exit status 0 only if everything is exact and in range.
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -mfma -I troy-nova_amd/csrc tools/fp64_lean_check.cpp oracle/troy_oracle.o -o fp64_lean_check
//   (add -fsanitize=address,undefined for the sanitizer build; host code only, no GPU)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dev_math_f64.hpp"
extern "C" {
#include "../oracle/troy_oracle.h"
}

using namespace troyn;
typedef unsigned __int128 u128_;
typedef __int128 i128_;

static const double TWO53 = 9007199254740992.0;
static int g_bad = 0;
static double g_max = 0.0;       // largest |value| / 2^53 seen anywhere
static void seen(double v, const char* where) {
    const double a = std::fabs(v);
    if (a / TWO53 > g_max) g_max = a / TWO53;
    if (!(a < TWO53)) { if (g_bad < 20) printf("RANGE: %s reaches %.4f x 2^53\n", where, a / TWO53); g_bad++; }
}
static void fail(const char* what, u64 p, double got, double want) {
    if (g_bad < 20) printf("MISMATCH: %s p=%llu got %.1f want %.1f\n", what, p, got, want);
    g_bad++;
}
static u64 mulmod(u64 a, u64 b, u64 p) { return (u64)((u128_)a * b % p); }
static u64 canon_i(i128_ v, u64 p) { i128_ r = v % (i128_)p; if (r < 0) r += p; return (u64)r; }
static u64 canon_d(double v, u64 p) { return canon_i((i128_)v, p); }      // |v| < 2^53: exact
static u64 powmod(u64 a, u64 e, u64 p) { u64 r = 1; while (e) { if (e & 1) r = mulmod(r, a, p); a = mulmod(a, a, p); e >>= 1; } return r; }
static u64 invmod(u64 a, u64 p) { return powmod(a % p, p - 2, p); }

struct Md { F64Mod m; u64 q; };
static Md make(u64 q) { return Md{F64Mod{(double)q, 1.0 / (double)q}, q}; }

// ---- ArithF64's sequences (ntt_kernels.hpp) ----
static double centred(double x, const Md& m) {
    const double c = f64_corr(x, m.m);
    const double step = std::fabs(c) > 0.5 * (m.m.p - 1.0) ? std::copysign(m.m.p, c) : 0.0;
    return c - step;
}
static double scale_by(double x, double w, const Md& m) { return f64_mulq(x, w, m.m.inv_p, m.m.p); }
static double held_last(double ys, double cs, double inv_kl, const Md& ml) { return centred(ys - scale_by(cs, inv_kl, ml), ml); }
static double held_tail_in(double cs, double cl, double inv_kj, const Md& mj) { return scale_by(cs, inv_kj, mj) + cl; }
static u64 canon_small(double x, const Md& m) { return f64_to_u64(x < 0.0 ? x + m.m.p : x); }
static u64 tail_out(u64 prod_word, double y, double inv_lj, const Md& m) {
    return canon_small(scale_by(f64_corr(f64_from_u64(prod_word) - y, m.m), inv_lj, m), m);
}
static double prod_in(u64 x, u64 y, const Md& m) { return f64_mulq(f64_from_u64(x), f64_from_u64(y), m.m.inv_p, m.m.p); }
static u64 digit_word(double x, double add, unsigned mask_hi, const Md& m) {
    double c = f64_corr(x, m.m);
    c = c < 0.0 ? c + m.m.p : c;
    return f64_double_to_bits(c + add) & (((u64)mask_hi << 32) | 0xffffffffull);
}

static std::vector<u64> corner_words(u64 p) {
    std::vector<u64> v = {0, 1, 2, p - 1, p - 2, p / 2, p / 2 + 1, p / 2 - 1, p / 3, p - p / 3};
    u64 s = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < 40; i++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v.push_back(s % p); }
    return v;
}

// (a) the hand-over: c(s), c(l) and the first forward round's input against the reference's rounding fixes
//     r_j(s) = ((s + qk/2) mod qk) - (qk/2 mod qj), f_j(l) = ((l + ql/2) mod ql) - (ql/2 mod qj)   (ski_util6 / divide_and_round_q_last step 1)
static void check_handover(u64 qk, u64 ql, u64 qj) {
    const Md mk = make(qk), ml = make(ql), mj = make(qj);
    const u64 hk = qk >> 1, hl = ql >> 1;
    const double inv_kl = (double)invmod(qk, ql), inv_kj = (double)invmod(qk, qj);
    double max_in = 0.0;
    for (u64 s : corner_words(qk)) {
        // the last inverse round leaves any representative of s with |x| <= 2 qk
        for (int rep = -2; rep <= 1; rep++) {
            const double xs = (double)s + (double)rep * (double)qk;
            const double cs = centred(xs, mk);
            const double want = s <= hk ? (double)s : (double)s - (double)qk;
            if (cs != want) fail("c(s)", qk, cs, want);
            for (u64 y : corner_words(ql)) {
                const double ys = (double)y - ((y & 1) ? (double)ql : 0.0);       // any representative of |ys| <= 1.25 ql
                const double cl = held_last(ys, cs, inv_kl, ml);
                seen(ys - scale_by(cs, inv_kl, ml), "ys - c(s) qk^-1");
                // l = ys - r(s) qk^-1 mod ql, r(s) = c(s) mod ql
                const u64 rs_l = canon_i((i128_)cs, ql);
                const u64 l = canon_i((i128_)canon_d(ys, ql) - (i128_)mulmod(rs_l, invmod(qk, ql), ql), ql);
                const double want_l = l <= hl ? (double)l : (double)l - (double)ql;
                if (cl != want_l) fail("c(l)", ql, cl, want_l);
                const double x0 = held_tail_in(cs, cl, inv_kj, mj);
                seen(x0, "held_tail_in");
                if (std::fabs(x0) > max_in) max_in = std::fabs(x0);
                if (std::fabs(x0) > 0.6875 * (double)qj + 0x1p49) fail("|held_tail_in| bound", qj, x0, 0.6875 * (double)qj + 0x1p49);
                // reference: T forms
                const u64 Ts = (s + hk) % qk, Tl = (l + hl) % ql;
                const u64 rj = canon_i((i128_)(Ts % qj) - (i128_)(hk % qj), qj), fj = canon_i((i128_)(Tl % qj) - (i128_)(hl % qj), qj);
                const u64 ref = (u64)(((u128_)mulmod(rj, invmod(qk, qj), qj) + fj) % qj);
                if (canon_d(x0, qj) != ref) fail("r_j(s) qk^-1 + f_j(l)", qj, (double)canon_d(x0, qj), (double)ref);
            }
        }
    }
    printf("hand-over qk=%llu ql=%llu qj=%llu: max |held_tail_in| = %.4f x 2^50\n", qk, ql, qj, max_in / 0x1p50);
}

// worst-case growth, with the +1 of the quotient's rounding: |x'| <= |x| + (0.5 + 1.5 |x| 2^-52) p + 1
static double grow_fwd(double a, double p, int layers) { for (int i = 0; i < layers; i++) a += (0.5 + 1.5 * a * 0x1p-52) * p + 1.0; return a; }
static void check_bounds(u64 q) {
    const double p = (double)q;
    // first forward block of the merged tail: 4 layers from |x| <= 0.6875 p + 2^49
    const double f = grow_fwd(0.6875 * p + 1.0 + 0x1p49, p, 4);
    seen(f, "forward block from held_tail_in (worst case)");
    // a forward block from a re-centred word, and Q - y in front of tail_out
    const double y = grow_fwd(0.5 * p + 1.0, p, 4);
    seen(y + p, "Q - y in front of tail_out (worst case, 4-layer last round)");
    // first inverse block of a1 (.) b1 from |x| <= 0.875 p: sums double per layer and are re-centred after 2; a difference output is
    // 0.5 p + 1.5 |u - v| p 2^-52 + 1
    auto diff = [&](double d) { return (0.5 + 1.5 * d * 0x1p-52) * p + 1.0; };
    const double m0 = 0.875 * p + 1.0;
    const double a1 = 2 * m0, b1 = diff(2 * m0);
    const double a2 = 2 * std::fmax(a1, b1), b2 = diff(a2);       // a2 is re-centred to 0.5 p + 1 afterwards
    const double s2 = std::fmax(0.5 * p + 1.0, b2);
    const double a3 = 2 * s2, b3 = diff(a3);
    const double a4 = 2 * std::fmax(a3, b3);
    seen(a2, "inverse block of a1 (.) b1, layer 2 (worst case)");
    seen(a4, "inverse block of a1 (.) b1, layer 4 (worst case)");
    printf("bounds q=%llu: forward block from held_tail_in %.4f, Q - y %.4f, inverse block of a1.b1 %.4f (x 2^50)\n", q, f / 0x1p50, (y + p) / 0x1p50, a4 / 0x1p50);
}

// (b) + (c): whole transforms at N = 2^log_n with the kernel's schedule, against the oracle
static void check_transforms(unsigned log_n, u64 q, u64 ql, int pattern) {
    const size_t n = (size_t)1 << log_n;
    const Md m = make(q);
    const double p = m.m.p;
    orc_ntt_tables* t = orc_ntt_tables_create(log_n, q);
    if (!t) { printf("no tables for %llu\n", q); g_bad++; return; }
    const orc_ntt_tables* tt = t;
    auto word = [&](size_t i, u64 salt) -> u64 {
        switch (pattern) {
            case 0: return q - 1;
            case 1: return 0;
            case 2: return (i & 1) ? q - 1 : 0;
            case 3: return (i & 1) ? q / 2 + 1 : q / 2;
            default: { u64 s = (i + 1) * 0x9e3779b97f4a7c15ull + salt; s ^= s >> 29; s *= 0xbf58476d1ce4e5b9ull; s ^= s >> 32; return s % q; }
        }
    };
    // ---- inverse of a1 (.) b1 -> digits as doubles: rounds of 4, 4, 4, 2 layers, sums re-centred after 2 of 4, the last layer folded with N^-1 ----
    std::vector<uint64_t> ref(n);
    std::vector<double> x(n);
    for (size_t i = 0; i < n; i++) {
        const u64 a = word(i, 1), b = word(i, 2);
        ref[i] = mulmod(a, b, q);
        x[i] = prod_in(a, b, m);                      // enters the first round as it is (to_lds_raw)
        seen(x[i], "a1 (.) b1");
    }
    orc_ntt_inverse(ref.data(), 1, 1, log_n, &tt, 1, 0, 0);
    const u64 ninv_u = invmod((u64)n % q, q);
    const double ninv = (double)ninv_u, ninv_p = ninv * m.m.inv_p;
    double max_inv = 0.0;
    for (unsigned layer = 0; layer < log_n; layer++) {
        const size_t gap = (size_t)1 << layer, mm = n >> (layer + 1);
        const bool last = layer + 1 == log_n;
        for (size_t g = 0; g < mm; g++) {
            const u64 wu = t->inv_root_powers[n - 2 * mm + 1 + g].operand;
            const double w = last ? (double)mulmod(wu, ninv_u, q) : (double)wu;
            for (size_t j = 0; j < gap; j++) {
                const size_t a = 2 * g * gap + j, b = a + gap;
                const double u = x[a], v = x[b];
                x[a] = u + v;
                seen(u - v, "inverse u - v");
                x[b] = f64_mulq(u - v, w, m.m.inv_p, p);
                seen(x[a], "inverse sum");
                max_inv = std::fmax(max_inv, std::fmax(std::fabs(x[a]), std::fabs(u - v)));
                if (layer % 4 == 1 && layer + 2 < log_n) x[a] = f64_corr(x[a], m.m);      // mid-block re-centring (blocks of 4 layers only)
            }
        }
        if ((layer + 1) % 4 == 0 && !last) for (size_t i = 0; i < n; i++) x[i] = f64_corr(x[i], m.m);      // exchange
    }
    int bad_inv = 0;
    for (size_t i = 0; i < n; i++) {
        const bool scaled = (i >> (log_n - 1)) & 1;       // the folded layer's difference outputs carry N^-1 already
        const double xr = scaled ? x[i] : f64_mulc(x[i], ninv, ninv_p, p);
        const u64 bits = digit_word(xr, 0.0, 0xffffffffu, m);                 // NTT_FLAG_STORE_F64: the double ksmac2 reads
        const u64 word = digit_word(xr, F64_TWO52, 0x000fffffu, m);            // the canonical word
        if (f64_bits_to_double(bits) != (double)ref[i] || bits != f64_double_to_bits(f64_from_u64(ref[i])) || word != ref[i]) bad_inv++;
    }
    if (bad_inv) { printf("MISMATCH: inverse of a1.b1 q=%llu pattern %d: %d words\n", q, pattern, bad_inv); g_bad += bad_inv; }
    // ---- forward from the hand-over's extremes -> (Q - y) ql^-1: rounds of 4, 4, 4, 2 layers, the last round's outputs not re-centred ----
    std::vector<uint64_t> in(n), fref(n);
    const double xmax = std::floor(0.6875 * p) + (0x1p49 - 1.0);
    for (size_t i = 0; i < n; i++) {
        const u64 wv = word(i, 3);
        double v;
        if (pattern < 4) v = (wv > q / 2 ? 1.0 : -1.0) * xmax - (double)(i % 3);       // the largest magnitudes held_tail_in can give
        else v = (double)wv - ((i & 2) ? p : 0.0);
        x[i] = v;
        in[i] = canon_d(v, q);
    }
    fref = in;
    orc_ntt_forward(fref.data(), 1, 1, log_n, &tt, 1, 0, 0);
    double max_fwd = 0.0, max_y = 0.0;
    for (unsigned layer = 0; layer < log_n; layer++) {
        const size_t mm = (size_t)1 << layer, gap = n >> (layer + 1);
        for (size_t g = 0; g < mm; g++) {
            const double w = (double)t->root_powers[mm + g].operand;
            for (size_t j = 0; j < gap; j++) {
                const size_t a = 2 * g * gap + j, b = a + gap;
                const double r = f64_mulq(x[b], w, m.m.inv_p, p), u = x[a];
                x[a] = u + r; x[b] = u - r;
                seen(x[a], "forward"); seen(x[b], "forward");
                max_fwd = std::fmax(max_fwd, std::fmax(std::fabs(x[a]), std::fabs(x[b])));
            }
        }
        if ((layer + 1) % 4 == 0 && layer + 1 < log_n) for (size_t i = 0; i < n; i++) x[i] = f64_corr(x[i], m.m);
    }
    const u64 inv_lj_u = invmod(ql, q);
    int bad_fwd = 0;
    for (size_t i = 0; i < n; i++) {
        max_y = std::fmax(max_y, std::fabs(x[i]));
        for (u64 Q : {(u64)0, (u64)1, q - 1, q / 2, q / 2 + 1, word(i, 4)}) {
            seen(f64_from_u64(Q) - x[i], "Q - y");
            const u64 got = tail_out(Q, x[i], (double)inv_lj_u, m);
            const u64 want = mulmod(canon_i((i128_)Q - (i128_)fref[i], q), inv_lj_u, q);
            if (got != want) bad_fwd++;
        }
    }
    if (bad_fwd) { printf("MISMATCH: forward + tail_out q=%llu pattern %d: %d words\n", q, pattern, bad_fwd); g_bad += bad_fwd; }
    printf("transforms logn=%u q=%llu pattern %d: inverse max %.4f, forward max %.4f, last round |y| max %.4f (x p)\n", log_n, q, pattern, max_inv / p, max_fwd / p, max_y / p);
    orc_ntt_tables_destroy(t);
}

int main() {
    const unsigned log_n = 14;
    const u64 two_n = 2ull << log_n;
    // the flagship chain, and the ends of the 50-bit class for this ring
    const size_t bits[6] = {50, 50, 50, 50, 50, 50};
    uint64_t chain[6];
    if (orc_coeff_modulus_create((size_t)1 << log_n, bits, 6, chain) != 0) { printf("no chain\n"); return 2; }
    u64 largest = 0, smallest = 0;
    for (u64 c = ((1ull << 50) - 1) / two_n * two_n + 1; c > (1ull << 49); c -= two_n) if (c < (1ull << 50) && orc_is_prime(c)) { largest = c; break; }
    for (u64 c = (1ull << 49) / two_n * two_n + 1; c < (1ull << 50); c += two_n) if (c > (1ull << 49) && orc_is_prime(c)) { smallest = c; break; }
    u64 second = 0;
    for (u64 c = largest - two_n; c > (1ull << 49); c -= two_n) if (orc_is_prime(c)) { second = c; break; }
    printf("chain:"); for (u64 c : chain) printf(" %llu", (u64)c); printf("\nlargest %llu second %llu smallest %llu\n", largest, second, smallest);
    std::vector<u64> all(chain, chain + 6);
    all.push_back(largest); all.push_back(second); all.push_back(smallest);
    // hand-over: the chain as it is used (special prime = last, dropped limb = L - 1 = 4, output limbs 0..3), and the ends mixed both ways
    for (int j = 0; j < 4; j++) check_handover(chain[5], chain[4], chain[j]);
    check_handover(largest, second, smallest);
    check_handover(smallest, largest, second);
    check_handover(second, smallest, largest);
    check_handover(largest, smallest, second);
    for (u64 q : all) check_bounds(q);
    check_bounds((1ull << 50) - 1);      // the supremum of the class (not a prime: the recurrence only)
    for (u64 q : all) for (int pattern = 0; pattern < 5; pattern++) check_transforms(log_n, q, q == chain[4] ? chain[5] : chain[4], pattern);
    printf("largest value seen: %.4f x 2^53\n", g_max);
    printf(g_bad ? "FAILED (%d)\n" : "ALL EXACT\n", g_bad);
    return g_bad != 0;
}
