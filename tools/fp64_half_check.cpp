// Host-side exactness check of mulpair_half_kernel (csrc/mulpair_half_kernels.hpp): the inverse transform of a1 (.) b1 at N = 16384 as two half-limb
// transforms of 5 + 5 + 3 Gentleman-Sande layers and one last layer across the halves.  A host build of the REAL csrc/dev_math_f64.hpp; the sequence
// below is the kernel's, in its order: the product enters as it is, every block (round A = layers 0..4, round B = 5..9, round C + the last layer =
// 10..13) re-centres the SUM outputs of its 2nd and of its 4th layer, every word is re-centred at the two exchanges, the last layer is folded with
// N^-1 and the digits leave through ArithF64::digit_word.  Every butterfly is compared with 128-bit integer arithmetic, the digits with the CPU
// oracle's inverse transform, every integer-valued intermediate is checked against 2^53, and the maxima reached per block are printed next to the
// worst-case recurrence of the header comment (with the +1 of every rounding).  Exit status 0 only if everything is exact and in range.
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -mfma -I troy-nova_amd/csrc tools/fp64_half_check.cpp oracle/troy_oracle.o -o fp64_half_check
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
static u64 mulmod(u64 a, u64 b, u64 p) { return (u64)((u128_)a * b % p); }
static u64 canon_i(i128_ v, u64 p) { i128_ r = v % (i128_)p; if (r < 0) r += p; return (u64)r; }
static u64 canon_d(double v, u64 p) { return canon_i((i128_)v, p); }      // |v| < 2^53: exact
static u64 powmod(u64 a, u64 e, u64 p) { u64 r = 1; while (e) { if (e & 1) r = mulmod(r, a, p); a = mulmod(a, a, p); e >>= 1; } return r; }
static u64 invmod(u64 a, u64 p) { return powmod(a % p, p - 2, p); }

static u64 digit_word(double x, double add, unsigned mask_hi, const F64Mod& m) {      // ArithF64::digit_word behind its N^-1 step
    double c = f64_corr(x, m);
    c = c < 0.0 ? c + m.p : c;
    return f64_double_to_bits(c + add) & (((u64)mask_hi << 32) | 0xffffffffull);
}

// the block structure of the kernel: layer (= index bit, low bit first) -> position inside its block
static int block_of(unsigned layer) { return layer < 5 ? 0 : layer < 10 ? 1 : 2; }
static int pos_in_block(unsigned layer) { return layer < 5 ? layer : layer < 10 ? layer - 5 : layer - 10; }

// worst case of the header comment with the +1 of every rounding: returns the peak of the three blocks (operands of any operation)
static double check_recurrence(double p, bool print) {
    auto diff = [&](double d) { return (0.5 + 1.5 * d * 0x1p-52) * p + 1.0; };
    const double start[3] = {0.875 * p + 1.0, 0.5 * p + 1.0, 0.5 * p + 1.0};
    const int layers[3] = {5, 5, 4};
    double peak_all = 0.0;
    for (int b = 0; b < 3; b++) {
        double m = start[b], peak = m;
        for (int l = 0; l < layers[b]; l++) {
            const double s = 2 * m, d = diff(2 * m);        // |u + v|, |u - v| <= 2 m
            peak = std::fmax(peak, s);
            seen(s, "recurrence: u + v / u - v");
            m = (l == 1 || l == 3) ? std::fmax(0.5 * p + 1.0, d) : std::fmax(s, d);
        }
        if (b == 2) { seen(diff(peak), "recurrence: last layer's products"); }
        if (print) printf("  block %c: peak %.4f x p\n", "ABC"[b], peak / p);
        peak_all = std::fmax(peak_all, peak);
    }
    return peak_all;
}

static void check_transform(unsigned log_n, u64 q, int pattern) {
    const size_t n = (size_t)1 << log_n;
    const F64Mod m{(double)q, 1.0 / (double)q};
    const double p = m.p;
    orc_ntt_tables* t = orc_ntt_tables_create(log_n, q);
    if (!t) { printf("no tables for %llu\n", (unsigned long long)q); g_bad++; return; }
    const orc_ntt_tables* tt = t;
    auto word = [&](size_t i, u64 salt) -> u64 {
        switch (pattern) {
            case 0: return q - 1;
            case 1: return 0;
            case 2: return (i & 1) ? q - 1 : 0;
            case 3: return (i & 1) ? q / 2 + 1 : q / 2;
            case 4: return i == 0 || i == n - 1 || i == n / 2 - 1 || i == n / 2 ? q - 1 : 0;      // impulses, both sides of the half boundary
            default: { u64 s = (i + 1) * 0x9e3779b97f4a7c15ull + salt; s ^= s >> 29; s *= 0xbf58476d1ce4e5b9ull; s ^= s >> 32; return s % q; }
        }
    };
    std::vector<uint64_t> ref(n);
    std::vector<double> x(n);
    for (size_t i = 0; i < n; i++) {
        const u64 a = word(i, 1), b = word(i, 2);
        ref[i] = mulmod(a, b, q);
        x[i] = f64_mulq(f64_from_u64(a), f64_from_u64(b), m.inv_p, p);      // the product in the loaded layout, as it is
        seen(x[i], "a1 (.) b1");
        if (canon_d(x[i], q) != ref[i]) { g_bad++; if (g_bad < 20) printf("MISMATCH: product q=%llu\n", (unsigned long long)q); }
        if (std::fabs(x[i]) > 0.875 * p + 1.0) { g_bad++; if (g_bad < 20) printf("BOUND: product %.4f p\n", std::fabs(x[i]) / p); }
    }
    orc_ntt_inverse(ref.data(), 1, 1, log_n, &tt, 1, 0, 0);
    const u64 ninv_u = invmod((u64)n % q, q);
    const double ninv = (double)ninv_u, ninv_p = ninv * m.inv_p;
    double peak[3] = {0.0, 0.0, 0.0};
    int bad_bf = 0;
    for (unsigned layer = 0; layer < log_n; layer++) {
        const size_t gap = (size_t)1 << layer, mm = n >> (layer + 1);
        const bool last = layer + 1 == log_n;
        const int blk = block_of(layer), pos = pos_in_block(layer);
        for (size_t g = 0; g < mm; g++) {
            const u64 wu0 = t->inv_root_powers[n - 2 * mm + 1 + g].operand;
            const u64 wu = last ? mulmod(wu0, ninv_u, q) : wu0;        // the folded last layer: w N^-1
            const double w = (double)wu;
            for (size_t j = 0; j < gap; j++) {
                const size_t a = 2 * g * gap + j, b = a + gap;
                const double u = x[a], v = x[b];
                const double s = u + v, d = u - v;
                seen(s, "u + v"); seen(d, "u - v");
                peak[blk] = std::fmax(peak[blk], std::fmax(std::fabs(s), std::fabs(d)));
                const double r = f64_mulq(d, w, m.inv_p, p);
                seen(r, "(u - v) w");
                if (canon_d(r, q) != mulmod(canon_d(d, q), wu, q) || std::fabs(r) > (0.5 + 1.5 * std::fabs(d) * 0x1p-52) * p + 1.0) bad_bf++;
                const bool fix = (pos == 1 || pos == 3) && !last;        // the 2nd and the 4th layer of a block re-centre their sums (the last layer's go to N^-1)
                x[a] = fix ? f64_corr(s, m) : s;
                if (fix && (canon_d(x[a], q) != canon_d(s, q) || std::fabs(x[a]) > 0.5 * p + 1.0)) bad_bf++;
                x[b] = r;
            }
        }
        if (layer == 4 || layer == 9) for (size_t i = 0; i < n; i++) x[i] = f64_corr(x[i], m);      // the two exchanges
    }
    if (bad_bf) { printf("MISMATCH: butterflies q=%llu pattern %d: %d\n", (unsigned long long)q, pattern, bad_bf); g_bad += bad_bf; }
    int bad = 0;
    for (size_t i = 0; i < n; i++) {
        const bool scaled = (i >> (log_n - 1)) & 1;       // the folded layer's difference outputs carry N^-1 already
        const double xr = scaled ? x[i] : f64_mulc(x[i], ninv, ninv_p, p);
        seen(xr, "digit in front of digit_word");
        const u64 bits = digit_word(xr, 0.0, 0xffffffffu, m);                 // NTT_FLAG_STORE_F64: the double ksmac2 reads
        const u64 wd = digit_word(xr, F64_TWO52, 0x000fffffu, m);              // the canonical word
        if (f64_bits_to_double(bits) != (double)ref[i] || bits != f64_double_to_bits(f64_from_u64(ref[i])) || wd != ref[i]) bad++;
    }
    if (bad) { printf("MISMATCH: digits q=%llu pattern %d: %d words\n", (unsigned long long)q, pattern, bad); g_bad += bad; }
    printf("transform q=%llu pattern %d: peaks A %.4f B %.4f C+last %.4f (x p)\n", (unsigned long long)q, pattern, peak[0] / p, peak[1] / p, peak[2] / p);
    // the maxima reached stay inside the derived bounds (header comment): 7.25 p, 5 p, 5 p (+ the +1 terms)
    const double bound[3] = {7.25, 5.0, 5.0};
    for (int b = 0; b < 3; b++) if (peak[b] > bound[b] * p + 64.0) { printf("BOUND: block %c reaches %.4f p > %.4f p\n", "ABC"[b], peak[b] / p, bound[b]); g_bad++; }
    orc_ntt_tables_destroy(t);
}

int main() {
    const unsigned log_n = 14;
    const u64 two_n = 2ull << log_n;
    // the flagship chain, both ends of the 50-bit class for this ring, and the smallest primes the ring has at all (the FP64 policy takes every
    // modulus below 2^50; the bounds are multiples of p, so small moduli are far from 2^53 -- replayed for the +1 terms)
    const size_t bits[6] = {50, 50, 50, 50, 50, 50};
    uint64_t chain[6];
    if (orc_coeff_modulus_create((size_t)1 << log_n, bits, 6, chain) != 0) { printf("no chain\n"); return 2; }
    u64 largest = 0, second = 0, smallest50 = 0, smallest = 0;
    for (u64 c = ((1ull << 50) - 1) / two_n * two_n + 1; c > (1ull << 49); c -= two_n) if (c < (1ull << 50) && orc_is_prime(c)) { largest = c; break; }
    for (u64 c = largest - two_n; c > (1ull << 49); c -= two_n) if (orc_is_prime(c)) { second = c; break; }
    for (u64 c = (1ull << 49) / two_n * two_n + 1; c < (1ull << 50); c += two_n) if (c > (1ull << 49) && orc_is_prime(c)) { smallest50 = c; break; }
    for (u64 c = two_n + 1; c < (1ull << 49); c += two_n) if (orc_is_prime(c)) { smallest = c; break; }
    printf("chain:"); for (u64 c : chain) printf(" %llu", (unsigned long long)c);
    printf("\nlargest %llu second %llu smallest 50-bit %llu smallest %llu\n", (unsigned long long)largest, (unsigned long long)second, (unsigned long long)smallest50, (unsigned long long)smallest);
    std::vector<u64> all(chain, chain + 6);
    all.push_back(largest); all.push_back(second); all.push_back(smallest50); all.push_back(smallest);
    printf("recurrence at the supremum of the class, p = 2^50 - 1:\n");
    const double sup = check_recurrence((double)((1ull << 50) - 1), true);
    printf("worst case peak %.4f x 2^50\n", sup / 0x1p50);
    for (u64 q : all) check_recurrence((double)q, false);
    for (u64 q : all) for (int pattern = 0; pattern < 6; pattern++) check_transform(log_n, q, pattern);
    printf("largest value seen: %.4f x 2^53\n", g_max);
    printf(g_bad ? "FAILED (%d)\n" : "ALL EXACT\n", g_bad);
    return g_bad != 0;
}
