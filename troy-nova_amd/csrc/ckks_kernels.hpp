// ckks_kernels.hpp -- the CKKS encoder on the device (ckks_encoder.cu): the canonical-embedding FFT in FP64, the RNS reduction of the
// rounded coefficients, and the CRT composition of a decoded plaintext.
//
// Bit-exactness.  The host transforms (CKKSEncoder::encode_complex64_simd / decode_complex64_simd, troy/troy.cpp) are radix-2 layers of
// IEEE double additions, subtractions and multiplications on table roots, compiled without FMA; this unit is compiled with
// -ffp-contract=off.  A butterfly here reads the same two points and the same table entry and evaluates the same expression tree
// (dr*rr - di*ri, dr*ri + di*rr / wr*rr - wi*ri, wr*ri + wi*rr), and a layer's butterflies are independent, so the result does not depend on
// how layers are divided among passes, workgroups, threads and register rounds: every point holds the host's bits after every layer.
//
// Shape.  A workgroup transforms a tile of 2^TB points, 8 per thread (ntt_sizes.hpp, column fft).  Up to three layers run on a thread's
// registers (a "round"), then the tile is exchanged through the LDS.  N <= 8192: one tile is the whole transform.  N >= 16384: two passes as
// in the NTT kernels -- the layers of gap < 2^TB on contiguous tiles, the layers of gap >= 2^TB on tiles of 2^(2 TB - log N) consecutive
// columns x 2^(log N - TB) rows; the points travel between the passes as double2 in the workspace.
//
// LDS.  Real and imaginary parts live in two planes of doubles (8-byte accesses: ds_read_b64 is served in 32-lane halves over 64 banks,
// ds_write_b64 in 16-lane groups over 32), point x at slot x + (x >> 3).  A round at bit s holds the points hi.k.lo (k = 3 bits at s): for
// s = 0 a half-wave's lanes are 9 slots = 18 banks apart (odd multiple of 2: all distinct), for s = 3 the 8-lane runs start 72 slots = 16 banks
// (mod 64) apart, for s >= 5 the lanes are consecutive and the pad costs a 2-way conflict on 3 of 32 lanes.  A 16-byte layout (ds_read_b128
// in four interleaved 16-lane groups, ds_write_b128 at 13 cycles) has no pad that serves every round.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "dev_math.hpp"

namespace troyn {

constexpr int CKKS_MAX_L = 16;            // decode: at most 16 primes (< 2^61 each) in 16 words

struct CkksFftArgs {
    const double2* roots;                 // [N]: inv_root_powers (encode) / root_powers (decode)
    const unsigned* slot_of;              // [N]: i with index_map[i] == position
    const double2* values;                // encode, first pass: [batch][count]
    unsigned count;
    const double* coeffs;                 // decode, first pass: [batch][N] real coefficients
    double2* work;                        // [batch][N] between the passes of the two-pass form
    double2* slots;                       // decode, last pass: [batch][N/2]
    u64* residues;                        // encode, last pass: [batch][L][N]
    const DevModulus* mods;
    unsigned L;
    double fix;                           // scale / N
    unsigned* too_large;                  // [batch] or null
    // encode, first pass, SRC != CKKS_SRC_VALUES (appended: the fields above keep their kernarg offsets)
    const double2* table;                 // diagonals [nd][n] / row-major matrix [n][n]
    const uint2* pairs;                   // [batch]: (a_t, s_t) = (diagonal, shift)
    unsigned n_mask, n_log, a_max;        // n - 1, log2 n, nd - 1 (diagonals: a_t is clamped) / n - 1 (matrix: a_t is masked)
};

// where the first pass of an encoding reads slot i of item t from
constexpr int CKKS_SRC_VALUES = 0;        // values[t][i], zero beyond count
constexpr int CKKS_SRC_DIAGONALS = 1;     // table[a_t][(i - s_t) mod n]
constexpr int CKKS_SRC_MATRIX = 2;        // table[j][(j + a_t) mod n], j = (i - s_t) mod n

// ---- rounded coefficient -> residues (set_plaintext, troy/troy.cpp) ---------------------------------------------------------------
struct CkksInt128 { u64 lo, hi; bool neg, too_large; };

__device__ __forceinline__ CkksInt128 ckks_round_split(double c) {
    const double two64 = 18446744073709551616.0;
    const double v = rint(c);                              // round half to even, as std::nearbyint in the default mode
    CkksInt128 r;
    r.neg = v < 0;
    const double a = fabs(v);
    r.too_large = !(a < two64 * two64);                     // a NaN is flagged as well
    r.hi = (u64)(a / two64);
    r.lo = (u64)(a - (double)r.hi * two64);
    return r;
}

__device__ __forceinline__ u64 ckks_residue(const CkksInt128& x, const DevModulus& m) {
    // below 2^64 (every practical scale): one Barrett reduction; both give the canonical residue the host's % gives
    const u64 r = x.hi ? barrett128(x.lo, x.hi, m.q, m.ratio_lo, m.ratio_hi) : barrett64(x.lo, m.q, m.ratio_hi);
    return (x.neg && r) ? m.q - r : r;
}

// ---- the FFT tile -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ckks_lds_slot(unsigned x) { return x + (x >> 3); }
constexpr unsigned ckks_lds_slots(int tb) { return (1u << tb) + (1u << (tb - 3)); }

// DEC = false: Gentleman-Sande layers with inv_root_powers, gap 1 upwards (encode).  DEC = true: Cooley-Tukey layers with root_powers, gap
// N/2 downwards (decode).  STRIDED: the pass over the layers of gap >= 2^TB (two-pass sizes only).
template <int LOGN, int TB, bool DEC, bool STRIDED, int SRC = CKKS_SRC_VALUES>
__global__ __launch_bounds__(1 << (TB - 3)) void ckks_fft_kernel(CkksFftArgs a) {
    static_assert(SRC == CKKS_SRC_VALUES || (!DEC && !STRIDED), "a diagonal source feeds the first pass of an encoding");
    static_assert(TB >= 6 && TB <= 13 && TB <= LOGN && 2 * TB >= LOGN, "tile geometry");
    static_assert(!STRIDED || TB < LOGN, "the strided pass exists at the two-pass sizes only");
    constexpr int LO = STRIDED ? 2 * TB - LOGN : 0;              // the tile's layers are its local bits LO .. TB-1
    constexpr int NL = TB - LO, ROUNDS = (NL + 2) / 3;
    constexpr unsigned N = 1u << LOGN;
    constexpr bool TWO_PASS = TB < LOGN;
    constexpr bool FIRST = !TWO_PASS || (DEC == STRIDED), LAST = !TWO_PASS || (DEC != STRIDED);
    __shared__ double lre[ROUNDS > 1 ? ckks_lds_slots(TB) : 1], lim[ROUNDS > 1 ? ckks_lds_slots(TB) : 1];
    const unsigned t = threadIdx.x;
    const unsigned tile = blockIdx.x & ((1u << (LOGN - TB)) - 1), item = blockIdx.x >> (LOGN - TB);
    // local point of register k in a round at bit s, and its position in the transform
    auto local_of = [&](int s, int k) -> unsigned { return ((t >> s) << (s + 3)) | ((unsigned)k << s) | (t & ((1u << s) - 1)); };
    auto global_of = [&](unsigned x) -> unsigned {
        if (STRIDED) return ((x >> LO) << TB) | (tile << LO) | (x & ((1u << LO) - 1));
        return (tile << TB) | x;
    };
    auto round_bit = [](int r) -> int {                           // the lowest local bit of the 8 points a thread holds in round r
        if (!DEC) return LO + 3 * r < TB - 3 ? LO + 3 * r : TB - 3;
        const int s = TB - 3 * (r + 1), floor = LO < TB - 3 ? LO : TB - 3;
        return s > floor ? s : floor;
    };
    double re[8], im[8];
    const size_t item_base = (size_t)item * N;

    // ---- load ----
    {
        const int s = round_bit(0);
        // a diagonal source: the item's (diagonal, shift), uniform over the workgroup; out-of-range words cannot leave the table
        unsigned src_a = 0, src_s = 0;
        if constexpr (SRC != CKKS_SRC_VALUES) {
            const uint2 pr = a.pairs[item];
            src_s = pr.y & a.n_mask;
            src_a = SRC == CKKS_SRC_DIAGONALS ? (pr.x < a.a_max ? pr.x : a.a_max) : (pr.x & a.n_mask);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const unsigned g = global_of(local_of(s, k));
            if (!FIRST) {
                const double2 v = a.work[item_base + g];
                re[k] = v.x; im[k] = v.y;
            } else if (DEC) {
                re[k] = a.coeffs[item_base + g]; im[k] = 0.0;
            } else {
                // set_conjugate_values: slot i at index_map[i], its conjugate at index_map[i + N/2]; zero beyond count
                const unsigned i = a.slot_of[g], slot = i & (N / 2 - 1);
                re[k] = 0.0; im[k] = 0.0;
                if constexpr (SRC != CKKS_SRC_VALUES) {
                    // the pre-rotated diagonal, selected while loading: every slot is present (count = N/2), a short diagonal repeats
                    const unsigned j = (slot - src_s) & a.n_mask;
                    const size_t at = SRC == CKKS_SRC_DIAGONALS ? ((size_t)src_a << a.n_log) + j : ((size_t)j << a.n_log) + ((j + src_a) & a.n_mask);
                    const double2 v = a.table[at];
                    re[k] = v.x; im[k] = (i >= N / 2) ? -v.y : v.y;
                } else if (slot < a.count) {
                    const double2 v = a.values[(size_t)item * a.count + slot];
                    re[k] = v.x; im[k] = (i >= N / 2) ? -v.y : v.y;
                }
            }
        }
    }

    // ---- rounds ----
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        const int s = round_bit(r);
        if (r > 0) {
            const int sp = round_bit(r - 1);
            if (r > 1) __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; k++) { const unsigned p = ckks_lds_slot(local_of(sp, k)); lre[p] = re[k]; lim[p] = im[k]; }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; k++) { const unsigned p = ckks_lds_slot(local_of(s, k)); re[k] = lre[p]; im[k] = lim[p]; }
        }
        // the layers of this round: local bits [l0, l1), ascending for encode, descending for decode
        const int l0 = DEC ? (TB - 3 * (r + 1) > LO ? TB - 3 * (r + 1) : LO) : LO + 3 * r;
        const int l1 = DEC ? TB - 3 * r : (LO + 3 * (r + 1) < TB ? LO + 3 * (r + 1) : TB);
#pragma unroll
        for (int step = 0; step < 3; step++) {
            const int l = DEC ? l1 - 1 - step : l0 + step;
            if (l < l0 || l >= l1) continue;
            const int kb = l - s;                                   // the layer's bit inside k
            const int sg = STRIDED ? l + (LOGN - TB) : l;           // the layer's gap is 2^sg in the whole transform
#pragma unroll
            for (int grp = 0; grp < (8 >> (kb + 1)); grp++) {
                const int ktop = grp << (kb + 1);
                const unsigned group = global_of(local_of(s, ktop)) >> (sg + 1);
                // the host loops count root_index up from 1 across the layers
                const unsigned ri_ = DEC ? (N >> (sg + 1)) + group : N - (N >> sg) + 1 + group;
                const double2 w = a.roots[ri_];
                const double rr = w.x, ri = w.y;
#pragma unroll
                for (int j = 0; j < (1 << kb); j++) {
                    const int top = ktop | j, bot = top | (1 << kb);
                    if (!DEC) {
                        const double dr = re[top] - re[bot], di = im[top] - im[bot];
                        re[top] = re[top] + re[bot]; im[top] = im[top] + im[bot];
                        re[bot] = dr * rr - di * ri; im[bot] = dr * ri + di * rr;
                    } else {
                        const double vr = re[bot] * rr - im[bot] * ri, vi = re[bot] * ri + im[bot] * rr;
                        const double ur = re[top], ui = im[top];
                        re[top] = ur + vr; im[top] = ui + vi;
                        re[bot] = ur - vr; im[bot] = ui - vi;
                    }
                }
            }
        }
    }

    // ---- store ----
    const int s = round_bit(ROUNDS - 1);
    if (!LAST) {
#pragma unroll
        for (int k = 0; k < 8; k++) a.work[item_base + global_of(local_of(s, k))] = make_double2(re[k], im[k]);
    } else if (DEC) {
        // slot i <- position index_map[i]: every position of the first half of the map holds one slot
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const unsigned i = a.slot_of[global_of(local_of(s, k))];
            if (i < N / 2) a.slots[(size_t)item * (N / 2) + i] = make_double2(re[k], im[k]);
        }
    } else {
        // coefficient = re * (scale / N), rounded, reduced modulo every prime: L rows from one read of the coefficient
        CkksInt128 c[8];
        bool too = false;
#pragma unroll
        for (int k = 0; k < 8; k++) { c[k] = ckks_round_split(re[k] * a.fix); too |= c[k].too_large; }
        if (too && a.too_large) a.too_large[item] = 1u;
        for (unsigned i = 0; i < a.L; i++) {
            const DevModulus m = a.mods[i];
            u64* row = a.residues + ((size_t)item * a.L + i) * N;
#pragma unroll
            for (int k = 0; k < 8; k++) row[global_of(local_of(s, k))] = ckks_residue(c[k], m);
        }
    }
}

// ---- encode_float64_polynomial: coefficient j = coeffs[j] * scale, zero beyond count -----------------------------------------------
static __global__ __launch_bounds__(256) void ckks_encode_polynomial_kernel(const double* coeffs, unsigned count, double scale, unsigned n, const DevModulus* mods,
                                                                            unsigned L, u64* residues, unsigned* too_large) {
    const unsigned chunks = n / 256, item = blockIdx.x / chunks, j = (blockIdx.x % chunks) * 256 + threadIdx.x;
    CkksInt128 c = {0, 0, false, false};
    if (j < count) c = ckks_round_split(coeffs[(size_t)item * count + j] * scale);
    if (c.too_large && too_large) too_large[item] = 1u;
    for (unsigned i = 0; i < L; i++) residues[((size_t)item * L + i) * n + j] = ckks_residue(c, mods[i]);
}

// ---- decode: residues (coefficient form) -> the centred integer, correctly rounded to double, divided by the scale -------------------
struct CkksComposeArgs {
    const u64* residues;                  // [batch][L][N]
    const DevModulus* mods;
    const ulonglong2* garner;             // [K][K]: (operand, quotient) of q_j^-1 mod q_i at [i][j], j < i
    unsigned K, L, n;
    const u64* q_words;                   // [CKKS_MAX_L] little-endian words of Q = q_0 ... q_{L-1}
    const u64* half_words;                // floor(Q / 2)
    double scale;
    double* out;                          // [batch][N]
};

// f(std::integral_constant<int, I>) for I = BEGIN .. END-1: a loop whose counter is a constant of every iteration
template <int BEGIN, int END, class F>
__device__ __forceinline__ void ckks_static_for(F&& f) {
    if constexpr (BEGIN < END) { f(std::integral_constant<int, BEGIN>{}); ckks_static_for<BEGIN + 1, END>(f); }
}

// Mixed-radix (Garner) digit i of a coefficient: X = d_0 + q_0 (d_1 + q_1 (d_2 + ...)), 0 <= d_i < q_i.  `residue` is the word of row i, d[0..i)
// the digits below, m = mods[i], garner_row = garner + i * K.  Shared by the decoder's composition and the base extension of
// raise_kernels.hpp.  i is a constant at every call (an unrolled loop's counter, or ckks_static_for's), so d stays in registers.
template <int LM>
__device__ __forceinline__ u64 ckks_mixed_radix_digit(int i, u64 residue, const u64 (&d)[LM], const DevModulus m, const ulonglong2* garner_row) {
    u64 v = barrett64(residue, m.q, m.ratio_hi);
#pragma unroll
    for (int j = 0; j < i; j++) {
        const ulonglong2 w = garner_row[j];
        v = shoup_mul(sub_mod(v, barrett64(d[j], m.q, m.ratio_hi), m.q), w.x, w.y, m.q);
    }
    return v;
}

// LM: the primes and the words held in registers (L <= LM; every loop is unrolled, so nothing is indexed at run time)
template <int LM>
__global__ __launch_bounds__(256) void ckks_compose_kernel(CkksComposeArgs a) {
    const unsigned chunks = a.n / 256, item = blockIdx.x / chunks, x = (blockIdx.x % chunks) * 256 + threadIdx.x;
    const unsigned L = a.L;
    u64 d[LM];
#pragma unroll
    for (int i = 0; i < LM; i++) {
        d[i] = 0;
        if ((unsigned)i < L)
            d[i] = ckks_mixed_radix_digit<LM>(i, a.residues[((size_t)item * L + i) * a.n + x], d, a.mods[i], a.garner + (size_t)i * a.K);
    }
    // Horner from the top digit: X as LM words (X < Q < 2^(61 L))
    u64 X[LM];
#pragma unroll
    for (int w = 0; w < LM; w++) X[w] = 0;
#pragma unroll
    for (int i = LM - 1; i >= 0; i--) {
        if ((unsigned)i < L) {
            const u64 q = a.mods[i].q;
            u64 carry = d[i];
#pragma unroll
            for (int w = 0; w < LM; w++) {
                const u128 p = (u128)X[w] * q + carry;
                X[w] = (u64)p; carry = (u64)(p >> 64);
            }
        }
    }
    // centred representative in (-Q/2, Q/2]: X > floor(Q/2) stands for X - Q
    bool greater = false, decided = false;
#pragma unroll
    for (int w = LM - 1; w >= 0; w--) {
        const u64 h = a.half_words[w];
        if (!decided && X[w] != h) { greater = X[w] > h; decided = true; }
    }
    if (greater) {
        u64 borrow = 0;
#pragma unroll
        for (int w = 0; w < LM; w++) {
            const u64 qw = a.q_words[w], t1 = qw - X[w], t2 = t1 - borrow;
            borrow = (qw < X[w]) | (t1 < borrow);
            X[w] = t2;
        }
    }
    // |x| -> nearest double, ties to even: the top 64 bits from the leading one, everything below as a sticky bit (bit 0 lies 10 places below
    // the rounding position of a 64-bit integer, so the u64 -> double conversion rounds the whole integer correctly)
    u64 top = 0, next = 0, sticky = 0;
    int top_word = 0, state = 0;
#pragma unroll
    for (int w = LM - 1; w >= 0; w--) {
        if (state == 0) { if (X[w]) { top = X[w]; top_word = w; state = 1; } }
        else if (state == 1) { next = X[w]; state = 2; }
        else sticky |= X[w];
    }
    double mag = 0.0;
    if (top) {
        const int lz = __clzll((long long)top);
        u64 m = lz ? (top << lz) | (next >> (64 - lz)) : top;
        const u64 rest = lz ? next << lz : next;
        if (rest | sticky) m |= 1;
        mag = ldexp((double)m, 64 * top_word - lz);
    }
    a.out[(size_t)item * a.n + x] = (greater ? -mag : mag) / a.scale;
}

// ---- factors of the special DFT (CoeffToSlot / SlotToCoeff; include/troyn.h, "Factors of the special DFT") --------------------------------
// The product of the radix-2 layers [first, first + count) of the special FFT on the rotation group (-3)^j, forward or inverse, written by its
// present diagonals in the layout the diagonal encoder reads: out[a][i] = M[i][(i + d_a) mod n].  One thread per (diagonal, slot); an entry
// is one product of butterfly coefficients in the order of application (tests/dft_factors_spec.py states the association), each multiply its
// own rounding: this unit is compiled with -ffp-contract=off.  Twiddles come from the handle's root_powers, the exponent (-3)^j from a
// running product over the bits of j (mod 2^32, which every 4 len divides).  No LDS; stores are double2, coalesced along the slot.
struct CkksDftFactorArgs {
    const double2* roots;                 // [N] root_powers
    double2* out;                         // [nd][n]
    double constant;
    unsigned log_n;                       // log2 N
    unsigned first, count;                // layers [first, first + count), count >= 1
    unsigned nd, wrap;                    // diagonals; wrap: first + count == log2 n (d_a = a 2^first for every a)
    unsigned inverse, conjugate, col_mask, row_mask;     // masks: 0 none, 1 even, 2 odd
};

// (-3)^(j mod 2^b) mod 2^32 by squaring over the b <= 14 low bits of j
__device__ __forceinline__ unsigned ckks_rotation_power(unsigned j, unsigned b) {
    unsigned p = 1, sq = 0u - 3u;
    for (unsigned t = 0; t < b; t++) { if ((j >> t) & 1) p *= sq; sq *= sq; }
    return p;
}

static __global__ __launch_bounds__(256) void ckks_dft_factor_kernel(CkksDftFactorArgs a) {
    const unsigned n = 1u << (a.log_n - 1);
    const unsigned row = blockIdx.x * 256u + threadIdx.x, da = blockIdx.y;
    if (row >= n) return;
    const unsigned reach = 1u << a.count;
    const unsigned d = (a.wrap || da < reach) ? da << a.first : n - ((a.nd - da) << a.first);
    const unsigned col = (row + d) & (n - 1);
    bool present = ((row ^ col) & ~((reach - 1) << a.first)) == 0;
    if (a.row_mask) present = present && (row & 1) == (a.row_mask == 2u);
    if (a.col_mask) present = present && (col & 1) == (a.col_mask == 2u);
    double ar = 0.0, ai = 0.0;
    if (present) {
        ar = a.constant;
        // forward: the layers upwards, the twiddle index from the row; inverse: downwards, from the column
        const unsigned j = a.inverse ? col : row;
        for (unsigned step = 0; step < a.count; step++) {
            const unsigned b = a.inverse ? a.first + a.count - 1 - step : a.first + step;
            const unsigned rb = (row >> b) & 1, cb = (col >> b) & 1;
            if (a.inverse ? rb : cb) {
                const unsigned k = (ckks_rotation_power(j, b) & ((8u << b) - 1)) << (a.log_n - b - 2);   // ((-3)^j mod 4 len) (2N / 4 len) in [0, 2N)
                const double2 r = a.roots[__brev(k & ((1u << a.log_n) - 1)) >> (32 - a.log_n)];
                double tr = r.x, ti = a.inverse ? -r.y : r.y;
                if ((k >> a.log_n) ^ (a.inverse ? cb : rb)) { tr = -tr; ti = -ti; }
                const double nr = ar * tr - ai * ti, ni = ar * ti + ai * tr;
                ar = nr; ai = ni;
            }
            if (a.inverse) { ar = ar * 0.5; ai = ai * 0.5; }
        }
        if (a.conjugate) ai = -ai;
    }
    a.out[(size_t)da * n + row] = make_double2(ar, ai);
}

// ---- the same factors on the sub-ring of n < N/2 slots (sparse packing; include/troyn.h, "Factors of the special DFT on n slots") ----------
// A sparsely packed message is a polynomial in Y = X^(N/2n); its special FFT has log2 n layers, and layer b's twiddle
// (zeta^(N/2n))^(((-3)^j mod 4 len) 4n / 4 len) is the full ring's layer b read from the same root_powers.  The table is therefore the one
// above on n rows: diagonal indices mod n, the wrap where first + count == log2 n.  Same geometry, same association, same unit
// (-ffp-contract=off): one thread per (diagonal, row), double2 stores coalesced along the row, no LDS.
struct CkksDftFactorSparseArgs {
    const double2* roots;                 // [N] root_powers
    double2* out;                         // [nd][n]
    double constant;
    unsigned log_n;                       // log2 N
    unsigned log_slots;                   // log2 n, 1 <= log_slots <= log_n - 1
    unsigned first, count;                // layers [first, first + count), count >= 1, first + count <= log_slots
    unsigned nd, wrap;                    // diagonals; wrap: first + count == log_slots
    unsigned inverse, conjugate, col_mask, row_mask;     // masks: 0 none, 1 even, 2 odd
};

static __global__ __launch_bounds__(256) void ckks_dft_factor_sparse_kernel(CkksDftFactorSparseArgs a) {
    const unsigned n = 1u << a.log_slots;
    const unsigned row = blockIdx.x * 256u + threadIdx.x, da = blockIdx.y;
    if (row >= n || da >= a.nd) return;
    const unsigned reach = 1u << a.count;
    const unsigned d = (a.wrap || da < reach) ? da << a.first : n - ((a.nd - da) << a.first);
    const unsigned col = (row + d) & (n - 1);
    bool present = ((row ^ col) & ~((reach - 1) << a.first)) == 0;
    if (a.row_mask) present = present && (row & 1) == (a.row_mask == 2u);
    if (a.col_mask) present = present && (col & 1) == (a.col_mask == 2u);
    double ar = 0.0, ai = 0.0;
    if (present) {
        ar = a.constant;
        const unsigned j = a.inverse ? col : row;
        for (unsigned step = 0; step < a.count; step++) {
            const unsigned b = a.inverse ? a.first + a.count - 1 - step : a.first + step;
            const unsigned rb = (row >> b) & 1, cb = (col >> b) & 1;
            if (a.inverse ? rb : cb) {
                // ((-3)^j mod 4 len) (2N / 4 len) in [0, 2N): b <= log_slots - 1 <= log_n - 2
                const unsigned k = (ckks_rotation_power(j, b) & ((8u << b) - 1)) << (a.log_n - b - 2);
                const double2 r = a.roots[__brev(k & ((1u << a.log_n) - 1)) >> (32 - a.log_n)];
                double tr = r.x, ti = a.inverse ? -r.y : r.y;
                if ((k >> a.log_n) ^ (a.inverse ? cb : rb)) { tr = -tr; ti = -ti; }
                const double nr = ar * tr - ai * ti, ni = ar * ti + ai * tr;
                ar = nr; ai = ni;
            }
            if (a.inverse) { ar = ar * 0.5; ai = ai * 0.5; }
        }
        if (a.conjugate) ai = -ai;
    }
    a.out[(size_t)da * n + row] = make_double2(ar, ai);
}

// ---- real and imaginary parts side by side (include/troyn.h, "Factors of the special DFT on n slots, both halves on period 2n") ------------
// Layers [first, first + count) with first + count <= log2 n taken on 2n rows are two identical n x n blocks and never the top group:
// 2^(count+1) - 1 diagonals, indices mod 2n, no entry crossing row n.  Rows < n are that table; rows >= n are the same words turned by a
// quarter, by -i in the inverse direction, (re, im) -> (im, -re), and by +i in the forward one, (re, im) -> (-im, re): a swap and one
// negation (-x, so a zero component becomes -0.0).  Absent entries stay +0 and are not turned.  No masks, no conjugate.  Same geometry,
// association and unit (-ffp-contract=off) as the sparse kernel: one thread per (diagonal, row), double2 stores coalesced along the row.
struct CkksDftFactorPackedArgs {
    const double2* roots;                 // [N] root_powers
    double2* out;                         // [nd][2n]
    double constant;
    unsigned log_n;                       // log2 N
    unsigned log_rows;                    // log2 2n, 2 <= log_rows <= log_n - 1
    unsigned first, count;                // layers [first, first + count), count >= 1, first + count <= log_rows - 1
    unsigned nd;                          // 2^(count+1) - 1
    unsigned inverse;
};

static __global__ __launch_bounds__(256) void ckks_dft_factor_packed_kernel(CkksDftFactorPackedArgs a) {
    const unsigned rows = 1u << a.log_rows;
    const unsigned row = blockIdx.x * 256u + threadIdx.x, da = blockIdx.y;
    if (row >= rows || da >= a.nd) return;
    const unsigned reach = 1u << a.count;
    const unsigned d = da < reach ? da << a.first : rows - ((a.nd - da) << a.first);
    const unsigned col = (row + d) & (rows - 1);
    const bool present = ((row ^ col) & ~((reach - 1) << a.first)) == 0;
    double ar = 0.0, ai = 0.0;
    if (present) {
        ar = a.constant;
        const unsigned j = a.inverse ? col : row;
        for (unsigned step = 0; step < a.count; step++) {
            const unsigned b = a.inverse ? a.first + a.count - 1 - step : a.first + step;
            const unsigned rb = (row >> b) & 1, cb = (col >> b) & 1;
            if (a.inverse ? rb : cb) {
                // ((-3)^j mod 4 len) (2N / 4 len) in [0, 2N): b <= log_rows - 2 <= log_n - 3
                const unsigned k = (ckks_rotation_power(j, b) & ((8u << b) - 1)) << (a.log_n - b - 2);
                const double2 r = a.roots[__brev(k & ((1u << a.log_n) - 1)) >> (32 - a.log_n)];
                double tr = r.x, ti = a.inverse ? -r.y : r.y;
                if ((k >> a.log_n) ^ (a.inverse ? cb : rb)) { tr = -tr; ti = -ti; }
                const double nr = ar * tr - ai * ti, ni = ar * ti + ai * tr;
                ar = nr; ai = ni;
            }
            if (a.inverse) { ar = ar * 0.5; ai = ai * 0.5; }
        }
        if (row >> (a.log_rows - 1)) {                                   // the lower block: times -i (inverse) / +i (forward)
            const double re = ar;
            if (a.inverse) { ar = ai; ai = -re; } else { ar = -ai; ai = re; }
        }
    }
    a.out[(size_t)da * rows + row] = make_double2(ar, ai);
}

}  // namespace troyn
