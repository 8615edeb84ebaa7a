// ckks_tables.hpp -- the host tables of the CKKS canonical embedding (ckks_encoder.cu:121-183): the slot index map (Galois generator 3,
// bit-reversed) and the root powers of both FFT directions.  Plain C++, no device code: CKKSEncoder (troy/troy.cpp) and troyn_ckks_create
// (troyn.hip) both build their tables here, so the device transform reads the very doubles the host transform reads.
#pragma once
#include <cmath>
#include <complex>
#include <cstddef>
#include <vector>

namespace troyn {
namespace ckks_tables {

inline size_t reverse_bits(size_t x, size_t bits) {
    size_t r = 0;
    for (size_t i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}

// n = 2^log_n >= 4.  index_map[i] / index_map[i + n/2]: the position of slot i / of its conjugate.
// psi = exp(2 pi i / 2n); root_powers[i] = psi^bitrev(i), inv_root_powers[i] = conj(psi^(bitrev(i-1)+1)); entry 0 of both is zero.
template <typename Index>
inline void build(size_t log_n, std::vector<Index>& index_map, std::vector<std::complex<double>>& root_powers,
                  std::vector<std::complex<double>>& inv_root_powers) {
    const size_t n = size_t(1) << log_n, slots = n >> 1, m = n << 1;
    index_map.resize(n);
    size_t pos = 1;
    for (size_t i = 0; i < slots; i++) {
        index_map[i] = static_cast<Index>(reverse_bits((pos - 1) >> 1, log_n));
        index_map[i + slots] = static_cast<Index>(reverse_bits((m - pos - 1) >> 1, log_n));
        pos = (pos * 3) & (m - 1);
    }
    const double pi = 3.14159265358979323846264338327950288;
    auto root = [&](size_t k) { const double ang = 2.0 * pi * static_cast<double>(k % m) / static_cast<double>(m); return std::complex<double>(std::cos(ang), std::sin(ang)); };
    root_powers.assign(n, {0, 0});
    inv_root_powers.assign(n, {0, 0});
    for (size_t i = 1; i < n; i++) {
        root_powers[i] = root(reverse_bits(i, log_n));
        inv_root_powers[i] = std::conj(root(reverse_bits(i - 1, log_n) + 1));
    }
}

}  // namespace ckks_tables
}  // namespace troyn
