// linear_transform.cpp -- see linear_transform.h.  Host logic only: the split of the diagonals into baby and giant steps; the encoding is one call of the
// device encoder, the evaluation the Evaluator's BSGS methods.
#include "linear_transform.h"

#include <algorithm>
#include <set>

namespace troy {

namespace {
const char* const LT = "[LinearTransform::LinearTransform]";
}

LinearTransform::LinearTransform(HeContextPointer context, const CKKSEncoder& encoder, size_t n, const ParmsID& parms_id, double scale, const Diagonals& diagonals,
                                 size_t baby_count, MemoryPoolHandle pool)
    : n_(n), n1_(baby_count), parms_id_(parms_id), scale_(scale) {
    if (diagonals.empty()) throw std::invalid_argument(std::string(LT) + " no diagonals.");
    std::vector<size_t> present;
    std::vector<std::complex<double>> source;                       // [present][n], ascending diagonal index (the map's order)
    for (const auto& kv : diagonals) {
        if (kv.first >= n) throw std::invalid_argument(std::string(LT) + " diagonal index must be below n.");
        if (kv.second.size() != n) throw std::invalid_argument(std::string(LT) + " a diagonal must hold n values.");
        present.push_back(kv.first);
        source.insert(source.end(), kv.second.begin(), kv.second.end());
    }
    build(context, encoder, present, source.data(), false, pool);
}

LinearTransform::LinearTransform(HeContextPointer context, const CKKSEncoder& encoder, size_t n, const ParmsID& parms_id, double scale,
                                 const std::vector<std::complex<double>>& matrix, size_t baby_count, MemoryPoolHandle pool)
    : n_(n), n1_(baby_count), parms_id_(parms_id), scale_(scale) {
    if (n == 0 || matrix.size() != n * n) throw std::invalid_argument(std::string(LT) + " the matrix must hold n * n values.");
    std::vector<size_t> present(n);
    for (size_t k = 0; k < n; k++) present[k] = k;
    build(context, encoder, present, matrix.data(), true, pool);
}

LinearTransform::LinearTransform(HeContextPointer context, const CKKSEncoder& encoder, size_t n, const ParmsID& parms_id, double scale, const std::vector<size_t>& present,
                                 DeviceTable table, size_t baby_count, MemoryPoolHandle pool)
    : n_(n), n1_(baby_count), parms_id_(parms_id), scale_(scale) {
    if (present.empty() || !table.diagonals) throw std::invalid_argument(std::string(LT) + " no diagonals.");
    build(context, encoder, present, nullptr, false, pool, table.diagonals);
}

void LinearTransform::build(HeContextPointer context, const CKKSEncoder& encoder, const std::vector<size_t>& present, const std::complex<double>* source, bool matrix,
                            MemoryPoolHandle pool, const double* device_source) {
    if (!context || !context->get_context_data(parms_id_).has_value()) throw std::invalid_argument(std::string(LT) + " parms_id not valid for context.");
    if (context->get_context_data(parms_id_).value()->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument(std::string(LT) + " a CKKS context is needed.");
    const size_t slots = encoder.slot_count();
    if (n_ == 0 || (n_ & (n_ - 1)) || n_ > slots || slots % n_) throw std::invalid_argument(std::string(LT) + " n must be a power of two that divides the slot count.");
    if (n1_ == 0) { n1_ = 1; while (n1_ * n1_ < n_) n1_ <<= 1; }
    if ((n1_ & (n1_ - 1)) || n1_ > n_) throw std::invalid_argument(std::string(LT) + " baby_count must be a power of two of at most n.");
    std::set<size_t> babies, giants;
    for (size_t k : present) { babies.insert(k % n1_); giants.insert(k - k % n1_); }
    baby_steps_.assign(babies.begin(), babies.end());
    giant_steps_.assign(giants.begin(), giants.end());
    std::set<int> steps(baby_steps_.begin(), baby_steps_.end());
    steps.insert(giant_steps_.begin(), giant_steps_.end());
    steps.erase(0);
    rotation_steps_.assign(steps.begin(), steps.end());
    // one item per present (giant, baby): (row of the source, shift = the giant step)
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    std::vector<std::pair<size_t, size_t>> where;
    for (size_t g = 0; g < giant_steps_.size(); g++)
        for (size_t b = 0; b < baby_steps_.size(); b++) {
            const size_t k = static_cast<size_t>(giant_steps_[g]) + static_cast<size_t>(baby_steps_[b]);
            const auto at = std::lower_bound(present.begin(), present.end(), k);
            if (at == present.end() || *at != k) continue;
            pairs.emplace_back(static_cast<uint32_t>(matrix ? k : static_cast<size_t>(at - present.begin())), static_cast<uint32_t>(giant_steps_[g]));
            where.emplace_back(g, b);
        }
    weights_ = device_source ? encoder.encode_device_diagonals_new(device_source, n_, present.size(), pairs, context->key_parms_id(), scale_, pool)
                             : encoder.encode_diagonals_new(source, matrix, n_, present.size(), pairs, context->key_parms_id(), scale_, pool);
    rows_.assign(giant_steps_.size(), WeightRow(baby_steps_.size(), nullptr));
    for (size_t i = 0; i < where.size(); i++) rows_[where[i].first][where[i].second] = &weights_[i];
}

namespace {
void linear_transform_check(const HeContext& context, const Ciphertext& encrypted, const LinearTransform& lt) {
    const char* P = "[Evaluator::linear_transform]";
    auto cd = context.get_context_data(encrypted.parms_id());
    if (!cd.has_value()) throw std::invalid_argument(std::string(P) + " parms_id not valid for context.");
    if (cd.value()->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument(std::string(P) + " a CKKS context is needed.");
    const size_t slots = cd.value()->parms().poly_modulus_degree() / 2;
    if (lt.n() == 0 || slots % lt.n()) throw std::invalid_argument(std::string(P) + " the size of the transform does not divide the slot count.");
    if (encrypted.parms_id() != lt.parms_id()) throw std::invalid_argument(std::string(P) + " the operand is not at the level of the transform.");
}
}  // namespace

void Evaluator::linear_transform(const Ciphertext& encrypted, const LinearTransform& lt, const GaloisKeys& galois_keys, Ciphertext& destination,
                                 MemoryPoolHandle pool) const {
    linear_transform_check(*context_, encrypted, lt);
    rotate_bsgs_sum_double_hoisted(encrypted, lt.baby_steps(), lt.giant_steps(), galois_keys, lt.weights(), destination, pool);
}

void Evaluator::linear_transform_single_hoisted(const Ciphertext& encrypted, const LinearTransform& lt, const GaloisKeys& galois_keys, Ciphertext& destination,
                                                MemoryPoolHandle pool) const {
    linear_transform_check(*context_, encrypted, lt);
    rotate_bsgs_sum(encrypted, lt.baby_steps(), lt.giant_steps(), galois_keys, lt.weights(), destination, pool);
}

}  // namespace troy
