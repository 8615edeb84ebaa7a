// slot_transform.cpp -- see slot_transform.h.  Host logic only: the groups, their levels and diagonals; the factors are written and encoded on the device
// (CKKSEncoder::dft_factor_diagonals, LinearTransform's device-table path), the evaluation is Evaluator::linear_transform group by group.
#include "slot_transform.h"

#include <cmath>
#include <set>

namespace troy {

std::vector<size_t> default_layers_per_group(size_t layers, size_t at_most) {
    if (layers == 0 || at_most == 0) return {};
    const size_t groups = (layers + at_most - 1) / at_most;
    std::vector<size_t> out(groups, layers / groups);
    for (size_t i = 0; i < layers % groups; i++) out[i]++;
    return out;
}

namespace {
// the present diagonals of the layers [first, first + count) on n = 2^m slots, ascending mod n
std::vector<size_t> present_diagonals(size_t m, size_t first, size_t count) {
    const size_t n = size_t(1) << m, step = size_t(1) << first, reach = size_t(1) << count;
    std::vector<size_t> out;
    for (size_t k = 0; k < reach; k++) out.push_back(k * step);
    if (first + count < m)
        for (size_t k = reach - 1; k >= 1; k--) out.push_back(n - k * step);
    return out;
}
}  // namespace

SlotTransformPlan::SlotTransformPlan(bool coeff_to_slot, HeContextPointer context, const CKKSEncoder& encoder, const ParmsID& parms_id, double scale,
                                     std::vector<size_t> layers_per_group, double constant, MemoryPoolHandle pool, size_t n, bool packed)
    : n_(n == 0 ? encoder.slot_count() : n), slot_count_(encoder.slot_count()), packed_(packed), scale_(scale), constant_(constant) {
    const std::string P = coeff_to_slot ? "[CoeffToSlotPlan::CoeffToSlotPlan]" : "[SlotToCoeffPlan::SlotToCoeffPlan]";
    if (!context || !context->get_context_data(parms_id).has_value()) throw std::invalid_argument(P + " parms_id not valid for context.");
    ContextDataPointer cd = context->get_context_data(parms_id).value();
    if (cd->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument(P + " a CKKS context is needed.");
    if (slot_count_ < 2 || slot_count_ * 2 != cd->parms().poly_modulus_degree()) throw std::invalid_argument(P + " the encoder does not belong to the context.");
    if (n_ < 2 || (n_ & (n_ - 1)) || n_ > slot_count_) throw std::invalid_argument(P + " n must be a power of two in [2, slot_count] (0: the slot count).");
    if (!std::isfinite(constant) || constant == 0.0) throw std::invalid_argument(P + " the constant must be finite and not zero.");
    size_t m = 0;
    while ((size_t(1) << m) < n_) m++;
    layers_ = layers_per_group.empty() ? default_layers_per_group(m) : std::move(layers_per_group);
    size_t sum = 0;
    for (size_t c : layers_) {
        if (c == 0) throw std::invalid_argument(P + " a group must hold at least one layer.");
        sum += c;
    }
    if (sum != m) throw std::invalid_argument(P + " the groups must sum to log2 n layers, n the plan's number of slots.");
    const size_t groups = layers_.size();
    // packed: the group of layers [0, c) -- the last of CoeffToSlot, the first of SlotToCoeff -- works on 2n rows and must not be the boundary group
    if (packed_ && (n_ < 4 || n_ * 2 > slot_count_)) throw std::invalid_argument(P + " a packed plan needs a power of two n in [4, slot_count / 2].");
    if (packed_ && groups < 2) throw std::invalid_argument(P + " a packed plan needs at least two groups: the packed group cannot be the boundary group.");
    packed_group_ = coeff_to_slot ? groups - 1 : 0;
    for (size_t g = 0; g < groups; g++) {
        parms_ids_.push_back(cd->parms_id());
        if (!cd->next_context_data().has_value()) throw std::invalid_argument(P + " the chain has fewer levels below the operand than groups.");
        cd = cd->next_context_data().value();
    }
    boundary_ = coeff_to_slot ? 0 : groups - 1;
    const double root = std::pow(std::fabs(constant), 1.0 / static_cast<double>(groups));
    std::set<int> steps;
    rotations_ = 1;
    auto make = [&](size_t g, size_t first, int mask, bool conjugate) {
        const size_t count = layers_[g];
        const double c = (g == 0 && constant < 0) ? -root : root;
        size_t nd = 0;
        // CoeffToSlot masks the columns of its boundary group, SlotToCoeff the rows
        utils::DynamicArray table = encoder.dft_factor_diagonals(n_, first, count, coeff_to_slot, coeff_to_slot ? mask : 0, coeff_to_slot ? 0 : mask, conjugate, c, nd, pool);
        std::unique_ptr<LinearTransform> lt(new LinearTransform(context, encoder, n_, parms_ids_[g], scale_, present_diagonals(m, first, count),
                                                                LinearTransform::DeviceTable{reinterpret_cast<const double*>(table.raw_pointer())}, size_t(1) << first, pool));
        steps.insert(lt->rotation_steps().begin(), lt->rotation_steps().end());
        rotations_ += lt->rotation_steps().size();
        return lt;
    };
    // the packed group on 2n rows: both blocks from one table, rows >= n turned by -i (CoeffToSlot) / +i (SlotToCoeff); first is 0, never the top group
    auto make_packed = [&](size_t g, size_t first) {
        const size_t count = layers_[g];
        const double c = (g == 0 && constant < 0) ? -root : root;
        size_t nd = 0;
        utils::DynamicArray table = encoder.dft_factor_diagonals_packed(n_, first, count, coeff_to_slot, c, nd, pool);
        std::unique_ptr<LinearTransform> lt(new LinearTransform(context, encoder, 2 * n_, parms_ids_[g], scale_, present_diagonals(m + 1, first, count),
                                                                LinearTransform::DeviceTable{reinterpret_cast<const double*>(table.raw_pointer())}, size_t(1) << first, pool));
        steps.insert(lt->rotation_steps().begin(), lt->rotation_steps().end());
        // the conjugation of P = v + conj(v) (CoeffToSlot) / the rotation by n of V + rot_n(V) (SlotToCoeff)
        rotations_ += lt->rotation_steps().size() + 1;
        if (!coeff_to_slot) steps.insert(static_cast<int>(n_));
        return lt;
    };
    size_t done = 0;
    for (size_t g = 0; g < groups; g++) {
        done += layers_[g];
        const size_t first = coeff_to_slot ? m - done : done - layers_[g];
        firsts_.push_back(first);
        const bool boundary = g == boundary_;
        if (packed_ && g == packed_group_) { transforms_.push_back(make_packed(g, first)); continue; }
        transforms_.push_back(make(g, first, boundary ? 1 : 0, false));
        if (boundary) twin_ = make(g, first, 2, coeff_to_slot);
    }
    rotation_steps_.assign(steps.begin(), steps.end());
}

namespace {
void slot_transform(const Evaluator& ev, const HeContext& context, const char* P, bool coeff_to_slot, const Ciphertext& encrypted, const SlotTransformPlan& plan, const GaloisKeys& galois_keys,
                    Ciphertext& destination, MemoryPoolHandle pool) {
    auto cd = context.get_context_data(encrypted.parms_id());
    if (!cd.has_value()) throw std::invalid_argument(std::string(P) + " parms_id not valid for context.");
    if (cd.value()->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument(std::string(P) + " a CKKS context is needed.");
    if (cd.value()->parms().poly_modulus_degree() != 2 * plan.slot_count())
        throw std::invalid_argument(std::string(P) + " Sparse packing is a plan's own n below its slot count: the operand belongs to a ring of another degree than the plan's.");
    if (encrypted.parms_id() != plan.parms_id()) throw std::invalid_argument(std::string(P) + " the operand is not at the level of the plan.");
    Ciphertext current;
    for (size_t g = 0; g < plan.groups(); g++) {
        const Ciphertext& operand = g == 0 ? encrypted : current;
        Ciphertext next = ev.linear_transform_new(operand, plan.transform(g), galois_keys, pool);
        if (g == plan.boundary_group()) {
            // the odd half: the conjugation after the weights, where the product's scale leaves its key-switch noise negligible
            const Ciphertext odd = ev.linear_transform_new(operand, plan.twin(), galois_keys, pool);
            ev.add_inplace(next, ev.complex_conjugate_new(odd, galois_keys, pool), pool);
        }
        if (plan.packed() && g == plan.packed_group()) {
            // before the rescale, at scale * weight scale.  CoeffToSlot: v + conj(v) = [2 Re; 2 Im] on period 2n.  SlotToCoeff: V + rot_n(V) = F (a + i b) on period n
            const Ciphertext other = coeff_to_slot ? ev.complex_conjugate_new(next, galois_keys, pool) : ev.rotate_vector_new(next, static_cast<int>(plan.n()), galois_keys, pool);
            ev.add_inplace(next, other, pool);
        }
        ev.rescale_to_next_inplace(next, pool);
        current = std::move(next);
    }
    destination = std::move(current);
}
}  // namespace

void Evaluator::coeff_to_slot(const Ciphertext& encrypted, const CoeffToSlotPlan& plan, const GaloisKeys& galois_keys, Ciphertext& destination, MemoryPoolHandle pool) const {
    slot_transform(*this, *context_, "[Evaluator::coeff_to_slot]", true, encrypted, plan, galois_keys, destination, pool);
}

void Evaluator::slot_to_coeff(const Ciphertext& encrypted, const SlotToCoeffPlan& plan, const GaloisKeys& galois_keys, Ciphertext& destination, MemoryPoolHandle pool) const {
    slot_transform(*this, *context_, "[Evaluator::slot_to_coeff]", false, encrypted, plan, galois_keys, destination, pool);
}

}  // namespace troy
