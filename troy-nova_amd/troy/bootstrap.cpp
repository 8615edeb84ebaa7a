// bootstrap.cpp -- see bootstrap.h.  Host logic only: the levels, scales and constants of the chain; the device work is the stages' own
// (Evaluator::mod_raise, coeff_to_slot, eval_mod_batched, slot_to_coeff) and the two streaming kernels behind split_real_imag / join_real_imag.
#include "bootstrap.h"

#include <algorithm>
#include <cmath>
#include <set>

#include "device_steps.h"

namespace troy {

namespace {
size_t log2_of(size_t n) { size_t m = 0; while ((size_t(1) << m) < n) m++; return m; }
}  // namespace

BootstrapPlan::BootstrapPlan(HeContextPointer context, const CKKSEncoder& encoder, double message_scale, double half_width, size_t degree, size_t double_angles,
                             std::vector<size_t> coeff_to_slot_layers, std::vector<size_t> slot_to_coeff_layers, double weight_scale, MemoryPoolHandle pool, size_t n,
                             size_t sub_sum_radix, bool packed)
    : message_scale_(message_scale), half_width_(half_width), degree_(degree), double_angles_(double_angles) {
    const std::string P = "[BootstrapPlan::BootstrapPlan]";
    if (!context || !context->first_context_data().has_value()) throw std::invalid_argument(P + " the context has no parameters.");
    ContextDataPointer first = context->first_context_data().value();
    if (first->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument(P + " a CKKS context is needed.");
    if (!(half_width > 0.0) || !std::isfinite(half_width)) throw std::invalid_argument(P + " the half width K must be positive and finite.");
    if (degree < 1 || degree > 127) throw std::invalid_argument(P + " the degree must be in 1 .. 127.");
    if (double_angles > 16) throw std::invalid_argument(P + " more than 16 double_angles.");
    if (!(message_scale > 0.0) || !std::isfinite(message_scale)) throw std::invalid_argument(P + " the message scale must be positive and finite.");
    if (!(weight_scale > 0.0) || !std::isfinite(weight_scale)) throw std::invalid_argument(P + " the weight scale must be positive and finite.");
    const auto& primes = first->parms().coeff_modulus();
    const size_t Ld = primes.size();
    auto prime = [&](size_t i) { return static_cast<double>(primes[i].value()); };
    q0_ = prime(0);
    if (q0_ / message_scale < 2.0) throw std::invalid_argument(P + " q0 / message_scale must be at least 2.");
    const size_t slot_count = encoder.slot_count(), slots = n == 0 ? slot_count : n;
    if (slots < 2 || (slots & (slots - 1)) || slots > slot_count) throw std::invalid_argument(P + " n must be a power of two in [2, slot_count] (0: the slot count).");
    if (sub_sum_radix != 0 && (sub_sum_radix < 2 || (sub_sum_radix & (sub_sum_radix - 1)))) throw std::invalid_argument(P + " sub_sum_radix must be 0 or a power of two >= 2.");
    sub_sum_radix_ = sub_sum_radix == 0 ? 4 : sub_sum_radix;
    const double sub_sum_factor = static_cast<double>(slot_count / slots);      // s, a power of two: dividing by it is exact
    // packed: both halves in one ciphertext of period 2n; the slot plans refuse a single group
    if (packed && (slots < 4 || slots * 2 > slot_count)) throw std::invalid_argument(P + " a packed plan needs a power of two n in [4, slot_count / 2].");
    const size_t m = log2_of(slots);
    const size_t gc = coeff_to_slot_layers.empty() ? default_layers_per_group(m).size() : coeff_to_slot_layers.size();
    const size_t gs = slot_to_coeff_layers.empty() ? default_layers_per_group(m).size() : slot_to_coeff_layers.size();
    eval_mod_depth_ = Evaluator::chebyshev_depth(degree) + double_angles;
    const size_t levels = gc + eval_mod_depth_ + gs;
    if (Ld < levels + 1)
        throw std::invalid_argument(P + " the chain has " + std::to_string(Ld) + " data levels, the bootstrap needs " + std::to_string(levels + 1) + " (levels() + 1).");
    // the scales as the evaluator will track them (bootstrap.h, steps 3 to 8)
    const size_t L1 = Ld - gc, L2 = L1 - eval_mod_depth_, L3 = L2 - gs;
    double s1 = q0_;
    for (size_t g = 0; g < gc; g++) s1 = s1 * weight_scale / prime(Ld - 1 - g);
    const double c1 = prime(L1 - 1) / (2.0 * half_width * s1);              // the slots read s x after sub_sum: the plan's constant is c1 / s
    double s = (s1 * (2.0 * c1)) * half_width;                      // EvalMod's working scale, q_w up to rounding
    const size_t cheb = eval_mod_depth_ - double_angles;
    for (size_t i = 0; i < double_angles; i++) s = s * s / prime(L1 - cheb - 1 - i);
    s *= 2.0 * 3.14159265358979323846;
    for (size_t g = 0; g < gs; g++) s = s * weight_scale / prime(L2 - 1 - g);
    const double c2 = q0_ / s;
    ContextDataPointer cd = first;
    for (size_t i = 0; i < L1 - L2 + gc; i++) cd = cd->next_context_data().value();
    coeff_to_slot_.reset(new CoeffToSlotPlan(context, encoder, first->parms_id(), weight_scale, std::move(coeff_to_slot_layers), c1 / sub_sum_factor, pool, slots, packed));
    slot_to_coeff_.reset(new SlotToCoeffPlan(context, encoder, cd->parms_id(), weight_scale, std::move(slot_to_coeff_layers), c2, pool, slots, packed));
    for (size_t i = 0; i < L2 - L3; i++) cd = cd->next_context_data().value();
    output_parms_id_ = cd->parms_id();
    std::set<int> steps{0};
    steps.insert(coeff_to_slot_->rotation_steps().begin(), coeff_to_slot_->rotation_steps().end());
    steps.insert(slot_to_coeff_->rotation_steps().begin(), slot_to_coeff_->rotation_steps().end());
    for (const std::vector<int>& stage : Evaluator::sub_sum_stages(slot_count, slots, sub_sum_radix_)) {
        steps.insert(stage.begin(), stage.end());
        sub_sum_key_switches_ += stage.size();
    }
    rotation_steps_.assign(steps.begin(), steps.end());
}

std::vector<std::vector<int>> Evaluator::sub_sum_stages(size_t slot_count, size_t n, size_t radix) {
    const std::string P = "[Evaluator::sub_sum]";
    if (slot_count < 2 || (slot_count & (slot_count - 1))) throw std::invalid_argument(P + " the slot count must be a power of two >= 2.");
    if (n < 2 || (n & (n - 1)) || n > slot_count) throw std::invalid_argument(P + " n must be a power of two in [2, slot_count].");
    if (radix != 0 && (radix < 2 || (radix & (radix - 1)))) throw std::invalid_argument(P + " the radix must be 0 or a power of two >= 2.");
    if (radix == 0) radix = 4;
    std::vector<std::vector<int>> stages;
    // PROD_i (1 + rot_{n 2^i}): a stage of R terms from `step` is SUM_{i < R} rot_{i step}; the last one takes what remains
    for (size_t step = n; step < slot_count;) {
        const size_t terms = std::min(radix, slot_count / step);
        std::vector<int> stage;
        for (size_t i = 1; i < terms; i++) stage.push_back(static_cast<int>(i * step));
        stages.push_back(std::move(stage));
        step *= terms;
    }
    return stages;
}

std::vector<int> Evaluator::sub_sum_steps(size_t slot_count, size_t n, size_t radix) {
    std::set<int> steps;
    for (const std::vector<int>& stage : sub_sum_stages(slot_count, n, radix)) steps.insert(stage.begin(), stage.end());
    return std::vector<int>(steps.begin(), steps.end());
}

void Evaluator::sub_sum(const Ciphertext& encrypted, size_t n, const GaloisKeys& galois_keys, Ciphertext& destination, size_t radix, MemoryPoolHandle pool) const {
    const std::string P = "[Evaluator::sub_sum]";
    auto cd = context_->get_context_data(encrypted.parms_id());
    if (!cd.has_value()) throw std::invalid_argument(P + " parms_id not valid for context.");
    if (cd.value()->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument(P + " a CKKS context is needed.");
    const std::vector<std::vector<int>> stages = sub_sum_stages(cd.value()->parms().poly_modulus_degree() / 2, n, radix);
    if (stages.empty()) {                                             // n = slot_count: the identity, no key touched
        if (&destination != &encrypted) destination = encrypted.clone(pool);
        return;
    }
    Ciphertext current;
    const Ciphertext* operand = &encrypted;
    for (const std::vector<int>& stage : stages) {
        Ciphertext next = rotate_sum_new(*operand, stage, galois_keys, pool);     // hoisted: one decomposition, one division
        add_inplace(next, *operand, pool);
        current = std::move(next);
        operand = &current;
    }
    destination = std::move(current);
}

void Evaluator::split_real_imag(const Ciphertext& encrypted, const GaloisKeys& galois_keys, Ciphertext& real2, Ciphertext& imag2_alt, MemoryPoolHandle pool) const {
    const std::string P = "[Evaluator::split_real_imag]";
    if (context_->key_context_data().value()->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument(P + " CKKS only.");
    if (!encrypted.is_ntt_form()) throw std::invalid_argument(P + " Ciphertext must be in NTT form.");
    if (encrypted.polynomial_count() != 2) throw std::invalid_argument(P + " The ciphertext must have two polynomials.");
    const Ciphertext conjugate = complex_conjugate_new(encrypted, galois_keys, pool);      // its refusals: keys, seed, device, parms_id
    Ciphertext s = Ciphertext::like(encrypted, false, pool), d = Ciphertext::like(encrypted, false, pool);
    detail::ckks_complex_split_step(detail::on_current_stream(pool), context_->plan(), static_cast<uint32_t>(encrypted.coeff_modulus_size()), encrypted.data().raw_pointer(),
                                    conjugate.data().raw_pointer(), s.data().raw_pointer(), d.data().raw_pointer(), 1);
    real2 = std::move(s);
    imag2_alt = std::move(d);
}

void Evaluator::join_real_imag(const Ciphertext& real, const Ciphertext& imag_alt, Ciphertext& destination, MemoryPoolHandle pool) const {
    const std::string P = "[Evaluator::join_real_imag]";
    if (context_->key_context_data().value()->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument(P + " CKKS only.");
    for (const Ciphertext* c : {&real, &imag_alt}) {
        if (c->contains_seed()) throw std::invalid_argument(P + " Argument contains seed.");
        if (!context_->on_device() || !c->on_device()) throw std::invalid_argument(P + " Operands must be on the device (the evaluator runs on the GPU only).");
        if (!c->is_ntt_form()) throw std::invalid_argument(P + " Ciphertext must be in NTT form.");
        if (c->polynomial_count() != 2) throw std::invalid_argument(P + " The ciphertext must have two polynomials.");
    }
    if (!context_->get_context_data(real.parms_id()).has_value()) throw std::invalid_argument(P + " ParmsID is not valid for the current context.");
    if (real.parms_id() != imag_alt.parms_id()) throw std::invalid_argument(P + " Operands have different parms_id.");
    if (!detail::scales_are_close(real.scale(), imag_alt.scale())) throw std::invalid_argument(P + " Operands have different scales.");
    Ciphertext out = Ciphertext::like(real, false, pool);
    detail::ckks_complex_join_step(detail::on_current_stream(pool), context_->plan(), static_cast<uint32_t>(real.coeff_modulus_size()), real.data().raw_pointer(),
                                   imag_alt.data().raw_pointer(), out.data().raw_pointer(), 1);
    destination = std::move(out);
}

double BootstrapPlan::half_width_for(size_t hamming_weight) { return 1.0 + 6.5 * std::sqrt((static_cast<double>(hamming_weight) + 1.0) / 12.0); }

void Evaluator::bootstrap_checks(const Ciphertext& encrypted, const BootstrapPlan& plan) const {
    const std::string P = "[Evaluator::bootstrap]";
    if (context_->key_context_data().value()->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument(P + " CKKS only.");
    if (!encrypted.is_ntt_form()) throw std::invalid_argument(P + " Ciphertext must be in NTT form.");
    if (encrypted.polynomial_count() != 2) throw std::invalid_argument(P + " The ciphertext must have two polynomials.");
    if (!detail::scales_are_close(encrypted.scale(), plan.message_scale())) throw std::invalid_argument(P + " The operand's scale is not the plan's message scale.");
}

void Evaluator::bootstrap(const Ciphertext& encrypted, const BootstrapPlan& plan, const RelinKeys& relin_keys, const GaloisKeys& galois_keys, Ciphertext& destination,
                          MemoryPoolHandle pool) const {
    bootstrap_checks(encrypted, plan);
    // 1. the last level: one prime, q0
    Ciphertext low;
    const Ciphertext* exhausted = &encrypted;
    if (encrypted.parms_id() != context_->last_parms_id()) { mod_switch_to(encrypted, context_->last_parms_id(), low, pool); exhausted = &low; }
    // 2. to the top: t = D m + q0 I;  2b (in bootstrap_raised). a sparse plan keeps the Y-part of t, s times
    bootstrap_raised(mod_raise_new(*exhausted, std::nullopt, pool), plan, relin_keys, galois_keys, destination, pool);
}

void Evaluator::bootstrap(const Ciphertext& encrypted, const BootstrapPlan& plan, const RelinKeys& relin_keys, const GaloisKeys& galois_keys,
                          const SparseEncapsulationKeys& encapsulation_keys, Ciphertext& destination, MemoryPoolHandle pool) const {
    const std::string P = "[Evaluator::bootstrap]";
    bootstrap_checks(encrypted, plan);
    for (const KSwitchKeys* k : {&encapsulation_keys.to_sparse, &encapsulation_keys.to_dense}) {
        if (k->data().size() != 1 || k->data()[0].empty()) throw std::invalid_argument(P + " The sparse encapsulation keys are empty.");
        if (k->parms_id() != context_->key_parms_id()) throw std::invalid_argument(P + " The sparse encapsulation keys have another key parms_id than the context.");
    }
    // 1. the last level: one prime, q0;  1a. to the sparse secret there, where to_sparse has its rows
    Ciphertext low;
    const Ciphertext* exhausted = &encrypted;
    if (encrypted.parms_id() != context_->last_parms_id()) { mod_switch_to(encrypted, context_->last_parms_id(), low, pool); exhausted = &low; }
    const Ciphertext sparse = apply_keyswitching_new(*exhausted, encapsulation_keys.to_sparse, pool);
    // 2. to the top under the sparse secret: t = D m + q0 I with I from s';  2a. back to the evaluation secret
    const Ciphertext raised = mod_raise_new(sparse, std::nullopt, pool);
    bootstrap_raised(apply_keyswitching_new(raised, encapsulation_keys.to_dense, pool), plan, relin_keys, galois_keys, destination, pool);
}

void Evaluator::bootstrap_raised(Ciphertext&& raised, const BootstrapPlan& plan, const RelinKeys& relin_keys, const GaloisKeys& galois_keys, Ciphertext& destination,
                                 MemoryPoolHandle pool) const {
    const std::string P = "[Evaluator::bootstrap]";
    // 2b. sparse packing: s (D p(Y) + q0 I'(Y)), a polynomial in Y = X^s whose slots repeat with period n
    if (plan.n() != plan.slot_count()) sub_sum(raised, plan.n(), galois_keys, raised, plan.sub_sum_radix(), pool);
    // 3. the coefficients read t / q0 = D m / q0 + I (s times that for a sparse plan)
    raised.scale() = plan.q0();
    // 4, 5. slots c1 BR(x_k + i x_{k+n}); their parts 2 c1 Re, (-1)^j 2 c1 Im relabelled to read Re, (-1)^j Im
    Ciphertext slots = coeff_to_slot_new(raised, plan.coeff_to_slot_plan(), galois_keys, pool);
    if (plan.packed()) {
        // 5'. a packed plan's slots already read [2 c1 Re; 2 c1 Im] on period 2n: the same relabel, no split, no sign
        slots.scale() = slots.scale() * (2.0 * plan.coeff_to_slot_constant() * plan.sub_sum_factor());
        // 6'. EvalMod once, on both halves side by side;  8', 9. SlotToCoeff's packed group adds the halves as a + i b
        std::vector<Ciphertext> reduced;
        eval_mod_batched({&slots}, relin_keys, plan.half_width(), plan.degree(), plan.double_angles(), reduced, pool, "[Evaluator::bootstrap]");
        Ciphertext out = slot_to_coeff_new(reduced[0], plan.slot_to_coeff_plan(), galois_keys, pool);
        if (std::fabs(out.scale() * plan.slot_to_coeff_constant() / plan.q0() - 1.0) > 1e-9)
            throw std::logic_error(P + " the tracked scale does not match the plan's constants.");
        out.scale() = plan.output_scale();
        destination = std::move(out);
        return;
    }
    Ciphertext re, im;
    split_real_imag(slots, galois_keys, re, im, pool);
    const double part_scale = slots.scale() * (2.0 * plan.coeff_to_slot_constant() * plan.sub_sum_factor());      // s = 1 for a full plan: exact
    re.scale() = part_scale; im.scale() = part_scale;
    // 6, 7. sin(2 pi x) / (2 pi) on both halves in one schedule, then Re' + i Im'
    std::vector<Ciphertext> reduced;
    eval_mod_batched({&re, &im}, relin_keys, plan.half_width(), plan.degree(), plan.double_angles(), reduced, pool, "[Evaluator::bootstrap]");
    const Ciphertext joined = join_real_imag_new(reduced[0], reduced[1], pool);
    // 8, 9. back to coefficients with c2 = q0 / (tracked scale): the payload is D z
    Ciphertext out = slot_to_coeff_new(joined, plan.slot_to_coeff_plan(), galois_keys, pool);
    // the plan computed c2 from the scales it expected the stages to track: a stage that tracks another scale would shift the message by a constant factor
    if (std::fabs(out.scale() * plan.slot_to_coeff_constant() / plan.q0() - 1.0) > 1e-9)
        throw std::logic_error(P + " the tracked scale does not match the plan's constants.");
    out.scale() = plan.output_scale();
    destination = std::move(out);
}

}  // namespace troy
