// The Evaluator's x_batched(vector<const T*>, vector<T*>, pool) forms (evaluator.h; batch_utils.h in the reference).
//
// The reference builds device arrays of slice pointers per call and lets every kernel thread loop over the batch.  Here a
// uniform batch is ONE contiguous block [count][polys][limbs][N]: scattered operands are staged by a single gather launch
// (operands that are already adjacent windows of one buffer -- which is what these functions return -- are used in place),
// the C-ABI entry runs once with batch = count, and the results are windows of one shared buffer.  The operation's *_prepare
// runs on item 0: it performs every argument check of the reference and fixes the result's shape and metadata without device work; the
// device work is the operation's step (device_steps.h) with batch = count.
#include <hip/hip_runtime.h>

#include "troy.h"
#include "device_steps.h"

namespace troy {

namespace {

using detail::hip_check;
using CVec = std::vector<const Ciphertext*>;
using Vec = std::vector<Ciphertext*>;

// same level, shape, form and scale as item 0, on the device, no seed
bool uniform(const CVec& v) {
    if (v.empty()) return false;
    const Ciphertext& a = *v[0];
    for (const Ciphertext* c : v)
        if (!c->on_device() || c->contains_seed() || c->parms_id() != a.parms_id() || c->polynomial_count() != a.polynomial_count() ||
            c->coeff_modulus_size() != a.coeff_modulus_size() || c->is_ntt_form() != a.is_ntt_form() || c->scale() != a.scale() ||
            c->correction_factor() != a.correction_factor() || c->data().size() != a.data().size())
            return false;
    return true;
}

CVec as_const(const Vec& v) { return CVec(v.begin(), v.end()); }

void same_size(const char* prompt, size_t a, size_t b) {
    if (a != b) throw std::invalid_argument(std::string(prompt) + " Input and destination have different sizes.");
}

// The one shape of every x_batched form.  Sizes agree; a batch at or above the threshold whose operand vectors are uniform and that passes
// the operation's own `batchable` runs as ONE device step: `prepare` shapes the result of item 0 (checks + metadata, no device work), the
// operands are staged as [count][words] (used in place when they are adjacent windows already), `step` gets the staged operands and a
// block of count results, and the destinations become windows of that block.  Any other batch goes through `each` object by object
// (into a temporary, so that in-place calls work).  `threshold`: the reference's BATCH_OP_THRESHOLD; an addition that promises one call for any count passes 1.
template <typename Batchable, typename Each, typename Prepare, typename Step>
void run_batched(const char* prompt, std::initializer_list<const CVec*> operands, const Vec& destination, MemoryPoolHandle pool, Batchable batchable, Each each,
                 Prepare prepare, Step step, size_t threshold = Evaluator::BATCH_OP_THRESHOLD) {
    const size_t count = destination.size();
    for (const CVec* v : operands) same_size(prompt, v->size(), count);
    bool batched = count >= threshold;
    for (const CVec* v : operands) batched = batched && uniform(*v);
    if (!batched || !batchable()) {
        for (size_t i = 0; i < count; i++) { Ciphertext out; each(i, out); *destination[i] = std::move(out); }
        return;
    }
    Ciphertext proto;
    prepare(proto);
    const detail::StepEnv env = detail::on_current_stream(pool);
    utils::DynamicArray staged[2], table;
    const uint64_t* in[2] = {nullptr, nullptr};
    size_t k = 0;
    for (const CVec* v : operands) {
        std::vector<const uint64_t*> src(count);
        for (size_t i = 0; i < count; i++) src[i] = (*v)[i]->data().raw_pointer();
        in[k] = detail::stage(env, src, (*v)[0]->data().size(), staged[k], table);
        k++;
    }
    const size_t words = proto.polynomial_count() * proto.coeff_modulus_size() * proto.poly_modulus_degree();
    auto block = std::make_shared<utils::DynamicArray>(count * words, true, pool);
    step(env, proto, in[0], in[1], block->raw_pointer(), count);
    // no synchronisation: the call is asynchronous on the thread's stream like the reference's evaluator methods; what the step took from the pool returns
    // to it, and the pool hands a block back to the thread that released it in stream order and to any other thread only after a device synchronisation
    // (MemoryPool).  "In stream order" holds by construction: every launch of this mirror goes to the calling thread's stream (with call combining on, to
    // the one shared stream, and the pool then treats every thread as the same owner).
    for (size_t i = 0; i < count; i++)
        *destination[i] = Ciphertext::from_members(proto.polynomial_count(), proto.coeff_modulus_size(), proto.poly_modulus_degree(), proto.parms_id(), proto.scale(),
                                                   proto.is_ntt_form(), proto.correction_factor(), 0,
                                                   utils::DynamicArray::device_view(block->raw_pointer() + i * words, words, block));
}

const auto always = [] { return true; };

}  // namespace

// -- negate ------------------------------------------------------------------------------------------------------------
void Evaluator::negate_batched(const CVec& encrypted, const Vec& destination, MemoryPoolHandle pool) const {
    run_batched("[Evaluator::negate_batched]", {&encrypted}, destination, pool, always,
        [&](size_t i, Ciphertext& out) { negate(*encrypted[i], out, pool); },
        [&](Ciphertext& proto) { negate_prepare(*encrypted[0], proto, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            detail::negate_step(env, context_->plan(), static_cast<uint32_t>(proto.coeff_modulus_size()), in, out, count * proto.polynomial_count());
        });
}

void Evaluator::negate_inplace_batched(const Vec& encrypted, MemoryPoolHandle pool) const { negate_batched(as_const(encrypted), encrypted, pool); }

// -- add / sub ---------------------------------------------------------------------------------------------------------
void Evaluator::translate_batched(const CVec& e1, const CVec& e2, const Vec& d, bool subtract, MemoryPoolHandle pool) const {
    run_batched("[Evaluator::translate_batched]", {&e1, &e2}, d, pool,
        // BGV operands with different factors are balanced one by one
        [&] { return e1[0]->polynomial_count() == e2[0]->polynomial_count() && e1[0]->correction_factor() == e2[0]->correction_factor(); },
        [&](size_t i, Ciphertext& out) { translate(*e1[i], *e2[i], out, subtract, pool); },
        [&](Ciphertext& proto) { translate_prepare(*e1[0], *e2[0], proto, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count) {
            detail::add_sub_step(env, context_->plan(), static_cast<uint32_t>(proto.coeff_modulus_size()), subtract, a, b, out, count * proto.polynomial_count());
        });
}

void Evaluator::add_batched(const CVec& e1, const CVec& e2, const Vec& d, MemoryPoolHandle pool) const { translate_batched(e1, e2, d, false, pool); }
void Evaluator::sub_batched(const CVec& e1, const CVec& e2, const Vec& d, MemoryPoolHandle pool) const { translate_batched(e1, e2, d, true, pool); }

// -- multiply ----------------------------------------------------------------------------------------------------------
void Evaluator::multiply_batched(const CVec& e1, const CVec& e2, const Vec& d, MemoryPoolHandle pool) const {
    run_batched("[Evaluator::multiply_batched]", {&e1, &e2}, d, pool, always,
        [&](size_t i, Ciphertext& out) { multiply(*e1[i], *e2[i], out, pool); },
        [&](Ciphertext& proto) { multiply_prepare(*e1[0], *e2[0], proto, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count) {
            const size_t p1 = e1[0]->polynomial_count(), p2 = e2[0]->polynomial_count();
            const uint32_t L = static_cast<uint32_t>(proto.coeff_modulus_size());
            if (context_->key_context_data().value()->parms().scheme() == SchemeType::BFV) detail::multiply_bfv_step(env, context_->behz(L), a, p1, b, p2, out, count);
            else detail::multiply_dyadic_step(env, context_->plan(), L, a, p1, b, p2, out, count);
        });
}

// -- multiply -> relinearize -> rescale_to_next, one call for the whole batch (addition) ------------------------------------------------
void Evaluator::multiply_relinearize_rescale_batched(const CVec& e1, const CVec& e2, const RelinKeys& relin_keys, const Vec& destination, MemoryPoolHandle pool) const {
    uint32_t L = 0; ParmsID next; double scale = 1.0; std::vector<const uint64_t*> keys;
    run_batched("[Evaluator::multiply_relinearize_rescale_batched]", {&e1, &e2}, destination, pool,
        [&] { return multiply_relinearize_rescale_prepare(*e1[0], *e2[0], relin_keys, L, next, scale, keys); },   // item 0 stands for every item of a uniform batch
        [&](size_t i, Ciphertext& out) { multiply_relinearize_rescale(*e1[i], *e2[i], relin_keys, out, pool); },
        [&](Ciphertext& proto) {
            proto = Ciphertext::like(*e1[0], 2, L - 1, false, pool);
            proto.parms_id() = next; proto.scale() = scale; proto.is_ntt_form() = true;
        },
        [&](const detail::StepEnv& env, const Ciphertext&, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count) {
            detail::multiply_relinearize_rescale_step(env, context_->plan(), L, a, b, keys.data(), out, count);
        });
}

// -- multiply -> relinearize -> mod_switch_to_next, BGV, one call for the whole batch (addition) -----------------------------------------
void Evaluator::multiply_relinearize_mod_switch_batched(const CVec& e1, const CVec& e2, const RelinKeys& relin_keys, const Vec& destination, MemoryPoolHandle pool) const {
    std::vector<const uint64_t*> keys;
    run_batched("[Evaluator::multiply_relinearize_mod_switch_batched]", {&e1, &e2}, destination, pool, always,
        [&](size_t i, Ciphertext& out) { multiply_relinearize_mod_switch(*e1[i], *e2[i], relin_keys, out, pool); },
        [&](Ciphertext& proto) { multiply_relinearize_mod_switch_prepare(*e1[0], *e2[0], relin_keys, proto, keys, pool); },   // item 0 stands for every item of a uniform batch
        [&](const detail::StepEnv& env, const Ciphertext&, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count) {
            const size_t L = e1[0]->coeff_modulus_size();
            detail::bgv_multiply_relinearize_mod_switch_step(env, key_level_bgv(SchemeType::BGV), context_->bgv(L), static_cast<uint32_t>(L), a, b, keys.data(), out, count);
        }, 1);
}

// -- relinearize -------------------------------------------------------------------------------------------------------
void Evaluator::relinearize_batched(const CVec& encrypted, const RelinKeys& relin_keys, const Vec& d, MemoryPoolHandle pool) const {
    const SchemeType scheme = context_->key_context_data().value()->parms().scheme();
    std::vector<const uint64_t*> keys;
    run_batched("[Evaluator::relinearize_batched]", {&encrypted}, d, pool,
        [&] { return scheme != SchemeType::BGV && encrypted[0]->polynomial_count() == 3; },   // BGV (ski_util5 tail): per-object path
        [&](size_t i, Ciphertext& out) { relinearize_internal(*encrypted[i], relin_keys, 2, out, pool); },
        [&](Ciphertext& proto) { relinearize_prepare(*encrypted[0], relin_keys, proto, keys, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            detail::relinearize_step(env, context_->plan(), nullptr, static_cast<uint32_t>(proto.coeff_modulus_size()), scheme == SchemeType::CKKS, proto.is_ntt_form(), in,
                                     keys.data(), out, count);
        });
}

// -- modulus switching -------------------------------------------------------------------------------------------------
void Evaluator::mod_switch_to_next_batched(const CVec& encrypted, const Vec& destination, MemoryPoolHandle pool) const {
    SchemeType scheme = context_->key_context_data().value()->parms().scheme();
    run_batched("[Evaluator::mod_switch_to_next_batched]", {&encrypted}, destination, pool,
        [&] { return scheme != SchemeType::BGV; },
        [&](size_t i, Ciphertext& out) { mod_switch_to_next(*encrypted[i], out, pool); },
        [&](Ciphertext& proto) { scheme = mod_switch_to_next_prepare(*encrypted[0], proto, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            const uint32_t L = static_cast<uint32_t>(encrypted[0]->coeff_modulus_size());
            if (scheme == SchemeType::BFV) detail::divide_round_q_last_step(env, context_->plan(), L, in, proto.polynomial_count(), out, count);
            else detail::mod_switch_drop_step(env, context_->plan(), L, static_cast<uint32_t>(proto.coeff_modulus_size()), in, proto.polynomial_count(), out, count);
        });
}

void Evaluator::rescale_to_next_batched(const CVec& encrypted, const Vec& destination, MemoryPoolHandle pool) const {
    run_batched("[Evaluator::rescale_to_next_batched]", {&encrypted}, destination, pool, always,
        [&](size_t i, Ciphertext& out) { rescale_to_next(*encrypted[i], out, pool); },
        [&](Ciphertext& proto) {
            // rescale_to_next's own checks (evaluator_modswitch.cu:445-461), then checks + shape of item 0 without device work
            if (encrypted[0]->contains_seed()) throw std::invalid_argument("[Evaluator::rescale_to_next] Argument contains seed.");
            if (context_->last_parms_id() == encrypted[0]->parms_id()) throw std::invalid_argument("[Evaluator::rescale_to_next] End of modulus switching chain reached.");
            if (context_->first_context_data().value()->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument("[Evaluator::rescale_to_next] Cannot rescale BFV/BGV ciphertext.");
            mod_switch_scale_prepare(*encrypted[0], proto, pool);
        },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            detail::rescale_step(env, context_->plan(), static_cast<uint32_t>(encrypted[0]->coeff_modulus_size()), in, proto.polynomial_count(), out, count);
        });
}

// -- ModRaise (addition) -----------------------------------------------------------------------------------------------------------------
void Evaluator::mod_raise_batched(const CVec& encrypted, const Vec& destination, std::optional<ParmsID> parms_id, MemoryPoolHandle pool) const {
    run_batched("[Evaluator::mod_raise_batched]", {&encrypted}, destination, pool, always,
        [&](size_t i, Ciphertext& out) { mod_raise(*encrypted[i], out, parms_id, pool); },
        [&](Ciphertext& proto) { mod_raise_prepare(*encrypted[0], proto, parms_id, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            detail::mod_raise_step(env, context_->ckks(), static_cast<uint32_t>(encrypted[0]->coeff_modulus_size()), static_cast<uint32_t>(proto.coeff_modulus_size()),
                                   proto.is_ntt_form(), in, proto.polynomial_count(), out, count);
        });
}

// -- NTT ---------------------------------------------------------------------------------------------------------------
void Evaluator::transform_batched(bool inverse, const CVec& encrypted, const Vec& destination, MemoryPoolHandle pool) const {
    run_batched(inverse ? "[Evaluator::transform_from_ntt_batched]" : "[Evaluator::transform_to_ntt_batched]", {&encrypted}, destination, pool, always,
        [&](size_t i, Ciphertext& out) { transform(inverse, *encrypted[i], out, pool); },
        [&](Ciphertext& proto) { transform_prepare(inverse, *encrypted[0], proto, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            detail::ntt_step(env, context_->plan(), inverse, in, out, count, proto.polynomial_count(), static_cast<uint32_t>(proto.coeff_modulus_size()));
        });
}

void Evaluator::transform_to_ntt_batched(const CVec& encrypted, const Vec& destination, MemoryPoolHandle pool) const { transform_batched(false, encrypted, destination, pool); }
void Evaluator::transform_from_ntt_batched(const CVec& encrypted, const Vec& destination, MemoryPoolHandle pool) const { transform_batched(true, encrypted, destination, pool); }
void Evaluator::transform_to_ntt_inplace_batched(const Vec& encrypted, MemoryPoolHandle pool) const { transform_batched(false, as_const(encrypted), encrypted, pool); }
void Evaluator::transform_from_ntt_inplace_batched(const Vec& encrypted, MemoryPoolHandle pool) const { transform_batched(true, as_const(encrypted), encrypted, pool); }

// -- Galois automorphism, key switching (evaluator_keyswitching.cu:52-93, :147-179) ------------------------------------------------------
void Evaluator::apply_galois_batched(const CVec& encrypted, size_t galois_element, const GaloisKeys& galois_keys, const Vec& destination, MemoryPoolHandle pool) const {
    const SchemeType scheme = context_->key_context_data().value()->parms().scheme();
    std::vector<const uint64_t*> keys;
    run_batched("[Evaluator::apply_galois_batched]", {&encrypted}, destination, pool,
        [&] { return scheme != SchemeType::BGV; },
        [&](size_t i, Ciphertext& out) { apply_galois(*encrypted[i], galois_element, galois_keys, out, pool); },
        [&](Ciphertext& proto) { apply_galois_prepare(*encrypted[0], galois_element, galois_keys, proto, keys, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            detail::apply_galois_step(env, context_->plan(), nullptr, static_cast<uint32_t>(proto.coeff_modulus_size()), proto.poly_modulus_degree(), scheme == SchemeType::CKKS,
                                      proto.is_ntt_form(), galois_element, in, keys.data(), out, count);
        });
}

void Evaluator::apply_keyswitching_batched(const CVec& encrypted, const KSwitchKeys& kswitch_keys, const Vec& destination, MemoryPoolHandle pool) const {
    const SchemeType scheme = context_->key_context_data().value()->parms().scheme();
    std::vector<const uint64_t*> keys;
    run_batched("[Evaluator::apply_keyswitching_batched]", {&encrypted}, destination, pool,
        [&] { return scheme != SchemeType::BGV; },
        [&](size_t i, Ciphertext& out) { apply_keyswitching(*encrypted[i], kswitch_keys, out, pool); },
        [&](Ciphertext& proto) { apply_keyswitching_prepare(*encrypted[0], kswitch_keys, proto, keys, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            detail::apply_keyswitching_step(env, context_->plan(), nullptr, static_cast<uint32_t>(proto.coeff_modulus_size()), proto.poly_modulus_degree(),
                                            scheme == SchemeType::CKKS, proto.is_ntt_form(), in, keys.data(), out, count);
        });
}

// -- ciphertext +/- plaintext, ciphertext x plaintext ----------------------------------------------------------------------
// (both keep the per-object call on item 0 as their prepare: its checks and metadata come out of sizeable host logic)
namespace {
// the mod-t plaintexts of a batch as zero-padded rows [count][n]
void pad_plains(const std::vector<const Plaintext*>& plain, size_t n, utils::DynamicArray& rows, const char* too_long, hipStream_t stream) {
    rows.set_zero();
    for (size_t i = 0; i < plain.size(); i++) {
        if (plain[i]->coeff_count() > n) throw std::invalid_argument(too_long);
        hip_check(hipMemcpyAsync(rows.raw_pointer() + i * n, plain[i]->poly(), plain[i]->coeff_count() * 8, hipMemcpyDeviceToDevice, stream), "copy_device_to_device");
    }
}
bool mod_t_on_device(const std::vector<const Plaintext*>& plain) {
    for (const Plaintext* p : plain) if (p->parms_id() != parms_id_zero || p->is_ntt_form() || !p->on_device()) return false;
    return true;
}
}  // namespace

void Evaluator::translate_plain_batched(const CVec& encrypted, const std::vector<const Plaintext*>& plain, const Vec& destination, bool subtract, MemoryPoolHandle pool) const {
    same_size("[Evaluator::translate_plain_batched]", plain.size(), destination.size());
    run_batched("[Evaluator::translate_plain_batched]", {&encrypted}, destination, pool,
        [&] { return context_->key_context_data().value()->parms().scheme() == SchemeType::BFV && mod_t_on_device(plain); },
        [&](size_t i, Ciphertext& out) { out = encrypted[i]->clone(pool); translate_plain_inplace(out, *plain[i], subtract, pool); },
        [&](Ciphertext& proto) { proto = encrypted[0]->clone(pool); translate_plain_inplace(proto, *plain[0], subtract, pool); },
        // BFV, plaintexts mod t: c0 +/- round(q/t * m) for the whole batch (scaling_variant::multiply_add_plain_inplace)
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            const size_t n = proto.poly_modulus_degree(), L = proto.coeff_modulus_size(), words = proto.data().size();
            utils::DynamicArray plains(count * n, true, pool);
            pad_plains(plain, n, plains, "[scaling_variant::scale_up] destination_coeff_count should no less than plain_coeff_count.", env.stream);
            hip_check(hipMemcpyAsync(out, in, count * words * 8, hipMemcpyDeviceToDevice, env.stream), "copy_device_to_device");
            troyn_check_public(troyn_bfv_scale_up(context_->behz(L), plains.raw_pointer(), n, n, in, words, out, words, subtract ? 1 : 0, count, env.stream));
        });
}

void Evaluator::multiply_plain_batched(const CVec& encrypted, const std::vector<const Plaintext*>& plain, const Vec& destination, MemoryPoolHandle pool) const {
    if (encrypted.size() != plain.size() || encrypted.size() != destination.size())
        throw std::invalid_argument("[Evaluator::multiply_plain_batched] Input and destination have different sizes.");
    bool ntt = !encrypted.empty();
    for (size_t i = 0; i < encrypted.size() && ntt; i++) ntt = encrypted[i]->is_ntt_form() && plain[i]->is_ntt_form();
    bool distinct = true;
    for (size_t i = 0; i < destination.size() && distinct; i++)
        for (size_t k = 0; k < i && distinct; k++) distinct = destination[k] != destination[i];
    if (ntt && distinct && uniform(encrypted)) {
        // evaluator_multiply_plain.cu:356-385 (multiply_plain_ntt_batched): one launch over all (ciphertext, plaintext) pairs;
        // an in-place call (destination[i] == encrypted[i]) goes through temporaries
        std::vector<Ciphertext> tmp(encrypted.size());
        Vec tp;
        for (Ciphertext& c : tmp) tp.push_back(&c);
        multiply_plain_accumulate(encrypted, plain, tp, true, pool);
        for (size_t i = 0; i < tmp.size(); i++) *destination[i] = std::move(tmp[i]);
        return;
    }
    // evaluator_multiply_plain.cu:70-194 (multiply_plain_normal_batched): coefficient-form ciphertexts times plaintexts modulo t (BFV) --
    // the showcase of examples/15_batched_operation.cu.  One gather, one centralize launch and one NTT launch for the plaintexts, one
    // NTT launch for the ciphertexts, one product launch, one inverse NTT launch.
    run_batched("[Evaluator::multiply_plain_batched]", {&encrypted}, destination, pool,
        [&] { return distinct && !encrypted[0]->is_ntt_form() && context_->key_context_data().value()->parms().scheme() == SchemeType::BFV && mod_t_on_device(plain); },
        [&](size_t i, Ciphertext& out) { multiply_plain(*encrypted[i], *plain[i], out, pool); },
        [&](Ciphertext& proto) { multiply_plain(*encrypted[0], *plain[0], proto, pool); },           // every check of the per-object form; fixes shape and metadata
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            const size_t n = proto.poly_modulus_degree(), pcnt = proto.polynomial_count();
            const uint32_t L = static_cast<uint32_t>(proto.coeff_modulus_size());
            const troyn_plan* plan = context_->plan();
            const uint64_t t = context_->first_context_data().value()->parms().plain_modulus().value();
            utils::DynamicArray plains(count * n, true, pool), lifted(count * L * n, true, pool);
            pad_plains(plain, n, plains, "[scaling_variant::centralize] plain_coeff_count exceeds the polynomial degree.", env.stream);
            troyn_check_public(troyn_plain_centralize_ntt(plan, L, t, plains.raw_pointer(), n, n, lifted.raw_pointer(), count, env.stream));
            detail::ntt_step(env, plan, false, in, out, count, pcnt, L);
            troyn_check_public(troyn_dyadic_broadcast_product(plan, 0, L, out, pcnt, lifted.raw_pointer(), static_cast<size_t>(L) * n, out, count, env.stream));
            detail::ntt_step(env, plan, true, out, out, count, pcnt, L);
        });
}

// -- rotations of a batch ------------------------------------------------------------------------------------------------------------
void Evaluator::rotate_internal_batched(const std::vector<const Ciphertext*>& encrypted, int steps, const GaloisKeys& galois_keys, const std::vector<Ciphertext*>& destination,
                                        MemoryPoolHandle pool) const {
    // evaluator_keyswitching.cu:263-294 for every member; the Galois elements depend on the step only, so each NAF term is one apply_galois_batched
    const char* P = "[Evaluator::rotate_inplace_internal]";
    same_size(P, encrypted.size(), destination.size());
    if (encrypted.empty()) return;
    if (galois_keys.parms_id() != context_->key_parms_id()) throw std::invalid_argument(std::string(P) + " Galois keys has incorrect parms id.");
    if (steps == 0) {
        for (size_t i = 0; i < encrypted.size(); i++) if (destination[i] != encrypted[i]) *destination[i] = encrypted[i]->clone(pool);
        return;
    }
    const size_t n = encrypted[0]->poly_modulus_degree();
    const size_t element = utils::galois_element_from_step(n, steps);
    if (galois_keys.has_key(element)) { apply_galois_batched(encrypted, element, galois_keys, destination, pool); return; }
    const std::vector<int> naf_steps = utils::naf(steps);
    if (naf_steps.size() == 1) throw std::invalid_argument(std::string(P) + " Galois key not present.");
    bool first = true;
    for (int st : naf_steps) {
        if (first) { rotate_internal_batched(encrypted, st, galois_keys, destination, pool); first = false; }
        else rotate_internal_batched(as_const(destination), st, galois_keys, destination, pool);
    }
}

void Evaluator::rotate_rows_batched(const std::vector<const Ciphertext*>& e, int steps, const GaloisKeys& k, const std::vector<Ciphertext*>& d, MemoryPoolHandle pool) const {
    const SchemeType scheme = context_->key_context_data().value()->parms().scheme();
    if (scheme != SchemeType::BFV && scheme != SchemeType::BGV) throw std::invalid_argument("[Evaluator::rotate_rows_inplace] Rotate rows only applies for BFV or BGV");
    rotate_internal_batched(e, steps, k, d, pool);
}

void Evaluator::rotate_vector_batched(const std::vector<const Ciphertext*>& e, int steps, const GaloisKeys& k, const std::vector<Ciphertext*>& d, MemoryPoolHandle pool) const {
    if (context_->key_context_data().value()->parms().scheme() != SchemeType::CKKS) throw std::invalid_argument("[Evaluator::rotate_vector_inplace] Rotate vector only applies for CKKS");
    rotate_internal_batched(e, steps, k, d, pool);
}

// conjugate_internal_batched: the element of step 0 for every member
void Evaluator::conjugate_batched(const std::vector<const Ciphertext*>& e, const GaloisKeys& k, const std::vector<Ciphertext*>& d, MemoryPoolHandle pool) const {
    same_size("[Evaluator::conjugate_internal_batched]", e.size(), d.size());
    if (e.empty()) return;
    apply_galois_batched(e, utils::galois_element_from_step(e[0]->poly_modulus_degree(), 0), k, d, pool);
}

void Evaluator::rotate_columns_batched(const std::vector<const Ciphertext*>& e, const GaloisKeys& k, const std::vector<Ciphertext*>& d, MemoryPoolHandle pool) const {
    const SchemeType scheme = context_->key_context_data().value()->parms().scheme();
    if (scheme != SchemeType::BFV && scheme != SchemeType::BGV) throw std::invalid_argument("[Evaluator::rotate_columns_inplace] Rotate columns only applies for BFV or BGV");
    conjugate_batched(e, k, d, pool);
}

void Evaluator::complex_conjugate_batched(const std::vector<const Ciphertext*>& e, const GaloisKeys& k, const std::vector<Ciphertext*>& d, MemoryPoolHandle pool) const {
    if (context_->key_context_data().value()->parms().scheme() != SchemeType::CKKS)
        throw std::invalid_argument("[Evaluator::complex_conjugate_inplace] Complex conjugate only applies for CKKS");
    conjugate_batched(e, k, d, pool);
}

// -- modulus switching down to a level -------------------------------------------------------------------------------------------------
void Evaluator::mod_switch_to_batched(const std::vector<const Ciphertext*>& encrypted, const ParmsID& parms_id, const std::vector<Ciphertext*>& destination,
                                      MemoryPoolHandle pool) const {
    // evaluator_modswitch.cu:222-260 per member; a uniform batch steps down together through mod_switch_to_next_batched
    const char* P = "[Evaluator::mod_switch_to_batched]";
    same_size(P, encrypted.size(), destination.size());
    if (encrypted.empty()) return;
    auto target = context_->get_context_data(parms_id);
    if (!target.has_value()) throw std::invalid_argument("[Evaluator::mod_switch_to] ParmsID is not valid for the current context.");
    if (!uniform(encrypted)) {
        for (size_t i = 0; i < encrypted.size(); i++) { Ciphertext out; mod_switch_to(*encrypted[i], parms_id, out, pool); *destination[i] = std::move(out); }
        return;
    }
    auto cd = context_->get_context_data(encrypted[0]->parms_id());
    if (!cd.has_value()) throw std::invalid_argument("[Evaluator::mod_switch_to] ParmsID is not valid for the current context.");
    if (cd.value()->chain_index() < target.value()->chain_index()) throw std::invalid_argument("[Evaluator::mod_switch_to_inplace] Cannot switch to a higher level.");
    if (encrypted[0]->parms_id() == parms_id) {
        for (size_t i = 0; i < encrypted.size(); i++) if (destination[i] != encrypted[i]) *destination[i] = encrypted[i]->clone(pool);
        return;
    }
    mod_switch_to_next_batched(encrypted, destination, pool);
    while (destination[0]->parms_id() != parms_id) mod_switch_to_next_batched(as_const(destination), destination, pool);
}

// -- shifts and the 1/N factor of the packing tree ----------------------------------------------------------------------------------------
void Evaluator::negacyclic_shift_batched(const std::vector<const Ciphertext*>& encrypted, size_t shift, const std::vector<Ciphertext*>& destination, MemoryPoolHandle pool) const {
    run_batched("[Evaluator::negacyclic_shift_batched]", {&encrypted}, destination, pool, always,
        [&](size_t i, Ciphertext& out) { negacyclic_shift(*encrypted[i], shift, out, pool); },
        [&](Ciphertext& proto) { negacyclic_shift_prepare(*encrypted[0], proto, pool); },
        [&](const detail::StepEnv& env, const Ciphertext& proto, const uint64_t* in, const uint64_t*, uint64_t* out, size_t count) {
            detail::negacyclic_shift_step(env, context_->plan(), static_cast<uint32_t>(proto.coeff_modulus_size()), in, out, shift, count * proto.polynomial_count());
        });
}

void Evaluator::divide_by_poly_modulus_degree_inplace_batched(const std::vector<Ciphertext*>& encrypted, uint64_t mul, MemoryPoolHandle pool) const {
    (void)pool;
    for (Ciphertext* c : encrypted) divide_by_poly_modulus_degree_inplace(*c, mul);
}

}  // namespace troy
