// The mirror's device steps (device_steps.h): workspace from the pool, then the C-ABI entry.  No argument checks, no Ciphertext.
#include "device_steps.h"

#include <hip/hip_runtime.h>

namespace troy {
namespace detail {

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("[kernel_provider::") + what + "] " + hipGetErrorString(e));
}

namespace {

// a workspace of `bytes` from the step's pool; it returns to the pool when the step ends and is reused in stream order (MemoryPool)
utils::DynamicArray workspace(const StepEnv& env, size_t bytes) { return utils::DynamicArray((bytes + 7) / 8, true, env.pool); }

void gather_table(const StepEnv& env, size_t count, utils::DynamicArray& table) {
    if (table.size() == 0) table = workspace(env, troyn_gather_workspace_bytes(count));
}

// the c1 of every (c0, c1) of `pairs` as [count][words]: the key-switch targets
void extract_c1(const StepEnv& env, const uint64_t* pairs, size_t words, uint64_t* target, size_t count) {
    if (count == 1) hip_check(hipMemcpyAsync(target, pairs + words, words * 8, hipMemcpyDeviceToDevice, env.stream), "copy_device_to_device");
    else hip_check(hipMemcpy2DAsync(target, words * 8, pairs + words, 2 * words * 8, words * 8, count, hipMemcpyDeviceToDevice, env.stream), "copy_device_to_device");
}

}  // namespace

const uint64_t* stage(const StepEnv& env, const std::vector<const uint64_t*>& src, size_t words, utils::DynamicArray& staged, utils::DynamicArray& table) {
    const size_t count = src.size();
    bool adjacent = true;
    for (size_t i = 0; i < count && adjacent; i++) adjacent = src[i] == src[0] + i * words;
    if (adjacent) return src[0];
    staged = utils::DynamicArray(count * words, true, env.pool);
    gather_table(env, count, table);
    env.check(troyn_gather(src.data(), count, words, staged.raw_pointer(), table.raw_pointer(), troyn_gather_workspace_bytes(count), env.stream));   // (`src` is consumed by the call)
    return staged.raw_pointer();
}

void scatter(const StepEnv& env, const uint64_t* block, const std::vector<uint64_t*>& dst, size_t words, utils::DynamicArray& table) {
    gather_table(env, dst.size(), table);
    env.check(troyn_scatter(block, dst.data(), dst.size(), words, table.raw_pointer(), troyn_gather_workspace_bytes(dst.size()), env.stream));
}

void multiply_dyadic_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* a, size_t p1, const uint64_t* b, size_t p2, uint64_t* out, size_t count) {
    env.check(troyn_dyadic_convolute(plan, 0, L, a, p1, b, p2, out, count, env.stream));
}

void multiply_bfv_step(const StepEnv& env, const troyn_behz* behz, const uint64_t* a, size_t p1, const uint64_t* b, size_t p2, uint64_t* out, size_t count) {
    const size_t bytes = troyn_bfv_multiply_workspace_bytes(behz, p1, p2, count);
    utils::DynamicArray ws = workspace(env, bytes);
    env.check(troyn_bfv_multiply(behz, a, p1, b, p2, out, ws.raw_pointer(), bytes, count, env.stream));
}

void square_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, uint64_t* out, size_t count) {
    env.check(troyn_dyadic_square(plan, 0, L, in, out, count, env.stream));
}

void relinearize_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* in,
                      const uint64_t* const* keys, uint64_t* out, size_t count) {
    const size_t bytes = troyn_relinearize_workspace_bytes(plan, L, count);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    if (bgv) env.check(troyn_bgv_relinearize(bgv, L, in, keys, out, ws.raw_pointer(), bytes, count, env.stream));
    else env.check(troyn_relinearize(plan, L, ckks, ntt_form, in, keys, out, ws.raw_pointer(), bytes, count, env.stream));
}

void switch_key_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* target,
                     const uint64_t* const* keys, int assign, uint64_t* out, size_t count) {
    const size_t bytes = troyn_switch_key_workspace_bytes(plan, L, count);
    utils::DynamicArray ws = workspace(env, bytes);
    // BGV: the ski_util5 tail needs the key level's q_special^-1 mod t (evaluator_keyswitching_core.cu:930-932)
    if (bgv) env.check(troyn_bgv_switch_key(bgv, L, target, keys, assign, out, ws.raw_pointer(), bytes, count, env.stream));
    else env.check(troyn_switch_key(plan, L, ckks, ntt_form, target, keys, assign, out, ws.raw_pointer(), bytes, count, env.stream));
}

void rescale_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, size_t polys, uint64_t* out, size_t count) {
    const size_t bytes = troyn_divide_and_round_q_last_ntt_workspace_bytes(plan, L, polys, count);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    env.check(troyn_divide_and_round_q_last_ntt(plan, L, in, polys, out, ws.raw_pointer(), bytes, count, env.stream));
}

void divide_round_q_last_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, size_t polys, uint64_t* out, size_t count) {
    env.check(troyn_divide_and_round_q_last(plan, L, in, polys, out, count, env.stream));
}

void bgv_mod_t_divide_step(const StepEnv& env, const troyn_bgv* bgv, const uint64_t* in, size_t polys, uint64_t* out, size_t count) {
    // RNSTool::mod_t_and_divide_q_last_ntt
    const size_t bytes = troyn_bgv_mod_switch_workspace_bytes(bgv, polys, count);
    utils::DynamicArray ws = workspace(env, bytes);
    env.check(troyn_bgv_mod_t_and_divide_q_last_ntt(bgv, in, polys, out, ws.raw_pointer(), bytes, count, env.stream));
}

void mod_switch_drop_step(const StepEnv& env, const troyn_plan* plan, uint32_t L_in, uint32_t L_out, const uint64_t* in, size_t polys, uint64_t* out, size_t count) {
    env.check(troyn_mod_switch_drop(plan, L_in, L_out, in, polys, out, count, env.stream));
}

void mod_raise_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t L_in, uint32_t L_out, bool ntt_form, const uint64_t* in, size_t polys, uint64_t* out, size_t count) {
    const size_t bytes = troyn_ckks_mod_raise_workspace_bytes(ckks, L_in, L_out, polys, count, ntt_form ? 1 : 0);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    env.check(troyn_ckks_mod_raise(ckks, L_in, L_out, ntt_form ? 1 : 0, in, polys, out, ws.raw_pointer(), bytes, count, env.stream));
}

void negate_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, uint64_t* out, size_t polys) {
    env.check(troyn_negate(plan, 0, L, in, out, polys, env.stream));
}

void add_sub_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, bool subtract, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t polys) {
    env.check((subtract ? troyn_sub : troyn_add)(plan, 0, L, a, b, out, polys, env.stream));
}

void ckks_complex_split_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* a, const uint64_t* b, uint64_t* s, uint64_t* d, size_t count) {
    env.check(troyn_ckks_complex_split(plan, L, a, b, s, d, count, env.stream));
}

void ckks_complex_join_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count) {
    env.check(troyn_ckks_complex_join(plan, L, a, b, out, count, env.stream));
}

void ntt_step(const StepEnv& env, const troyn_plan* plan, bool inverse, const uint64_t* in, uint64_t* out, size_t count, size_t polys, uint32_t L) {
    env.check(troyn_ntt(plan, inverse ? 1 : 0, in, out, count, polys, L, 0, L, TROYN_IDX_COMPONENTWISE, 0, env.stream));
}

void apply_galois_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, size_t n, bool ckks, bool ntt_form, size_t galois_element,
                       const uint64_t* in, const uint64_t* const* keys, uint64_t* out, size_t count) {
    // Evaluator::apply_galois (evaluator_keyswitching.cu:147-179) over the batch: the permuted c1s are the targets, the switched result overwrites them
    const size_t words = static_cast<size_t>(L) * n;
    env.check(troyn_apply_galois(plan, 0, L, ntt_form ? 1 : 0, galois_element, in, out, count * 2, env.stream));
    utils::DynamicArray target(count * words, true, env.pool);
    extract_c1(env, out, words, target.raw_pointer(), count);
    switch_key_step(env, plan, bgv, L, ckks, ntt_form, target.raw_pointer(), keys, TROYN_ASSIGN_OVERWRITE_EXCEPT_FIRST, out, count);
}

void apply_keyswitching_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, size_t n, bool ckks, bool ntt_form, const uint64_t* in,
                             const uint64_t* const* keys, uint64_t* out, size_t count) {
    // evaluator_keyswitching.cu:11-93: the result starts as a copy of the operands
    const size_t words = static_cast<size_t>(L) * n;
    hip_check(hipMemcpyAsync(out, in, count * 2 * words * sizeof(uint64_t), hipMemcpyDeviceToDevice, env.stream), "copy_device_to_device");
    if (count == 1) {   // the one c1 is its own [1][words]
        switch_key_step(env, plan, bgv, L, ckks, ntt_form, in + words, keys, TROYN_ASSIGN_OVERWRITE_EXCEPT_FIRST, out, 1);
        return;
    }
    utils::DynamicArray target(count * words, true, env.pool);
    extract_c1(env, in, words, target.raw_pointer(), count);
    switch_key_step(env, plan, bgv, L, ckks, ntt_form, target.raw_pointer(), keys, TROYN_ASSIGN_OVERWRITE_EXCEPT_FIRST, out, count);
}

void negacyclic_shift_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, uint64_t* out, size_t shift, size_t polys) {
    env.check(troyn_negacyclic_shift(plan, 0, L, in, out, shift, polys, env.stream));
}

void multiply_relinearize_rescale_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* a, const uint64_t* b, const uint64_t* const* keys,
                                       uint64_t* out, size_t count) {
    const size_t bytes = troyn_ckks_multiply_relinearize_rescale_workspace_bytes(plan, L, count);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    env.check(troyn_ckks_multiply_relinearize_rescale(plan, L, a, b, keys, out, ws.raw_pointer(), bytes, count, env.stream));
}

void bgv_multiply_relinearize_mod_switch_step(const StepEnv& env, const troyn_bgv* key_level, const troyn_bgv* level, uint32_t L, const uint64_t* a, const uint64_t* b,
                                              const uint64_t* const* keys, uint64_t* out, size_t count) {
    const size_t bytes = troyn_bgv_multiply_relinearize_mod_switch_workspace_bytes(key_level, L, count);
    utils::DynamicArray ws = workspace(env, bytes);
    env.check(troyn_bgv_multiply_relinearize_mod_switch(key_level, level, a, b, keys, out, ws.raw_pointer(), bytes, count, env.stream));
}

void apply_galois_many_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                            const uint64_t* elements, const uint64_t* const* keys, size_t terms, uint64_t* out, size_t count) {
    const size_t bytes = troyn_apply_galois_hoisted_workspace_bytes(plan, L, terms, count, 0);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    if (bgv) env.check(troyn_bgv_apply_galois_many(bgv, L, ct, elements, keys, terms, out, ws.raw_pointer(), bytes, count, env.stream));
    else env.check(troyn_apply_galois_many(plan, L, ckks, ntt_form, ct, elements, keys, terms, out, ws.raw_pointer(), bytes, count, env.stream));
}

void apply_galois_sum_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                           const uint64_t* elements, const uint64_t* const* keys, size_t terms, uint64_t* out, size_t count) {
    const size_t bytes = troyn_apply_galois_hoisted_workspace_bytes(plan, L, terms, count, 1);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    if (bgv) env.check(troyn_bgv_apply_galois_sum(bgv, L, ct, elements, keys, terms, out, ws.raw_pointer(), bytes, count, env.stream));
    else env.check(troyn_apply_galois_sum(plan, L, ckks, ntt_form, ct, elements, keys, terms, out, ws.raw_pointer(), bytes, count, env.stream));
}

void apply_galois_weighted_sums_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                                     const uint64_t* elements, const uint64_t* const* keys, size_t terms, const uint64_t* const* weights, size_t slots, uint64_t* out,
                                     size_t count) {
    const size_t bytes = troyn_apply_galois_weighted_workspace_bytes(plan, L, terms, slots, count, ntt_form ? 1 : 0);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    if (bgv) env.check(troyn_bgv_apply_galois_weighted_sums(bgv, L, ct, elements, keys, terms, weights, slots, out, ws.raw_pointer(), bytes, count, env.stream));
    else env.check(troyn_apply_galois_weighted_sums(plan, L, ckks, ntt_form, ct, elements, keys, terms, weights, slots, out, ws.raw_pointer(), bytes, count, env.stream));
}

void apply_galois_sum_each_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* cts,
                                const uint64_t* elements, const uint64_t* const* keys, size_t terms, uint64_t* out, size_t count) {
    const size_t bytes = troyn_apply_galois_sum_each_workspace_bytes(plan, L, terms, count, ntt_form ? 1 : 0);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    if (bgv) env.check(troyn_bgv_apply_galois_sum_each(bgv, L, cts, elements, keys, terms, out, ws.raw_pointer(), bytes, count, env.stream));
    else env.check(troyn_apply_galois_sum_each(plan, L, ckks, ntt_form, cts, elements, keys, terms, out, ws.raw_pointer(), bytes, count, env.stream));
}

void linear_transform_bsgs_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                                const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies, const uint64_t* giant_elements,
                                const uint64_t* const* giant_keys, size_t giants, const uint64_t* const* weights, uint64_t* out, size_t count) {
    const size_t bytes = troyn_linear_transform_bsgs_workspace_bytes(plan, L, babies, giants, count, ntt_form ? 1 : 0);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    if (bgv)
        env.check(troyn_bgv_linear_transform_bsgs(bgv, L, ct, baby_elements, baby_keys, babies, giant_elements, giant_keys, giants, weights, out, ws.raw_pointer(), bytes,
                                                  count, env.stream));
    else
        env.check(troyn_linear_transform_bsgs(plan, L, ckks, ntt_form, ct, baby_elements, baby_keys, babies, giant_elements, giant_keys, giants, weights, out,
                                              ws.raw_pointer(), bytes, count, env.stream));
}

void linear_transform_bsgs_double_hoisted_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                                               const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies, const uint64_t* giant_elements,
                                               const uint64_t* const* giant_keys, size_t giants, const uint64_t* const* weights, uint64_t* out, size_t count) {
    const size_t bytes = troyn_linear_transform_bsgs_double_hoisted_workspace_bytes(plan, L, babies, giants, count, ntt_form ? 1 : 0);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    env.check(troyn_linear_transform_bsgs_double_hoisted(plan, L, ckks, ntt_form, ct, baby_elements, baby_keys, babies, giant_elements, giant_keys, giants, weights, out,
                                                         ws.raw_pointer(), bytes, count, env.stream));
}

void multiply_accumulate_relinearize_rescale_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* const* a, const uint64_t* const* b, size_t terms,
                                                  const uint64_t* const* keys, uint64_t* out, size_t count) {
    const size_t bytes = troyn_ckks_multiply_accumulate_relinearize_rescale_workspace_bytes(plan, L, terms, count);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    env.check(troyn_ckks_multiply_accumulate_relinearize_rescale(plan, L, a, b, terms, keys, out, ws.raw_pointer(), bytes, count, env.stream));
}

void multiply_affine_relinearize_rescale_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* const* a, const uint64_t* const* b,
                                              const uint64_t* const* c, const uint32_t* c_nmod, const uint64_t* alpha, const uint64_t* weight, const uint64_t* constant,
                                              const uint64_t* const* keys, uint64_t* out, size_t count) {
    const size_t bytes = troyn_ckks_multiply_affine_relinearize_rescale_workspace_bytes(plan, L, count);
    // (one spare word, as before the step: the entry rounds the offset of its 16-byte-aligned table inside its own byte count and needs none)
    utils::DynamicArray ws((bytes + 15) / 8, true, env.pool);
    LaunchGate gate(env.gated);
    env.check(troyn_ckks_multiply_affine_relinearize_rescale(plan, L, a, b, c, c_nmod, alpha, weight, constant, keys, out, ws.raw_pointer(), bytes, count, env.stream));
}

void bfv_multiply_accumulate_step(const StepEnv& env, const troyn_behz* behz, const uint64_t* const* a, const uint64_t* const* b, size_t terms, const uint64_t* const* keys,
                                  uint64_t* out, size_t count) {
    const size_t bytes = keys ? troyn_bfv_multiply_accumulate_relinearize_workspace_bytes(behz, terms, count) : troyn_bfv_multiply_accumulate_workspace_bytes(behz, terms, count);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    if (keys) env.check(troyn_bfv_multiply_accumulate_relinearize(behz, a, b, terms, keys, out, ws.raw_pointer(), bytes, count, env.stream));
    else env.check(troyn_bfv_multiply_accumulate(behz, a, b, terms, out, ws.raw_pointer(), bytes, count, env.stream));
}

void scalar_weighted_sums_step(const StepEnv& env, const troyn_plan* plan, uint32_t nmod, const uint64_t* const* ins, const uint32_t* in_nmod, size_t terms,
                               const uint64_t* scalars, const uint64_t* constants, size_t pcount, uint64_t* out, size_t slots) {
    const size_t bytes = troyn_scalar_weighted_sums_workspace_bytes(plan, nmod, terms, slots);
    // (one spare word, as before the step: the entry's byte count is a whole number of words and it aligns nothing inside the workspace)
    utils::DynamicArray ws((bytes + 15) / 8, true, env.pool);
    LaunchGate gate(env.gated);
    env.check(troyn_scalar_weighted_sums(plan, 0, nmod, ins, in_nmod, terms, scalars, constants, 0, pcount, out, slots, 1, ws.raw_pointer(), bytes, env.stream));
}

void multiply_plain_accumulate_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, size_t polys, const uint64_t* const* cts, const uint64_t* const* pts,
                                    uint64_t* const* dsts, size_t count, bool set_zero) {
    const size_t bytes = troyn_multiply_plain_accumulate_workspace_bytes(count);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    env.check(troyn_multiply_plain_accumulate(plan, 0, L, polys, cts, pts, dsts, count, set_zero ? 1 : 0, ws.raw_pointer(), bytes, env.stream));
}

void ckks_encode_step(const StepEnv& env, const troyn_ckks* ckks, bool simd, uint32_t L, const double* values, size_t row, double scale, uint64_t* out, uint32_t* flags,
                      size_t count) {
    const size_t bytes = troyn_ckks_encode_workspace_bytes(ckks, count);
    utils::DynamicArray ws((bytes + 7) / 8 + 2, true, env.pool);     // (two spare words, as before the step)
    LaunchGate gate(env.gated);
    env.check((simd ? troyn_ckks_encode_simd : troyn_ckks_encode_polynomial)(ckks, L, values, row, scale, out, flags, ws.raw_pointer(), bytes, count, env.stream));
}

void ckks_encode_diagonals_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t L, const double* src, bool matrix, uint32_t n, uint32_t nd, const uint32_t* pairs,
                                double scale, uint64_t* out, uint32_t* flags, size_t count) {
    const size_t bytes = troyn_ckks_encode_diagonals_workspace_bytes(ckks, count);
    utils::DynamicArray ws = workspace(env, bytes + 16);
    LaunchGate gate(env.gated);
    env.check(troyn_ckks_encode_diagonals(ckks, L, src, matrix ? 1 : 0, n, nd, pairs, scale, out, flags, ws.raw_pointer(), bytes, count, env.stream));
}

void ckks_dft_factor_diagonals_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t first, uint32_t count, bool inverse, int col_mask, int row_mask, bool conjugate,
                                    double constant, double* out) {
    env.check(troyn_ckks_dft_factor_diagonals(ckks, first, count, inverse ? 1 : 0, col_mask, row_mask, conjugate ? 1 : 0, constant, out, env.stream));
}

void ckks_dft_factor_diagonals_sparse_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t n, uint32_t first, uint32_t count, bool inverse, int col_mask, int row_mask,
                                           bool conjugate, double constant, double* out) {
    env.check(troyn_ckks_dft_factor_diagonals_sparse(ckks, n, first, count, inverse ? 1 : 0, col_mask, row_mask, conjugate ? 1 : 0, constant, out, env.stream));
}

void ckks_dft_factor_diagonals_packed_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t n, uint32_t first, uint32_t count, bool inverse, double constant, double* out) {
    env.check(troyn_ckks_dft_factor_diagonals_packed(ckks, n, first, count, inverse ? 1 : 0, constant, out, env.stream));
}

void ckks_decode_step(const StepEnv& env, const troyn_ckks* ckks, bool simd, uint32_t L, const uint64_t* in, double scale, double* out, size_t count) {
    const size_t bytes = troyn_ckks_workspace_bytes(ckks, L, count);
    utils::DynamicArray ws((bytes + 7) / 8 + 2, true, env.pool);     // (two spare words, as before the step)
    LaunchGate gate(env.gated);
    env.check((simd ? troyn_ckks_decode_simd : troyn_ckks_decode_polynomial)(ckks, L, in, scale, out, ws.raw_pointer(), bytes, count, env.stream));
}

void extract_lwe_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* const* srcs, const size_t* terms, uint64_t* c0, uint64_t* c1, size_t count) {
    const size_t bytes = troyn_extract_lwe_workspace_bytes(count);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    env.check(troyn_extract_lwe(plan, L, srcs, terms, c0, c1, count, ws.raw_pointer(), bytes, env.stream));
}

void pack_prepare_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, size_t polys, const uint64_t* const* srcs, size_t slots, uint64_t mul, size_t shift,
                       uint64_t* out) {
    const size_t bytes = troyn_pack_prepare_workspace_bytes(slots);
    utils::DynamicArray ws = workspace(env, bytes);
    LaunchGate gate(env.gated);
    env.check(troyn_pack_prepare(plan, L, polys, srcs, slots, mul, shift, out, ws.raw_pointer(), bytes, env.stream));
}

}  // namespace detail
}  // namespace troy
