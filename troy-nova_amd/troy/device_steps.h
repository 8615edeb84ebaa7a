// The device steps of the mirror: ONE function per C-ABI operation sizes the workspace, takes it from the pool and calls the C-ABI
// (include/troyn.h).  The per-object methods (troy.cpp, lwe.cpp) call a step with count = 1 on the calling thread's stream, the
// *_batched forms (batched.cpp) with the batch's count, the call-combining rendezvous (combine.cpp) on the shared stream.  A step
// checks no Ciphertext and touches none: the callers' *_prepare functions have done the checks and shaped the result.
//
// Rule: every C-ABI entry that takes a workspace is called from exactly one function of the mirror -- its step in device_steps.cpp --
// and no other file asks for a workspace size.  A change to an entry's workspace contract is a change to one function
// (tests/test_device_steps_rule.py reads the sources and holds the mirror to this).  The entries without a workspace that the Evaluator's
// operations use have their steps here too.  The one exception class: entries WITHOUT a workspace may be called directly where no
// Evaluator operation stands behind them -- the plaintext paths of plain_ops.cpp, ring2k.cpp and matmul.cpp, and what the encryptor,
// decryptor, encoders, key generator and packing tree do with troyn_ntt, troyn_add, troyn_negate and troyn_apply_galois.
//
// Operands are [count][...] contiguous words on the device; `out` may alias an input only where the entry allows it.
#pragma once

#include <hip/hip_runtime_api.h>

#include "troy.h"

namespace troy {
namespace detail {
#pragma GCC visibility push(hidden)   // internal to libtroy_amd.so: direct calls, nothing here is part of the library's surface

// where a step runs and who hears about a failure: the pool its workspace comes from, the stream, and the caller's checker of a C-ABI
// return code (troyn_check_public for the methods and the batched forms; the rendezvous has its own)
// the evaluator's scale comparison (utils/basics.h:150-160, as Evaluator::add uses it), for the units that implement Evaluator methods outside troy.cpp
bool scales_are_close(double a, double b);

struct StepEnv {
    const MemoryPoolHandle& pool;   // the CALLER's handle, by reference (no reference count per call): an environment is built in the argument list of a
                                    // step or as a local next to the handle it names, and never outlives that handle
    hipStream_t stream;
    void (*check)(int);
    bool gated = false;             // the caller's decision: a step that takes a workspace holds the stream gate around its C-ABI call only
};

// The threads that share a stream enter the library one at a time (troy.cpp).  A per-object caller that gates a step without a workspace
// holds one around the step; around a step with a workspace it sets StepEnv::gated, so that the pool is not used under the gate.
struct LaunchGate {
    std::mutex* m = nullptr;
    explicit LaunchGate(bool take = true);
    ~LaunchGate();
    LaunchGate(const LaunchGate&) = delete;
    LaunchGate& operator=(const LaunchGate&) = delete;
};

hipStream_t current_stream();                      // the calling thread's stream (troy.cpp)
void hip_check(hipError_t e, const char* what);   // kernel_provider.h:11-16: std::runtime_error with the runtime's message
inline StepEnv on_current_stream(const MemoryPoolHandle& pool, bool gated = false) { return StepEnv{pool, current_stream(), troyn_check_public, gated}; }

// `src[i]` as [count][words]: in place when the operands are consecutive windows, else one gather launch into `staged`.
// `table` is the gather's pointer table: taken from the pool here when the caller has not sized it already.
const uint64_t* stage(const StepEnv& env, const std::vector<const uint64_t*>& src, size_t words, utils::DynamicArray& staged, utils::DynamicArray& table);
// the inverse of a gather: [count][words] to `dst[i]`
void scatter(const StepEnv& env, const uint64_t* block, const std::vector<uint64_t*>& dst, size_t words, utils::DynamicArray& table);

void multiply_dyadic_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* a, size_t p1, const uint64_t* b, size_t p2, uint64_t* out, size_t count);
void multiply_bfv_step(const StepEnv& env, const troyn_behz* behz, const uint64_t* a, size_t p1, const uint64_t* b, size_t p2, uint64_t* out, size_t count);
void square_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, uint64_t* out, size_t count);
// 3 -> 2 components; `bgv` (the key level's handle) selects the BGV tail
void relinearize_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* in,
                      const uint64_t* const* keys, uint64_t* out, size_t count);
// `target` is [count][L][N]; `assign` a TROYN_ASSIGN_* value applied to out = [count][2][L][N]
void switch_key_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* target,
                     const uint64_t* const* keys, int assign, uint64_t* out, size_t count);
void rescale_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, size_t polys, uint64_t* out, size_t count);   // divide_and_round_q_last_ntt
void divide_round_q_last_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, size_t polys, uint64_t* out, size_t count);   // BFV
void bgv_mod_t_divide_step(const StepEnv& env, const troyn_bgv* bgv, const uint64_t* in, size_t polys, uint64_t* out, size_t count);
void mod_switch_drop_step(const StepEnv& env, const troyn_plan* plan, uint32_t L_in, uint32_t L_out, const uint64_t* in, size_t polys, uint64_t* out, size_t count);
// the centred base extension [count][polys][L_in][N] -> [count][polys][L_out][N] (CKKS ModRaise)
void mod_raise_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t L_in, uint32_t L_out, bool ntt_form, const uint64_t* in, size_t polys, uint64_t* out, size_t count);
void negate_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, uint64_t* out, size_t polys);
void add_sub_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, bool subtract, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t polys);
void ntt_step(const StepEnv& env, const troyn_plan* plan, bool inverse, const uint64_t* in, uint64_t* out, size_t count, size_t polys, uint32_t L);
// real and imaginary parts of CKKS slots (troyn_ckks_complex_split / _join, include/troyn.h): a, b, s, d, out [count][2][L][N] in NTT form; no workspace.
//   split: s = a + b, d = mu . (b - a); join: out = a + mu . b, mu the forward transform of X^(N/2)
void ckks_complex_split_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* a, const uint64_t* b, uint64_t* s, uint64_t* d, size_t count);
void ckks_complex_join_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count);
// (c0, c1) permuted by the element, the permuted c1s switched back: c0 += ks0, c1 = ks1
void apply_galois_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, size_t n, bool ckks, bool ntt_form, size_t galois_element,
                       const uint64_t* in, const uint64_t* const* keys, uint64_t* out, size_t count);
// (c0, c1) -> (c0 + ks0, ks1) with the c1s as key-switch targets
void apply_keyswitching_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, size_t n, bool ckks, bool ntt_form, const uint64_t* in,
                             const uint64_t* const* keys, uint64_t* out, size_t count);
void negacyclic_shift_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* in, uint64_t* out, size_t shift, size_t polys);
void multiply_relinearize_rescale_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* a, const uint64_t* b, const uint64_t* const* keys,
                                       uint64_t* out, size_t count);
// BGV: multiply -> relinearize -> mod_switch_to_next of `count` pairs at level L; key_level / level as troyn_bgv_multiply_relinearize_mod_switch
void bgv_multiply_relinearize_mod_switch_step(const StepEnv& env, const troyn_bgv* key_level, const troyn_bgv* level, uint32_t L, const uint64_t* a, const uint64_t* b,
                                              const uint64_t* const* keys, uint64_t* out, size_t count);

// Hoisted family (troyn_apply_galois_* / troyn_linear_transform_bsgs and their troyn_bgv_* forms): `bgv` (the key level's handle) selects the BGV entry,
// whose operands are in NTT form (ntt_form = true); the workspaces are the plan's for all three schemes.  ct is [count][2][L][N]; keys [terms][L] (null rows
// for the element 1 where the entry takes it); weights [slots][terms] / [giants][babies] key-level NTT rows or null
void apply_galois_many_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                            const uint64_t* elements, const uint64_t* const* keys, size_t terms, uint64_t* out, size_t count);     // out [count][terms][2][L][N]
void apply_galois_sum_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                           const uint64_t* elements, const uint64_t* const* keys, size_t terms, uint64_t* out, size_t count);      // out [count][2][L][N]
void apply_galois_weighted_sums_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                                     const uint64_t* elements, const uint64_t* const* keys, size_t terms, const uint64_t* const* weights, size_t slots, uint64_t* out,
                                     size_t count);
// cts [count][terms][2][L][N], one ciphertext per term
void apply_galois_sum_each_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* cts,
                                const uint64_t* elements, const uint64_t* const* keys, size_t terms, uint64_t* out, size_t count);
void linear_transform_bsgs_step(const StepEnv& env, const troyn_plan* plan, const troyn_bgv* bgv, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                                const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies, const uint64_t* giant_elements,
                                const uint64_t* const* giant_keys, size_t giants, const uint64_t* const* weights, uint64_t* out, size_t count);
// the same transform without the inner c0 divisions; BFV / CKKS only (the library has no BGV form)
void linear_transform_bsgs_double_hoisted_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, bool ckks, bool ntt_form, const uint64_t* ct,
                                               const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies, const uint64_t* giant_elements,
                                               const uint64_t* const* giant_keys, size_t giants, const uint64_t* const* weights, uint64_t* out, size_t count);

// Inner products: `a`, `b` are HOST tables of `terms` device pointers, each to [count] operands; out [count][...]
// CKKS: SUM_t a_t * b_t -> relinearize -> rescale, out [count][2][L - 1][N]
void multiply_accumulate_relinearize_rescale_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* const* a, const uint64_t* const* b, size_t terms,
                                                  const uint64_t* const* keys, uint64_t* out, size_t count);
// CKKS: alpha * a * b + weight * c + constant -> relinearize -> rescale per item: a, b, c host tables of `count` device pointers (c: null for no addend),
// the per-limb residue tables [count][L] prepared by the caller, out [count][2][L - 1][N]
void multiply_affine_relinearize_rescale_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* const* a, const uint64_t* const* b,
                                              const uint64_t* const* c, const uint32_t* c_nmod, const uint64_t* alpha, const uint64_t* weight, const uint64_t* constant,
                                              const uint64_t* const* keys, uint64_t* out, size_t count);
// BFV: the sum of BEHZ tensor products scaled down once, out [count][3][L][N]; with `keys` relinearized as well, out [count][2][L][N]
void bfv_multiply_accumulate_step(const StepEnv& env, const troyn_behz* behz, const uint64_t* const* a, const uint64_t* const* b, size_t terms, const uint64_t* const* keys,
                                  uint64_t* out, size_t count);
// out[s] = SUM_t scalars[s][t] * in_t (+ constants[s]) on `pcount` polynomials: the host tables [slots][terms][nmod] / [slots][nmod] (or null) are residues already
void scalar_weighted_sums_step(const StepEnv& env, const troyn_plan* plan, uint32_t nmod, const uint64_t* const* ins, const uint32_t* in_nmod, size_t terms,
                               const uint64_t* scalars, const uint64_t* constants, size_t pcount, uint64_t* out, size_t slots);
// dsts[i] (+)= cts[i] * pts[i] over host pointer tables of `count` items, NTT form
void multiply_plain_accumulate_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, size_t polys, const uint64_t* const* cts, const uint64_t* const* pts,
                                    uint64_t* const* dsts, size_t count, bool set_zero);

// The CKKS encoder on the device (troyn_ckks_encode_* / troyn_ckks_decode_*): `simd` selects the slot form, else the coefficient form.
// values [count][row] doubles (row complex values / doubles per item), out [count][L][N] NTT form, flags [count] (non-zero: too large)
void ckks_encode_step(const StepEnv& env, const troyn_ckks* ckks, bool simd, uint32_t L, const double* values, size_t row, double scale, uint64_t* out, uint32_t* flags,
                      size_t count);
// matrix diagonals into BSGS weights (troyn_ckks_encode_diagonals): src [nd][n][2] diagonals or [n][n][2] row-major matrix, pairs [count][2] =
// (diagonal, shift); out and flags as above.  All device memory.
void ckks_encode_diagonals_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t L, const double* src, bool matrix, uint32_t n, uint32_t nd, const uint32_t* pairs,
                                double scale, uint64_t* out, uint32_t* flags, size_t count);
// the product of the layers [first, first + count) of the special DFT by its present diagonals (troyn_ckks_dft_factor_diagonals): out [nd][N/2][2], device
// memory, the `src` of ckks_encode_diagonals_step in diagonals mode; masks: 0 none, 1 even, 2 odd.  No workspace.
void ckks_dft_factor_diagonals_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t first, uint32_t count, bool inverse, int col_mask, int row_mask, bool conjugate,
                                    double constant, double* out);
// the same on the sub-ring of n < N/2 slots (troyn_ckks_dft_factor_diagonals_sparse): out [nd][n][2], the `src` of ckks_encode_diagonals_step with that n
void ckks_dft_factor_diagonals_sparse_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t n, uint32_t first, uint32_t count, bool inverse, int col_mask, int row_mask,
                                           bool conjugate, double constant, double* out);
// both halves on period 2n (troyn_ckks_dft_factor_diagonals_packed, n <= N/4): out [nd][2n][2], the `src` of ckks_encode_diagonals_step with n = 2n
void ckks_dft_factor_diagonals_packed_step(const StepEnv& env, const troyn_ckks* ckks, uint32_t n, uint32_t first, uint32_t count, bool inverse, double constant, double* out);
void ckks_decode_step(const StepEnv& env, const troyn_ckks* ckks, bool simd, uint32_t L, const uint64_t* in, double scale, double* out, size_t count);

// LWE (lwe.cpp): coefficient `terms[i]` of srcs[i] as an LWE ciphertext, c0 [count][L] and c1 [count][L][N]; the leaves of the packing tree
void extract_lwe_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, const uint64_t* const* srcs, const size_t* terms, uint64_t* c0, uint64_t* c1, size_t count);
void pack_prepare_step(const StepEnv& env, const troyn_plan* plan, uint32_t L, size_t polys, const uint64_t* const* srcs, size_t slots, uint64_t mul, size_t shift,
                       uint64_t* out);

#pragma GCC visibility pop
}  // namespace detail
}  // namespace troy
