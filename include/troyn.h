/*
 * troyn.h -- C-ABI of the MI355X-native RNS-RLWE hot path (libtroyn.so).
 *
 * This is the drop-in boundary for the data-parallel hot path of lightbulb128/troy-nova:
 * negacyclic NTT/INTT, RNS dyadic multiply/add, key switching (relinearize), modulus
 * switching / CKKS rescale, and the BEHZ BFV multiply.  The reference has no FFI layer for
 * this path (its device code is reached by `if (on_device()) kernel<<<>>>` branches inside
 * C++ functions), so every entry point below names the reference C++
 * function (file:line under the reference's src/) whose *device branch* it replaces.
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - plain C: pointers + sizes only.  All polynomial data are DEVICE pointers to uint64_t in
 *    the reference layout data[(p*L + l)*N + i] (ciphertext.h:211-247), canonical residues.
 *  - every op takes `batch` independent items laid out contiguously ([batch][...]) unless a
 *    stride is given explicitly; batch = 1 reproduces the reference's single-object calls,
 *    batch > 1 replaces its `*_batched` pointer-table variants (box_batch.h:231-257).
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only enqueue
 *    work; they never synchronise and never allocate device memory.  Temporaries come from a
 *    caller-supplied workspace (size from the matching *_workspace_bytes query), which is how
 *    the reference's MemoryPool plugs in.
 *  - return value: 0 = success; > 0 = hipError_t from the runtime; < 0 = TROYN_E_* below.
 *    troyn_last_error() returns a thread-local message (the C++ mirror turns negative codes
 *    into std::invalid_argument and positive codes into std::runtime_error, matching
 *    kernel_provider.h:11-16 and the reference's "[Class::method] ..." messages).
 */
#ifndef TROYN_H
#define TROYN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TROYN_VERSION 1

enum {
    TROYN_OK = 0,
    TROYN_E_INVALID = -1,     /* bad argument (sizes, null pointers, unsupported N) */
    TROYN_E_MODULUS = -2,     /* modulus not usable (not < 2^61, no 2N-th root, not coprime) */
    TROYN_E_WORKSPACE = -3,   /* workspace too small */
    TROYN_E_UNSUPPORTED = -4  /* scheme / shape not implemented */
};

typedef void* troyn_stream_t;
typedef struct troyn_plan troyn_plan;
typedef struct troyn_behz troyn_behz;

const char* troyn_last_error(void);
int troyn_version(void);

/* Measurement hook (the reference times its kernels with bench::Timer around whole calls, test/bench/he_operations.cu:57-104;
 * a fused call here contains several launches, so the library can bracket ONE named launch with hipEvents on the launch stream).
 *   troyn_kernel_timer_enable(region, on)   start / stop recording an event pair around every launch of that region
 *   troyn_kernel_timer_read(region, &ms, &n) wait for the recorded events, return their summed duration and count, and clear
 * Region TROYN_TIMER_KS_INNER_PRODUCT = the fused key-switch inner product (kernel_set_accumulate + ntt +
 * kernel_accumulate_products of fgk/switch_key.cu, one launch here);
 * TROYN_TIMER_BFV_TENSOR = the transform + tensor-product launches of bfv_multiply (ntt_inplace_ps x2 + kernel_dyadic_convolute +
 * intt_inplace_ps, evaluator.cu:56-93; one launch per base and arithmetic class here);
 * TROYN_TIMER_PLAIN_MAC = the ct x pt multiply-accumulate launch (multiply_plain_ntt_accumulate, evaluator_multiply_plain.cu:356-385);
 * TROYN_TIMER_BEHZ_FLOOR = fast_floor_fast_b_conv_sk (fgk/rns_tool.cu:147-343). */
enum { TROYN_TIMER_KS_INNER_PRODUCT = 0, TROYN_TIMER_BFV_TENSOR = 1, TROYN_TIMER_PLAIN_MAC = 2, TROYN_TIMER_BEHZ_FLOOR = 3, TROYN_TIMER_REGIONS = 4 };
int troyn_kernel_timer_enable(int region, int on);
int troyn_kernel_timer_read(int region, double* total_ms, uint64_t* launches);

/* Host-only helpers (no GPU touched) so that a host can build the same parameter sets as the
 * reference: CoeffModulus::create (coeff_modulus.cu:65-108: for every bit size the k largest primes
 * = 1 mod 2N, handed out smallest-first) and utils::get_primes (utils/number_theory.cu:22-39). */
int troyn_coeff_modulus_create(size_t poly_modulus_degree, const size_t* bit_sizes, size_t n, uint64_t* out);
int troyn_get_primes(uint64_t factor, size_t bit_size, size_t count, uint64_t* out);

/* ---------------------------------------------------------------------------------------
 * Plan = device-resident mirror of one modulus chain: for each of the `n_moduli` primes
 * (key level order, special prime last) the Modulus constants (modulus.h:8-124), the
 * NTTTables (utils/ntt.h:12-87, built exactly as utils/ntt.cu:14-76 does: minimal primitive
 * 2N-th root, bit-reversed psi powers, scrambled inverse powers, N^-1) and, for every level
 * L <= n_moduli, q_{L-1}^-1 mod q_i (RNSTool::inv_q_last_mod_q, utils/rns_tool.cu:225-236).
 * Replaces ContextData::to_device_inplace (context_data.cu:34-69).
 * `roots` may be NULL (roots are then searched as number_theory.cu:68-87 does) or hold the
 * reference's NTTTables::root() per modulus.
 * ------------------------------------------------------------------------------------- */
int troyn_plan_create(troyn_plan** plan, int device, uint32_t log_n, uint32_t n_moduli,
                      const uint64_t* moduli, const uint64_t* roots);
int troyn_plan_destroy(troyn_plan* plan);
/* A/B switches (DESIGN.md section 4 "A/B switches"): read from the environment variables of the same names ONCE, when the plan is created;
 * this sets one of them on an existing plan ("TROYN_KS_ORDER", "row"; value NULL or "" = the default).  The library never reads the
 * environment on a call path.  Not to be called while other threads use the plan.  Replaces nothing in the reference (development hook). */
int troyn_plan_set_option(troyn_plan* plan, const char* name, const char* value);
uint32_t troyn_plan_log_n(const troyn_plan* plan);
uint32_t troyn_plan_n_moduli(const troyn_plan* plan);
/* host copies of table contents, for known-answer checks: out[2*i] = operand, out[2*i+1] = quotient */
int troyn_plan_get_root(const troyn_plan* plan, uint32_t modulus_index, uint64_t* root);
int troyn_plan_get_root_powers(const troyn_plan* plan, uint32_t modulus_index, int inverse, uint64_t* out);

/* NTTTableIndexer modes (utils/ntt.h:89-130) */
enum { TROYN_IDX_COMPONENTWISE = 0, TROYN_IDX_KS_SET_PRODUCTS = 1, TROYN_IDX_KS_SKIP_FINALS = 2 };

/* ---------------------------------------------------------------------------------------
 * troyn_ntt: negacyclic NTT (inverse = 0; natural -> bit-reversed, canonical output) or INTT
 * (inverse = 1; includes the N^-1 scaling) of batch*pcount*ncomp limb-polynomials.
 * Replaces the device branches of fgk::ntt_grouped::ntt / intt (fgk/ntt_grouped.cu:258-295,
 * :597-640) and their _batched forms, i.e. utils::ntt_ps / intt_ps / *_inplace_* /
 * *_b* (utils/ntt.h:164-391).  in == out is allowed.  Component j of polynomial k uses table
 * `table_start + get(k, j)` where get() is NTTTableIndexer::get over a slice of
 * `table_count` tables (utils/ntt.h:105-124).
 * ------------------------------------------------------------------------------------- */
int troyn_ntt(const troyn_plan* plan, int inverse, const uint64_t* in, uint64_t* out,
              size_t batch, size_t pcount, size_t ncomp,
              uint32_t table_start, uint32_t table_count, int indexer_mode, uint32_t decomp_size,
              troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Element-wise RNS polynomial ops over count*nmod limb-polynomials ([count][nmod][N]); limb l
 * uses modulus mod_start + l.  Replace the device branches of utils::add_ps / sub_ps /
 * negate_ps / multiply_scalar_ps / dyadic_product_ps / modulo_ps / multiply_uint64operand_ps
 * (utils/poly_small_mod.cu:243-304, :306-365, :182-241, :653-714, :816-900, :119-180, :752-814).
 * troyn_modulo: Modulus::reduce (Barrett-64, modulus.h:22-42) of ANY 64-bit word.
 * troyn_multiply_uint64operand: `operands` = nmod device-resident (operand, quotient) pairs, one
 * MultiplyUint64Operand (utils/uint_small_mod.h:92-122) per limb of the slice; the input may be any
 * 64-bit word, the result is canonical (multiply_uint64operand_mod, :130-139).
 * ------------------------------------------------------------------------------------- */
int troyn_add(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* a, const uint64_t* b,
              uint64_t* out, size_t count, troyn_stream_t stream);
int troyn_sub(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* a, const uint64_t* b,
              uint64_t* out, size_t count, troyn_stream_t stream);
int troyn_negate(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* a,
                 uint64_t* out, size_t count, troyn_stream_t stream);
int troyn_multiply_scalar(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* a, uint64_t scalar,
                          uint64_t* out, size_t count, troyn_stream_t stream);
int troyn_dyadic_product(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* a, const uint64_t* b,
                         uint64_t* out, size_t count, troyn_stream_t stream);
int troyn_modulo(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* a,
                 uint64_t* out, size_t count, troyn_stream_t stream);
int troyn_multiply_uint64operand(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* a,
                                 const uint64_t* operands, uint64_t* out, size_t count, troyn_stream_t stream);

/* fgk::dyadic_convolute::dyadic_convolute (fgk/dyadic_convolute.cu:43-90): a[pa][nmod][N] x
 * b[pb][nmod][N] -> out[pa+pb-1][nmod][N], per batch item.  CKKS/BGV multiply is exactly this
 * (evaluator.cu:118-173). */
int troyn_dyadic_convolute(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod,
                           const uint64_t* a, size_t pa, const uint64_t* b, size_t pb, uint64_t* out,
                           size_t batch, troyn_stream_t stream);
/* fgk::dyadic_convolute::dyadic_square (fgk/dyadic_convolute.cu:116-150) */
int troyn_dyadic_square(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod,
                        const uint64_t* a, uint64_t* out, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Key switching core: Evaluator::switch_key_internal(_batched)
 * (evaluator_keyswitching_core.cu:757-1052, :1055-1267), device branch, BFV/CKKS.
 *   L            decomposition size = limbs of the data level (L <= n_moduli - 1)
 *   target       [batch][L][N]   polynomial to switch (NTT form iff is_ntt_form)
 *   keys         host array of L DEVICE pointers, keys[j] -> u64[2][K][N] in NTT form
 *                (KSwitchKeys::get_data_ptrs, kswitch_keys.h:34-54); shared by the batch
 *   destination  [batch][2][L][N], written or accumulated per `assign_method`
 *                (SwitchKeyDestinationAssignMethod, evaluator.h)
 *   workspace    query it with the batch the call will use: small launches (a single ciphertext) take the digit-parallel
 *                inner product (one workgroup per digit on the caller's own keys, no key preparation pass), whose slots are
 *                part of the workspace; the result words do not depend on which form runs
 * ------------------------------------------------------------------------------------- */
enum { TROYN_ASSIGN_ADD_INPLACE = 0, TROYN_ASSIGN_OVERWRITE = 1, TROYN_ASSIGN_OVERWRITE_EXCEPT_FIRST = 2 };
size_t troyn_switch_key_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t batch);
int troyn_switch_key(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form,
                     const uint64_t* target, const uint64_t* const* keys, int assign_method,
                     uint64_t* destination, void* workspace, size_t workspace_bytes,
                     size_t batch, troyn_stream_t stream);

/* Evaluator::relinearize_internal for a 3-polynomial ciphertext (evaluator_keyswitching.cu:
 * 119-144): ct[batch][3][L][N] -> out[batch][2][L][N] = switch_key(ct[2], Overwrite) + ct[0..2). */
size_t troyn_relinearize_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t batch);
int troyn_relinearize(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form,
                      const uint64_t* ct3, const uint64_t* const* keys, uint64_t* out2,
                      void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fused CKKS chain: Evaluator::multiply (evaluator.cu:118-145) -> Evaluator::relinearize (evaluator_keyswitching.cu:119-144)
 * -> Evaluator::rescale_to_next (evaluator_modswitch.cu, RNSTool::divide_and_round_q_last_ntt utils/rns_tool.cu:499-694) of
 * `batch` ciphertext pairs in one call.  Results are bit-identical to troyn_dyadic_convolute + troyn_relinearize +
 * troyn_divide_and_round_q_last_ntt; on whole-limb FP64 rings (N = 8192 / 16384, moduli < 2^50) the tensor product is formed
 * inside the loaders of the transforms that consume it and the rounding steps of the key switch and of the rescale share one
 * forward transform per output limb; other shapes run the three calls.
 *   a, b  [batch][2][L][N] NTT form;  keys as troyn_switch_key;  out [batch][2][L-1][N] NTT form
 * ------------------------------------------------------------------------------------- */
size_t troyn_ckks_multiply_relinearize_rescale_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t batch);
int troyn_ckks_multiply_relinearize_rescale(const troyn_plan* plan, uint32_t L, const uint64_t* a, const uint64_t* b,
                                            const uint64_t* const* keys, uint64_t* out, void* workspace, size_t workspace_bytes,
                                            size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Dot product of ciphertexts with lazy relinearization.  Both entries are ADDITIONS to the reference's surface (as the fused chain above):
 * a sum of `terms` products pays one key switch and one rescale instead of one per term.
 *
 * troyn_dyadic_convolute_accumulate: out (+)= SUM_t a[t] (x) b[t], the two-by-two tensor product of Evaluator::multiply
 * (evaluator.cu:118-145) summed over the terms in ONE pass: every input word is read once, every output word written once, one
 * Barrett reduction per output word.
 *   a, b   host arrays of `terms` DEVICE pointers, each -> u64[batch][2][nmod][N] in NTT form, 16-byte aligned; limb l under modulus
 *          mod_start + l
 *   out    [batch][3][nmod][N]; accumulate = 0 overwrites it, accumulate = 1 adds to it (it must hold canonical residues)
 * Contract: the words are bit-identical to `terms` x troyn_dyadic_convolute folded with troyn_add (the sum modulo each q_l in canonical
 * form does not depend on where the reductions happen).  TROYN_E_INVALID: terms == 0, a null table or entry, a misaligned pointer, a
 * modulus slice outside the plan, `out` overlapping an input.  batch == 0 returns TROYN_OK and launches nothing.  The tables are read
 * before the call returns (they travel in the kernel arguments, 32 terms per launch; longer sums run as successive launches).
 *
 * troyn_ckks_multiply_accumulate_relinearize_rescale: rescale_to_next(relinearize(SUM_t multiply(a[t], b[t]))) -- the accumulated product
 * into the workspace, then the drivers of troyn_relinearize (evaluator_keyswitching.cu:119-144) and troyn_divide_and_round_q_last_ntt
 * (utils/rns_tool.cu:499-694) on it.
 *   a, b as above with nmod = L;  keys as troyn_switch_key;  out [batch][2][L-1][N] NTT form
 * Contract: bit-identical to troyn_dyadic_convolute_accumulate + troyn_relinearize + troyn_divide_and_round_q_last_ntt, hence with
 * terms = 1 to troyn_ckks_multiply_relinearize_rescale.  Errors as above, TROYN_E_WORKSPACE for a workspace below the queried size;
 * batch == 0 returns TROYN_OK, launches nothing and looks at neither `out` nor the workspace (both may be null).
 * ------------------------------------------------------------------------------------- */
int troyn_dyadic_convolute_accumulate(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod,
                                      const uint64_t* const* a, const uint64_t* const* b, size_t terms,
                                      uint64_t* out, int accumulate, size_t batch, troyn_stream_t stream);
size_t troyn_ckks_multiply_accumulate_relinearize_rescale_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t terms, size_t batch);
int troyn_ckks_multiply_accumulate_relinearize_rescale(const troyn_plan* plan, uint32_t L,
                                                       const uint64_t* const* a, const uint64_t* const* b, size_t terms,
                                                       const uint64_t* const* keys, uint64_t* out, void* workspace, size_t workspace_bytes,
                                                       size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Product plus affine part, relinearized and rescaled: the Chebyshev recurrence T_{a+b} = 2 T_a T_b - T_{a-b} and the double angle
 * cos 2t = 2 cos^2 t - 1 as ONE step.  An ADDITION to the reference's surface, on the accumulate -> relinearize -> rescale driver path of
 * troyn_ckks_multiply_accumulate_relinearize_rescale above.  For each item i < batch
 *   P_0 = alpha_i (a0 . b0) + w_i c0 + k_i          (k_i at every index: a constant in NTT form)
 *   P_1 = alpha_i (a0 . b1 + a1 . b0) + w_i c1
 *   P_2 = alpha_i (a1 . b1)
 *   out_i = divide_and_round_q_last_ntt( relinearize( P ) )
 * all modulo q_l in canonical form, on limbs 0 .. L-1.
 *   a, b, c    host arrays of `batch` DEVICE pointers (the form of troyn_dyadic_convolute_accumulate: the operands of a ladder live in
 *              separate ciphertexts, there is no gather).  a[i], b[i] -> u64[2][L][N] in NTT form; c[i] -> u64[2][c_nmod[i]][N] with
 *              c_nmod[i] >= L, of which only the first L limbs are read, or NULL: then there is no addend and w_i is ignored.
 *              Every pointer 16-byte aligned.
 *   alpha, weight, constant   host [batch][L], canonical residues (word < q_l); `constant` may be NULL
 *   keys       as for troyn_switch_key
 *   out        [batch][2][L-1][N] in NTT form, 16-byte aligned
 * Contract on integers: P_c[l][j] = ( alpha_i[l] * conv_c(a, b)[l][j] + (c < 2 and c[i] ? w_i[l] * c_c[l][j] : 0) + (c == 0 ? k_i[l] : 0) )
 * mod q_l with conv = troyn_dyadic_convolute's tensor product.  Hence the result is bit-identical to this sequence per item:
 * troyn_dyadic_convolute, troyn_multiply_scalar by alpha, troyn_multiply_scalar and troyn_add of the addend, the constant,
 * troyn_relinearize, troyn_divide_and_round_q_last_ntt -- the sum modulo q does not depend on where the reductions happen.
 * P is formed in the workspace in ONE pass: each word of a, b and c is read once, each word of P written once.
 * TROYN_E_INVALID: L < 2 (or no next level), a null table, a null a[i] or b[i], a misaligned pointer, c_nmod[i] < L, a scalar word >= its
 * modulus, `out` (or the workspace) overlapping an input, `out` overlapping the workspace.  TROYN_E_WORKSPACE for a workspace below the queried size.  batch == 0 returns
 * TROYN_OK, launches nothing and looks at no buffer.  The host tables are read before the call returns: the scalars go through one upload
 * into the workspace, the pointers and limb counts travel in the kernel arguments (32 items per launch).
 * ------------------------------------------------------------------------------------- */
size_t troyn_ckks_multiply_affine_relinearize_rescale_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t batch);
int troyn_ckks_multiply_affine_relinearize_rescale(const troyn_plan* plan, uint32_t L, const uint64_t* const* a, const uint64_t* const* b,
                                                   const uint64_t* const* c, const uint32_t* c_nmod, const uint64_t* alpha,
                                                   const uint64_t* weight, const uint64_t* constant, const uint64_t* const* keys,
                                                   uint64_t* out, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Scalar-weighted sums of ciphertexts: a small dense matrix of residues times a vector of ciphertexts in ONE pass.  An ADDITION to the
 * reference's surface (as the dot-product block above): the step between the powers and the recombination of a polynomial evaluation,
 * SUM_t s_t * ct_t + c, which is otherwise `terms` x (troyn_multiply_scalar + troyn_add) per output.
 *   in         host array of `terms` DEVICE pointers, in[t] -> u64[batch][pcount][in_nmod[t]][N], 16-byte aligned
 *   in_nmod    host, in_nmod[t] >= nmod: only the first nmod limbs of every input are read (dropping limbs in RNS is ignoring them, so
 *              inputs at a higher level than the output need no troyn_mod_switch_drop first)
 *   scalars    host [slots][terms][nmod], canonical residues (word < q_{mod_start+l})
 *   constants  host [slots][nmod] canonical residues, or NULL
 *   constant_at_index0   0: the constant is added at every index of polynomial 0 (a constant in NTT form); 1: at index 0 only
 *              (coefficient form).  Apart from this flag the entry does not look at the form: it is scheme-agnostic RNS arithmetic.
 *   out        [slots][batch][pcount][nmod][N], 16-byte aligned
 * Contract on integers:
 *   out[s][b][c][l][i] = ( SUM_t scalars[s][t][l] * in[t][b][c][l][i] + (c == 0 and (i == 0 or !constant_at_index0) ? constants[s][l] : 0) )
 *                        mod q_{mod_start+l}, in canonical form.
 * Hence the words are bit-identical to folding troyn_multiply_scalar and troyn_add (plus the constant) term by term: the sum modulo q does
 * not depend on where the reductions happen.  Every input is read once per tile of up to 8 slots, every output word is written once after
 * one Barrett reduction; sums of more than 64 terms run as successive launches that carry `out` (64 products of residues below 2^61
 * plus a canonical carry stay below 2^128), the words do not depend on the cut.
 * TROYN_E_INVALID: terms == 0, slots == 0 or pcount == 0, a null table or entry, a misaligned pointer, in_nmod[t] < nmod, a modulus slice
 * outside the plan, a scalar or constant word >= its modulus, `out` overlapping an input.  TROYN_E_WORKSPACE for a workspace below the
 * queried size.  batch == 0 returns TROYN_OK, launches nothing and looks at no buffer (`out` and the workspace may be null).  The host
 * tables are read before the call returns: the scalars and constants go through one upload into the workspace, the pointers and limb
 * counts travel in the kernel arguments.
 * ------------------------------------------------------------------------------------- */
size_t troyn_scalar_weighted_sums_workspace_bytes(const troyn_plan* plan, uint32_t nmod, size_t terms, size_t slots);
int troyn_scalar_weighted_sums(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod,
                               const uint64_t* const* in, const uint32_t* in_nmod, size_t terms,
                               const uint64_t* scalars, const uint64_t* constants, int constant_at_index0,
                               size_t pcount, uint64_t* out, size_t slots, size_t batch,
                               void* workspace, size_t workspace_bytes, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Modulus switching.
 * troyn_divide_and_round_q_last      RNSTool::divide_and_round_q_last (utils/rns_tool.cu:374-466),
 *                                    BFV mod_switch_to_next, coefficient form.
 * troyn_divide_and_round_q_last_ntt  RNSTool::divide_and_round_q_last_ntt (utils/rns_tool.cu:499-694),
 *                                    CKKS rescale_to_next, NTT form.
 * troyn_mod_switch_drop              kernel_mod_switch_drop_to (evaluator_modswitch.cu:164-171).
 * in [batch][pcount][L][N] -> out [batch][pcount][L-1][N] (drop: [L_out]).
 * ------------------------------------------------------------------------------------- */
int troyn_divide_and_round_q_last(const troyn_plan* plan, uint32_t L, const uint64_t* in, size_t pcount,
                                  uint64_t* out, size_t batch, troyn_stream_t stream);
size_t troyn_divide_and_round_q_last_ntt_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t pcount, size_t batch);
int troyn_divide_and_round_q_last_ntt(const troyn_plan* plan, uint32_t L, const uint64_t* in, size_t pcount,
                                      uint64_t* out, void* workspace, size_t workspace_bytes,
                                      size_t batch, troyn_stream_t stream);
int troyn_mod_switch_drop(const troyn_plan* plan, uint32_t L_in, uint32_t L_out, const uint64_t* in, size_t pcount,
                          uint64_t* out, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Callers either side of the evaluator path, kept on the device:
 *
 * Context PRNG = AES-128 in counter mode (utils/random_generator.cu:37-58,:112-117): key = seed[2]
 * (low, high), block i = AES(counter + i).  The samplers write `nmod` limbs (the first nmod plan
 * moduli) of one polynomial and report how many blocks they consumed so the caller can advance its
 * counter exactly like RandomGenerator does:
 *   troyn_sample_ternary            RandomGenerator::sample_poly_ternary            (:318-336)  ceil(N/16) blocks
 *   troyn_sample_centered_binomial  RandomGenerator::sample_poly_centered_binomial  (:421-440)  ceil(N/2)  blocks
 *   troyn_sample_uniform            RandomGenerator::sample_poly_uniform            (:475-481)  ceil(nmod*N/2) blocks
 *   troyn_sample_ternary_sparse     (not in the reference)                         N/2        blocks
 *   troyn_prng_block                host_generate_uint128 (:112-117), host only: sample_uint64() = out[0]
 *
 * troyn_sample_ternary_sparse draws a ternary polynomial of EXACTLY `hamming_weight` nonzero coefficients (the same
 * polynomial in every limb, -1 stored as q_i - 1), reproducible from the seed:
 *   stream   word w_j, j = 0 .. N-1, is word j & 1 of block counter + (j >> 1) (the word order of
 *            troyn_sample_centered_binomial); *blocks_used = N/2
 *   key      key_j = (w_j & ~0xFFFF) | j: 48 random bits above the index, so keys are distinct (N <= 65536)
 *   support  the `hamming_weight` coefficients with the smallest keys are nonzero
 *   sign     bit 0 of w_j: 0 -> +1, 1 -> -1
 * One workgroup, no workspace: row 0 of `out` (16-byte aligned) stages the keys while the call runs.
 * TROYN_E_INVALID "[RandomGenerator::sample_poly_ternary_sparse] ..." for hamming_weight == 0 or > N, nmod out of
 * range, a null pointer, N > 65536 or a misaligned `out`.
 * ------------------------------------------------------------------------------------- */
int troyn_prng_block(const uint64_t seed[2], uint64_t counter, uint64_t out[2]);
int troyn_sample_ternary(const troyn_plan* plan, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint64_t* out,
                         uint64_t* blocks_used, troyn_stream_t stream);
int troyn_sample_ternary_sparse(const troyn_plan* plan, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint32_t hamming_weight,
                                uint64_t* out, uint64_t* blocks_used, troyn_stream_t stream);
int troyn_sample_centered_binomial(const troyn_plan* plan, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint64_t* out,
                                   uint64_t* blocks_used, troyn_stream_t stream);
int troyn_sample_uniform(const troyn_plan* plan, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint64_t* out,
                         uint64_t* blocks_used, troyn_stream_t stream);
/* batched forms (one launch for `count` polynomials, out[count][nmod][N]):
 *   _strided: polynomial i continues the SAME generator at counter + i*counter_stride -- the positions `count`
 *             sequential encryptions would have used (each consumes ceil(N/2) blocks here plus whatever else it draws);
 *   _multi:   polynomial i comes from its own generator seeds[2i], seeds[2i+1] at counter 0 (the per-ciphertext
 *             c1 generators of rlwe::symmetric, utils/rlwe.cu:262-266). */
int troyn_sample_centered_binomial_strided(const troyn_plan* plan, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint64_t counter_stride,
                                           uint64_t* out, size_t count, troyn_stream_t stream);
int troyn_sample_uniform_multi(const troyn_plan* plan, uint32_t nmod, const uint64_t* seeds, uint64_t* out, size_t count, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Ciphertext x plaintext (the BASELINE config 5 matmul path):
 *   troyn_plain_centralize        scaling_variant::centralize (utils/scaling_variant.cu:326-357, fast-plain-lift case):
 *                                 plain[batch][count] mod t -> dest[batch][L][N], ready for the forward NTT
 *                                 (Evaluator::transform_plain_to_ntt, evaluator_transform_ntt.cu:35-70)
 *   troyn_dyadic_broadcast_product fgk::dyadic_convolute::dyadic_broadcast_product_ps (fgk/dyadic_convolute.cu:173-195):
 *                                 out[b][p][l] = ct[b][p][l] (.) pt[b][l]; pt_bstride = 0 shares one plaintext
 *   troyn_multiply_plain_accumulate Evaluator::multiply_plain_ntt_accumulate (evaluator_multiply_plain.cu:258-307):
 *                                 dst[k] (+)= ct[k] (.) pt[k] over `count` triples of device pointers (host arrays);
 *                                 equal dst pointers accumulate; set_zero != 0 overwrites instead of adding to dst.
 * ------------------------------------------------------------------------------------- */
int troyn_plain_centralize(const troyn_plan* plan, uint32_t L, uint64_t plain_modulus, const uint64_t* plain, size_t plain_coeff_count,
                           size_t plain_bstride, uint64_t* dest, size_t batch, troyn_stream_t stream);
/* Evaluator::transform_plain_to_ntt (evaluator_transform_ntt.cu:35-70) as ONE launch: scaling_variant::centralize (utils/scaling_variant.cu:326-357) in the
 * loader of the forward transform -- dest[batch][L][N] = NTT_j(centralize_j(plain[b])), the words troyn_plain_centralize + troyn_ntt give; the centred
 * coefficient-form polynomial is never written and the zeros beyond plain_coeff_count are never read.  (Falls back to the two launches where the fused loader
 * does not apply: N < 1024, or t not below every modulus.) */
int troyn_plain_centralize_ntt(const troyn_plan* plan, uint32_t L, uint64_t plain_modulus, const uint64_t* plain, size_t plain_coeff_count,
                               size_t plain_bstride, uint64_t* dest, size_t batch, troyn_stream_t stream);
int troyn_dyadic_broadcast_product(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* ct, size_t pcount,
                                   const uint64_t* pt, size_t pt_bstride, uint64_t* out, size_t batch, troyn_stream_t stream);
/* Galois automorphism X -> X^g of `count` polynomials of nmod limbs each:
 * GaloisTool::apply_ps (coefficient form, utils/galois.cu:168-206) / apply_ntt_ps (NTT form, :24-41,:250-343).
 * Out of place (in != out).  Evaluator::apply_galois = this permutation of (c0, c1) followed by troyn_switch_key on
 * the permuted c1 with TROYN_ASSIGN_OVERWRITE_EXCEPT_FIRST (evaluator_keyswitching.cu:147-179). */
int troyn_apply_galois(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, int is_ntt_form, uint64_t galois_element,
                       const uint64_t* in, uint64_t* out, size_t count, troyn_stream_t stream);
/* GaloisTool::apply (utils/galois.cu:43-66) on `count` coefficient-form polynomials [N] modulo ONE explicit modulus -- the plain
 * modulus t of a BFV / BGV plaintext (Evaluator::apply_galois_plain, evaluator_keyswitching.cu:235-261). */
int troyn_apply_galois_plain(const troyn_plan* plan, uint64_t modulus, uint64_t galois_element, const uint64_t* in, uint64_t* out, size_t count,
                             troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Hoisted rotations: many Galois keys applied to ONE ciphertext with one digit decomposition.  Both entries are ADDITIONS to the
 * reference's surface (the reference applies one automorphism and one complete key switch per rotation, evaluator_keyswitching.cu:147-179).
 *   ct               [batch][2][L][N] = (c0, c1), NTT form iff is_ntt_form (CKKS: NTT form, BFV: coefficient form, as troyn_switch_key)
 *   galois_elements  host array of `terms` elements g_t, each odd with 1 < g_t < 2N; duplicates are allowed
 *   keys             host array of terms * L DEVICE pointers, keys[t * L + j] -> u64[2][K][N] in NTT form (the Galois key of g_t), 16-byte aligned
 *   out              many: [terms][batch][2][L][N], one ciphertext per term;  sum: [batch][2][L][N];  same form as ct
 * Contract, per item, on integers (tests/hoist_spec.py; the notation of tests/ks_spec.py):
 *   d_j          limb j of c1 in coefficient form, an integer in [0, q_j)
 *   sigma_g      (sigma_g x)[i * g mod N] = (-1)^floor(i * g / N) x[i]
 *   e_{t,j}      sigma_{g_t}(d_j), signed coefficients in (-q_j, q_j)
 *   X_c[m]       SUM_{t in S} SUM_j (e_{t,j} mod m) (*) k_{t,j}[c][m]  mod m   for every key modulus m in {q_0 .. q_{L-1}, q_special}
 *   r_c, result_c[l] = (X_c[q_l] - r_c) * q_special^-1 mod q_l   exactly as in troyn_switch_key (ONE rounded division by the special prime)
 *   out[0][l] = SUM_{t in S} sigma_{g_t}(c0)[l] + result_0[l]  mod q_l,   out[1][l] = result_1[l]
 * many: S = {t}, one output per term -- one decomposition, `terms` tails.  sum: S = every term -- one decomposition, ONE tail.
 * With terms = 1 the words are NOT bit-identical to troyn_apply_galois + troyn_switch_key: the words differ from apply_galois.  Where the
 * automorphism negates a coefficient x of d_j, the reference decomposes sigma(c1) afresh and its digit under key modulus m is
 * (q_j - x) mod m; the hoisted digit is (-x) mod m.  The two agree for m = q_j and differ by a multiple of q_j on the other rows.  Both
 * are key switches with digits bounded by q_j in magnitude, so both decrypt to the same message under the same noise bound; the
 * contract is the integer specification above, not the reference's words.
 * Scope: BFV and CKKS.  BGV is left out (its tail divides differently, troyn_bgv_switch_key).
 * BGV has entries of its own with the same arguments: troyn_bgv_apply_galois_many / _sum in the hoisted BGV block below.
 * TROYN_E_INVALID: terms == 0, a null table or entry, a misaligned pointer, an element that is even, 1 or >= 2N, L outside [1, K-1],
 * `out` overlapping `ct`.  TROYN_E_WORKSPACE: a workspace below troyn_apply_galois_hoisted_workspace_bytes(plan, L, terms, batch, sum)
 * (sum = 0 for _many, 1 for _sum).  batch == 0 returns TROYN_OK, launches nothing and looks at neither `ct`, `out` nor the workspace.  The
 * tables are read before the call returns.
 * ------------------------------------------------------------------------------------- */
size_t troyn_apply_galois_hoisted_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t terms, size_t batch, int sum);
int troyn_apply_galois_many(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct,
                            const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms, uint64_t* out,
                            void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);
int troyn_apply_galois_sum(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct,
                           const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms, uint64_t* out,
                           void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Plaintext-weighted hoisted rotations: out[s] = SUM_t w_{s,t} (.) rot_t(ct), the diagonal method of a plaintext matrix times an
 * encrypted vector (with baby-step/giant-step: several such sums over the same rotations of one ciphertext).  An ADDITION to the
 * reference's surface, built on the hoisted entries above: one digit decomposition per ciphertext, ONE division by the special prime
 * per slot -- the weight is applied BEFORE the division, on the extended basis q_0 .. q_{L-1}, q_special.
 *   ct               [batch][2][L][N], NTT form iff is_ntt_form (CKKS: NTT form, BFV: coefficient form, as troyn_switch_key)
 *   galois_elements  host array of `terms` elements g_t, each odd and < 2N; duplicates are allowed.  The element 1 IS allowed here: the
 *                    unrotated ciphertext (the main diagonal); its L key entries are ignored and may be NULL
 *   keys             host array of terms * L DEVICE pointers, keys[t * L + j] -> u64[2][K][N] in NTT form, 16-byte aligned
 *   weights          host array of slots * terms DEVICE pointers, weights[s * terms + t] -> u64[K][N] in NTT form and KEY-LEVEL layout:
 *                    rows 0 .. K-2 under q_0 .. q_{K-2}, row K-1 under the special prime; only rows 0 .. L-1 and K-1 are read; words are
 *                    canonical (below their modulus); 16-byte aligned; NULL = the term is absent from that slot.  Shared by the batch.
 *   out              [slots][batch][2][L][N], same form as ct
 * Contract, per item and slot s, on integers (tests/weighted_hoist_spec.py; the notation of the block above).  T_s = {t : weight (s, t)
 * non-NULL}; (*) is the negacyclic product = the pointwise product of the NTT-form words as given:
 *   e_{t,j}      sigma_{g_t}(d_j), signed
 *   X_c[m]       SUM_{t in T_s, g_t != 1} w_{s,t}[m] (*) SUM_j (e_{t,j} mod m) (*) k_{t,j}[c][m]  mod m,  m in {q_0 .. q_{L-1}, q_special}
 *   r_c, result_c[l]   exactly as in troyn_switch_key (ONE rounded division by the special prime per slot)
 *   out[s][0][l] = SUM_{t in T_s}          w_{s,t}[q_l] (*) sigma_{g_t}(c0)[l] + result_0[l]  mod q_l
 *   out[s][1][l] = SUM_{t in T_s, g_t = 1} w_{s,t}[q_l] (*) c1[l]              + result_1[l]  mod q_l
 * The unkeyed contributions y (c0 of every term, c1 of the identity terms) may be added after the division, as written, or injected
 * before it as (q_special mod q_l) * y on the rows q_l and nothing on the special row; the output WORDS are the same either way: the
 * special row and hence r_c is unchanged, and ((X + q_special * y) - r) * q_special^-1 = (X - r) * q_special^-1 + y  mod q_l.  The
 * implementation injects before the division (one tail with TROYN_ASSIGN_OVERWRITE serves both components and both forms).
 * With every weight the constant 1 and no identity term the words equal troyn_apply_galois_sum's.  As stated above, the words are NOT
 * those of troyn_apply_galois + troyn_switch_key + a plaintext multiplication: the digits of a negated coefficient differ by multiples
 * of q_j, and the reference would round once per term; both decrypt to the same message under the same kind of noise bound.
 * Scope: BFV and CKKS.  BGV is left out (its tail divides differently).
 * BGV has an entry of its own with the same arguments: troyn_bgv_apply_galois_weighted_sums in the hoisted BGV block below.
 * TROYN_E_INVALID: terms == 0, slots == 0, a slot with no weight, a null table, a null or misaligned key entry of a term with g != 1, a
 * misaligned pointer (ct, out, workspace, a weight), an element that is even or >= 2N, L outside [1, K-1], `out` overlapping `ct`.
 * TROYN_E_WORKSPACE: a workspace below troyn_apply_galois_weighted_workspace_bytes(plan, L, terms, slots, batch, is_ntt_form).
 * batch == 0 returns TROYN_OK, launches nothing and looks at neither `ct`, `out` nor the workspace.  The tables are read before the
 * call returns.
 * ------------------------------------------------------------------------------------- */
size_t troyn_apply_galois_weighted_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t terms, size_t slots, size_t batch, int is_ntt_form);
int troyn_apply_galois_weighted_sums(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct,
                                     const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms,
                                     const uint64_t* const* weights, size_t slots, uint64_t* out,
                                     void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The sum of key-switched automorphisms of DIFFERENT ciphertexts, and the baby-step/giant-step (BSGS) linear transform on top of it.  Both
 * entries are ADDITIONS to the reference's surface, built on the two blocks above.
 *
 * troyn_apply_galois_sum_each: out = SUM_t sigma_{g_t}(cts[t]) with ONE division by the special prime.
 *   cts              [terms][batch][2][L][N], one ciphertext PER TERM (exactly the layout of troyn_apply_galois_weighted_sums' `out`),
 *                    NTT form iff is_ntt_form
 *   galois_elements  host array of `terms` elements g_t, each odd and < 2N; duplicates are allowed.  The element 1 IS allowed: the term is
 *                    added unrotated; its L key entries are ignored and may be NULL
 *   keys             host array of terms * L DEVICE pointers, keys[t * L + j] -> u64[2][K][N] in NTT form, 16-byte aligned
 *   out              [batch][2][L][N], same form as cts
 * Contract, per item, on integers (tests/bsgs_spec.py; the notation of the two blocks above):
 *   d_{t,j}      limb j of c1 of term t in coefficient form, an integer in [0, q_j)
 *   e_{t,j}      sigma_{g_t}(d_{t,j}), signed
 *   X_c[m]       SUM_{t, g_t != 1} SUM_j (e_{t,j} mod m) (*) k_{t,j}[c][m]  mod m,  m in {q_0 .. q_{L-1}, q_special}
 *   r_c, result_c[l]   exactly as in troyn_switch_key (ONE rounded division by the special prime)
 *   out[0][l] = SUM_t            sigma_{g_t}(c0_t)[l] + result_0[l]  mod q_l
 *   out[1][l] = SUM_{t, g_t = 1} c1_t[l]              + result_1[l]  mod q_l
 * The unkeyed contributions y (c0 of every term, c1 of the identity terms) may be added after the division, as written, or injected
 * before it as (q_special mod q_l) * y on the rows q_l and nothing on the special row; the WORDS are the same either way (the argument of
 * the block above).  The implementation injects before the division, in both forms: in coefficient form (BFV) after one forward
 * transform of the terms' c0 into the workspace.  With every cts[t] the same ciphertext and no identity term the words equal
 * troyn_apply_galois_sum's; with only identity terms the result is the plain sum.
 * The transformed digits of at most TROYN_HOIST_EACH_GROUP terms are resident at once; later groups add into the extended-basis sum
 * modulo each key modulus.  Modular addition is associative: the words do not depend on the grouping, and the workspace does not grow
 * with `terms` beyond one group.
 * Scope: BFV and CKKS.  BGV is left out (its tail divides differently).
 * BGV has entries of its own with the same arguments: troyn_bgv_apply_galois_sum_each and troyn_bgv_linear_transform_bsgs, in the
 * hoisted BGV block below.
 * TROYN_E_INVALID: terms == 0, a null table, a null or misaligned key entry of a term with g != 1, a misaligned pointer (cts, out,
 * workspace), an element that is even or >= 2N, L outside [1, K-1], `out` overlapping `cts`.  TROYN_E_WORKSPACE: a workspace below
 * troyn_apply_galois_sum_each_workspace_bytes(plan, L, terms, batch, is_ntt_form).  batch == 0 returns TROYN_OK, launches nothing and
 * looks at neither `cts`, `out` nor the workspace.  The tables are read before the call returns.
 *
 * troyn_linear_transform_bsgs: out = SUM_g sigma_{G_g}( SUM_b w_{g,b} (.) sigma_{B_b}(ct) ).
 *   ct               [batch][2][L][N], NTT form iff is_ntt_form
 *   baby_elements    host array of `babies` elements B_b, odd, < 2N, 1 allowed;   baby_keys   host array of babies * L device pointers
 *   giant_elements   host array of `giants` elements G_g, odd, < 2N, 1 allowed;   giant_keys  host array of giants * L device pointers
 *   weights          host array of giants * babies DEVICE pointers, weights[g * babies + b] -> u64[K][N] in NTT form and key-level layout
 *                    (as in the block above), NULL = absent; a giant step with no weight is invalid.  The caller supplies the weights
 *                    ALREADY ROTATED BACK by the giant step: for the matrix diagonal diag_{g,b} that multiplies rot_{G_g + B_b}(v),
 *                    w_{g,b} = rot_{-G_g}(diag_{g,b}), so that rot_{G_g}(w_{g,b} (.) rot_{B_b}(v)) = diag_{g,b} (.) rot_{G_g + B_b}(v)
 *   out              [batch][2][L][N], same form as ct
 * Contract: the words are those of troyn_apply_galois_weighted_sums(ct, baby_*, weights, slots = giants) followed by
 * troyn_apply_galois_sum_each on that result with the giant elements and keys: one decomposition of ct, `giants` divisions for the inner
 * sums, ONE division for the outer sum.  One workspace, one table upload per stage (per group of TROYN_HOIST_EACH_GROUP giant steps in
 * the second); the inner results live in the workspace and are never visible.
 * "double hoisting", keeping the inner c0 component on the extended basis and skipping its division, changes the words of the inner
 * stage: it is troyn_linear_transform_bsgs_double_hoisted, the block below.
 * TROYN_E_INVALID: babies == 0, giants == 0, a giant step with no weight, a misaligned weight, and what the two entries refuse for their
 * tables and buffers (`out` may not overlap `ct`).  TROYN_E_WORKSPACE: a workspace below
 * troyn_linear_transform_bsgs_workspace_bytes(plan, L, babies, giants, batch, is_ntt_form).  batch == 0 returns TROYN_OK and launches
 * nothing.  The tables are read before the call returns.
 * ------------------------------------------------------------------------------------- */
#define TROYN_HOIST_EACH_GROUP 8
size_t troyn_apply_galois_sum_each_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t terms, size_t batch, int is_ntt_form);
int troyn_apply_galois_sum_each(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* cts,
                                const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms, uint64_t* out,
                                void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);
size_t troyn_linear_transform_bsgs_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t babies, size_t giants, size_t batch, int is_ntt_form);
int troyn_linear_transform_bsgs(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct,
                                const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies,
                                const uint64_t* giant_elements, const uint64_t* const* giant_keys, size_t giants,
                                const uint64_t* const* weights, uint64_t* out,
                                void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The double-hoisted BSGS linear transform: troyn_linear_transform_bsgs with the second hoisting level (Bossuat et al.).  The inner sums
 * stay on the extended basis q_0 .. q_{L-1}, q_special; of a giant step only component 1 is divided by the special prime, because only c1
 * is decomposed for the giant key; component 0 goes through the giant automorphism on the extended basis and into the outer sum before
 * the ONE final division.  An ADDITION; the arguments, layouts, alignment rules and refusals are those of troyn_linear_transform_bsgs
 * (babies, giants, both key tables, weights[g * babies + b] in key-level layout and already rotated back by the giant step; BFV in
 * coefficient form, CKKS in NTT form).
 * Contract, per item, on integers (tests/bsgs_double_spec.py; the notation of the three blocks above).  T_g = {b : weight (g, b) non-NULL}:
 *   X^(g)_c[m]   the inner extended-basis value of the weighted-sums block for slot g WITH its unkeyed contributions injected, for every
 *                m in {q_0 .. q_{L-1}, q_special}:
 *                SUM_{b in T_g, B_b != 1} w_{g,b}[m] (*) SUM_j (e_{b,j} mod m) (*) k_{b,j}[c][m]  +  (q_special mod m) * U^(g)_c[m]   mod m
 *                U_0 = SUM_{b in T_g} w_{g,b} (*) sigma_{B_b}(c0),   U_1 = SUM_{b in T_g, B_b = 1} w_{g,b} (*) c1;  nothing is added on
 *                the special row (q_special mod q_special = 0)
 *   G_g != 1:    v^(g)[l] = (X^(g)_1[q_l] - r) * q_special^-1 mod q_l, r the centred representative of the special row exactly as in
 *                troyn_switch_key -- the ONLY inner division, on component 1 alone
 *                d^(g)_j = limb j of v^(g) in coefficient form,  e^(g)_j = sigma_{G_g}(d^(g)_j), signed
 *                Y_c[m] += SUM_j (e^(g)_j mod m) (*) kG_{g,j}[c][m]
 *                Y_0[m] += sigma_{G_g}(X^(g)_0[m])  on EVERY row, the special one included; sigma acts on a residue row as the signed
 *                permutation modulo m
 *   G_g = 1:     Y_c[m] += X^(g)_c[m] for both components: no division, no key
 *   out_c[l] = (Y_c[q_l] - r_c) * q_special^-1 mod q_l, r_c the centred representative of Y_c[q_special]: ONE division for the transform
 * The words are NOT those of troyn_linear_transform_bsgs: that entry rounds both components of every inner sum; this one rounds only
 * component 1 of the giant steps with a key.  Both decrypt to the same message under the same kind of noise bound, and this entry has
 * one rounding per giant step fewer.  Per giant step with a key it saves the inverse transform of one special row, L forward transforms
 * and one finish pass; per identity giant step the whole inner division.
 * The workspace holds the inner results [giants][batch][2][L+1][N]; everything else is sized by one group of TROYN_HOIST_EACH_GROUP giant
 * steps.  One table upload for the inner stage and one per group.
 * Scope: BFV and CKKS.  BGV is left out (its tail divides differently).
 * The hoisted BGV block below has no double-hoisted entry: the inner division on one component needs a BGV tail of its own.
 * TROYN_E_INVALID / TROYN_E_WORKSPACE: as troyn_linear_transform_bsgs, against
 * troyn_linear_transform_bsgs_double_hoisted_workspace_bytes(plan, L, babies, giants, batch, is_ntt_form).  batch == 0 returns TROYN_OK and
 * launches nothing.  The tables are read before the call returns.
 * ------------------------------------------------------------------------------------- */
size_t troyn_linear_transform_bsgs_double_hoisted_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t babies, size_t giants, size_t batch,
                                                                  int is_ntt_form);
int troyn_linear_transform_bsgs_double_hoisted(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct,
                                               const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies,
                                               const uint64_t* giant_elements, const uint64_t* const* giant_keys, size_t giants,
                                               const uint64_t* const* weights, uint64_t* out,
                                               void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * BGV.  BGV ciphertexts live in NTT form and reuse troyn_ntt, troyn_dyadic_convolute (bgv_multiply,
 * evaluator.cu:150-173), troyn_add/sub/negate/multiply_scalar, troyn_apply_galois and troyn_plain_centralize unchanged; the
 * entries below are the steps where BGV differs.  troyn_bgv holds the constants of ONE level's RNSTool that only BGV reads
 * (utils/rns_tool.cu:205-232): the converter q -> {t}, q_last^-1 mod t.
 *   troyn_bgv_mod_t_and_divide_q_last_ntt  RNSTool::mod_t_and_divide_q_last_ntt (utils/rns_tool.cu:1540-1772):
 *                                   in [batch][pcount][L][N] NTT -> out [batch][pcount][L-1][N] NTT; the caller multiplies
 *                                   the correction factor by troyn_bgv_inv_q_last_mod_t (evaluator_modswitch.cu:70-72)
 *   troyn_bgv_decrypt_mod_t         scaling_variant::decentralize (utils/scaling_variant.cu:415-431) = BaseConverter::
 *                                   exact_convey_array (utils/rns_base.cu:445-598, double-precision vote summed in limb
 *                                   order) then * correction_factor^-1 mod t: phase [batch][L][N] coefficient form -> [batch][N]
 *   troyn_bgv_multiply_scalar_mod_t utils::multiply_scalar on mod-t plaintext words (evaluator_translate_plain.cu:80-82)
 *   troyn_bgv_switch_key / _relinearize  switch_key_internal / relinearize_internal with the ski_util5 tail
 *                                   (evaluator_keyswitching_core.cu:436-538, :998-1030); `key_level` must be created with
 *                                   L = the plan's modulus count (its last prime is the special prime).  Shapes and
 *                                   workspace as troyn_switch_key / troyn_relinearize, NTT-form operands.
 * ------------------------------------------------------------------------------------- */
typedef struct troyn_bgv troyn_bgv;
int troyn_bgv_create(troyn_bgv** out, const troyn_plan* plan, uint32_t L, uint64_t plain_modulus);
int troyn_bgv_destroy(troyn_bgv* bgv);
uint64_t troyn_bgv_inv_q_last_mod_t(const troyn_bgv* bgv);
size_t troyn_bgv_mod_switch_workspace_bytes(const troyn_bgv* bgv, size_t pcount, size_t batch);
int troyn_bgv_mod_t_and_divide_q_last_ntt(const troyn_bgv* bgv, const uint64_t* in, size_t pcount, uint64_t* out, void* workspace, size_t workspace_bytes,
                                          size_t batch, troyn_stream_t stream);
int troyn_bgv_decrypt_mod_t(const troyn_bgv* bgv, const uint64_t* phase, uint64_t correction_factor, uint64_t* dest, size_t batch, troyn_stream_t stream);
int troyn_bgv_multiply_scalar_mod_t(const troyn_bgv* bgv, const uint64_t* in, uint64_t scalar, uint64_t* out, size_t count, troyn_stream_t stream);
int troyn_bgv_switch_key(const troyn_bgv* key_level, uint32_t L, const uint64_t* target, const uint64_t* const* keys, int assign_method,
                         uint64_t* destination, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);
int troyn_bgv_relinearize(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct3, const uint64_t* const* keys, uint64_t* out2, void* workspace,
                          size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Hoisted BGV rotations: the hoisted family above (many Galois keys on one decomposition, plaintext-weighted sums, the sum over different
 * ciphertexts, the baby-step/giant-step linear transform) with the BGV division as its tail.  All five entries are ADDITIONS to the
 * reference's surface.  Each takes the arguments of its namesake -- troyn_apply_galois_many, troyn_apply_galois_sum,
 * troyn_apply_galois_weighted_sums, troyn_apply_galois_sum_each, troyn_linear_transform_bsgs -- with `key_level` in place of
 * `plan, is_ckks, is_ntt_form`:
 *   key_level  troyn_bgv_create(plan, n_moduli, t), as for troyn_bgv_switch_key: created with L = the plan's modulus count (its last prime
 *              is the special prime) and with its inverse of the special prime mod t present.  The errors are troyn_bgv_switch_key's.
 * Operands are in NTT form.  The layouts (ct, cts, galois_elements, keys, out), the alignment rules, the identity element where the
 * namesake allows it, and the weights -- u64[K][N] NTT-form rows in KEY-LEVEL layout, NULL = absent -- are those of the namesakes.
 * Contract, per item (and slot), on integers (tests/bgv_hoist_spec.py; the notation of the hoisted blocks above):
 *   X_c[m]       unchanged: the extended-basis value of the namesake, for every key modulus m in {q_0 .. q_{L-1}, q_special}, with the same
 *                signed hoisted digits e_{t,j} = sigma_{g_t}(d_j) and the same injection of the unkeyed terms
 *   s_c          the special row X_c[q_special] in coefficient form, canonical (an integer in [0, q_special))
 *   dk_l(s)      = [-s * q_special^-1 mod t]_{q_l} * q_special + [s]_{q_l}  mod q_l
 *   result_c[l]  exactly as in troyn_bgv_switch_key: result_c[l] = (X_c[q_l] - dk_l(s_c)) * q_special^-1 mod q_l (ski_util5: X_c - dk(s_c)
 *                is divisible by q_special and congruent to X_c mod t)
 *   out          from result_c and the unkeyed terms exactly as the namesake states
 * The unkeyed contributions y may be added after the division or injected before it as (q_special mod q_l) * y on the rows q_l and
 * nothing on the special row; the WORDS are the same either way, by the argument of the weighted block: dk_l depends on the special row
 * alone, and ((X + q_special * y) - dk_l) * q_special^-1 = (X - dk_l) * q_special^-1 + y mod q_l.  troyn_bgv_apply_galois_many / _sum add
 * the permuted c0 after the division, the other entries inject before it.
 * The words are those of NEITHER troyn_apply_galois + troyn_bgv_switch_key NOR the reference, for the reason the hoisted blocks give: where
 * the automorphism negates a coefficient x of d_j the hoisted digit under key modulus m is (-x) mod m, not (q_j - x) mod m, and a sum
 * is divided once, not once per term.  Both are BGV key switches with digits bounded by q_j in magnitude: both decrypt to the same
 * plaintext mod t, exactly, while the noise stays within the bound.  The plaintext's correction factor is unchanged, as for
 * troyn_bgv_switch_key; its bookkeeping stays with the caller.
 * The words of troyn_bgv_linear_transform_bsgs equal troyn_bgv_apply_galois_weighted_sums (slots = giants) followed by
 * troyn_bgv_apply_galois_sum_each on that result with the giant elements and keys.
 * Workspace: the namesakes' queries with is_ntt_form = 1 -- troyn_apply_galois_hoisted_workspace_bytes (sum = 0 for _many, 1 for _sum),
 * troyn_apply_galois_weighted_workspace_bytes, troyn_apply_galois_sum_each_workspace_bytes, troyn_linear_transform_bsgs_workspace_bytes --
 * on the handle's plan, as troyn_bgv_switch_key uses troyn_switch_key_workspace_bytes.
 * Refusals: a null handle, a handle not at the key level (TROYN_E_INVALID) or without its inverse mod t (TROYN_E_MODULUS,
 * "[RNSTool::RNSTool] Unable to invert q[last] mod t."), checked first; then TROYN_E_INVALID / TROYN_E_WORKSPACE exactly as the namesake.
 * batch == 0 returns TROYN_OK, launches nothing and looks at neither the ciphertexts, `out` nor the workspace.  The tables are read before
 * the call returns.  troyn_linear_transform_bsgs_double_hoisted has no BGV form.
 * The division runs as two element-wise kernels around the transforms (bgv_hoist_kernels.hpp): the special row is read once per item and
 * component and the mod-t multiplier formed once per coefficient; the rows of every slot and item share one launch.
 * ------------------------------------------------------------------------------------- */
int troyn_bgv_apply_galois_many(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct, const uint64_t* galois_elements,
                                const uint64_t* const* keys, size_t terms, uint64_t* out, void* workspace, size_t workspace_bytes,
                                size_t batch, troyn_stream_t stream);
int troyn_bgv_apply_galois_sum(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct, const uint64_t* galois_elements,
                               const uint64_t* const* keys, size_t terms, uint64_t* out, void* workspace, size_t workspace_bytes,
                               size_t batch, troyn_stream_t stream);
int troyn_bgv_apply_galois_weighted_sums(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct, const uint64_t* galois_elements,
                                         const uint64_t* const* keys, size_t terms, const uint64_t* const* weights, size_t slots,
                                         uint64_t* out, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);
int troyn_bgv_apply_galois_sum_each(const troyn_bgv* key_level, uint32_t L, const uint64_t* cts, const uint64_t* galois_elements,
                                    const uint64_t* const* keys, size_t terms, uint64_t* out, void* workspace, size_t workspace_bytes,
                                    size_t batch, troyn_stream_t stream);
int troyn_bgv_linear_transform_bsgs(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct,
                                    const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies,
                                    const uint64_t* giant_elements, const uint64_t* const* giant_keys, size_t giants,
                                    const uint64_t* const* weights, uint64_t* out,
                                    void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fused BGV chain: Evaluator::multiply (bgv_multiply, evaluator.cu:150-173) -> Evaluator::relinearize -> Evaluator::mod_switch_to_next
 * of `batch` ciphertext pairs in one call.  An ADDITION to the reference's surface (as the fused CKKS chain above).
 *   key_level  troyn_bgv_create(plan, n_moduli, t), as for troyn_bgv_switch_key
 *   level      troyn_bgv_create(plan, L, t) on the same plan with the same t; L is taken from it, 2 <= L <= n_moduli - 1
 *   a, b       [batch][2][L][N] NTT form, canonical residues;  keys: L device pointers to u64[2][K][N], as for troyn_bgv_relinearize
 *   out        [batch][2][L-1][N] NTT form
 * Contract: the output words equal, word for word, those of these three calls in order:
 *   1. troyn_dyadic_convolute(a, b) on limbs 0 .. L-1
 *   2. troyn_bgv_relinearize(key_level, L, ...)
 *   3. troyn_bgv_mod_t_and_divide_q_last_ntt(level, pcount = 2)
 * As with the stand-alone modulus switch the correction-factor bookkeeping stays with the caller, who multiplies the product's factor
 * by troyn_bgv_inv_q_last_mod_t(level).
 * Derivation (exact integer arithmetic modulo each q_j; qk the special prime, ql = q_{L-1} the dropped one, c = a (x) b):
 *   P        the key-switch inner product of c_2;   s = INTT of P's special row
 *   dk_j(s)  = [-s qk^-1 mod t]_{q_j} qk + [s]_{q_j}
 *   Q_j      = P_j qk^-1 + c_j
 *   l        = INTT(Q_{L-1}) - dk_{L-1}(s) qk^-1 mod q_{L-1}, canonical
 *   dl_j(l)  = [-l ql^-1 mod t]_{q_j} ql + [l]_{q_j}
 *   out_j    = (Q_j - NTT_j(dk_j(s) qk^-1 + dl_j(l))) ql^-1 mod q_j,  j < L-1
 * By linearity of the transforms both corrections are added in coefficient form: one forward transform of 2 (L-1) rows per item where
 * the three calls take 2 L and then 2 (L-1); the relinearized ciphertext and c_0, c_1 never reach memory (bgv_chain_kernels.hpp).
 * TROYN_E_INVALID: a null handle or pointer, a misaligned pointer (16 bytes), handles on different plans or with different t, key_level
 * not at the key level, L outside [2, n_moduli - 1], a null key entry, `out` overlapping a or b.  TROYN_E_MODULUS: either handle lacks
 * its inverse mod t ("[RNSTool::RNSTool] Unable to invert q[last] mod t.").  TROYN_E_WORKSPACE: a workspace below the query.
 * batch == 0 returns TROYN_OK, launches nothing and looks at none of a, b, out and the workspace (all may be null).  Everything is
 * enqueued on the caller's stream; the entry does not synchronise and does not touch the default stream.
 * ------------------------------------------------------------------------------------- */
size_t troyn_bgv_multiply_relinearize_mod_switch_workspace_bytes(const troyn_bgv* key_level, uint32_t L, size_t batch);
int troyn_bgv_multiply_relinearize_mod_switch(const troyn_bgv* key_level, const troyn_bgv* level, const uint64_t* a, const uint64_t* b,
                                              const uint64_t* const* keys, uint64_t* out, void* workspace, size_t workspace_bytes,
                                              size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Ring-2^k polynomial encoder (src/app/bfv_ring2k.{h,cu}: PolynomialEncoderRNSHelper<T>, T = uint32_t / uint64_t / uint128_t):
 * plaintext modulus t = 2^k outside the context's own plain modulus.  One handle per level (first L primes), k and element width.
 *   troyn_ring2k_scale_up     scale_up (:299-360): src elements [count] -> out u64[L][N] = round(Q/t * m), zero beyond `count`
 *   troyn_ring2k_centralize   centralize (:488-560): centred lift of m
 *   troyn_ring2k_scale_down   scale_down (:620-735): in u64[L][N] (phase, coefficient form) -> dst elements [N]
 *   troyn_ring2k_decentralize decentralize (:752-911): in u64[L][N] (x mod Q, coefficient form) -> dst elements [N] = x mod 2^k, times correction^-1 mod 2^k
 *                             (correction_lo / _hi: the odd correction factor as a 128-bit value; 1, 0 for none)
 * ------------------------------------------------------------------------------------- */
typedef struct troyn_ring2k troyn_ring2k;
int troyn_ring2k_create(troyn_ring2k** out, const troyn_plan* plan, uint32_t L, uint32_t t_bit_length, uint32_t element_bytes);
int troyn_ring2k_destroy(troyn_ring2k* h);
uint64_t troyn_ring2k_gamma(const troyn_ring2k* h);
int troyn_ring2k_scale_up(const troyn_ring2k* h, const void* src, size_t count, uint64_t* out, troyn_stream_t stream);
int troyn_ring2k_centralize(const troyn_ring2k* h, const void* src, size_t count, uint64_t* out, troyn_stream_t stream);
int troyn_ring2k_scale_down(const troyn_ring2k* h, const uint64_t* in, void* dst, troyn_stream_t stream);
int troyn_ring2k_decentralize(const troyn_ring2k* h, const uint64_t* in, void* dst, uint64_t correction_lo, uint64_t correction_hi, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * CKKS encoder on the device (src/ckks_encoder.cu: kernel_set_conjugate_values, kernel_fft_transform_{from,to}_rev_layer,
 * kernel_set_plaintext_value_array_*, decode_internal).  One handle per plan; it holds the slot index map (Galois generator 3,
 * bit-reversed) and the root powers of both FFT directions, built on the host with the formulas of CKKSEncoder::CKKSEncoder and
 * uploaded: their contents never depend on the device.  Rows 0..L-1 of a plaintext are under the plan's moduli 0..L-1; L = the plan's
 * modulus count gives the key-level layout that troyn_apply_galois_weighted_sums reads.
 *
 * ENCODING CONTRACT: the words equal those of the host path (troy/troy.cpp), which is the specification:
 *   encode_complex64_simd   a[0..N) = 0; a[index_map[i]] = values[i], a[index_map[i + N/2]] = conj(values[i]) for i < count;
 *                           Gentleman-Sande layers, gap 1, 2, .., N/2, root_index counting up from 1 across the layers:
 *                             r = inv_root_powers[root_index++]; u = a[j], v = a[j + gap]; d = u - v; a[j] = u + v;
 *                             a[j + gap] = (d.re * r.re - d.im * r.im, d.re * r.im + d.im * r.re);
 *                           coefficient j = a[j].re * (scale / N)
 *   encode_float64_polynomial  coefficient j = coeffs[j] * scale, zero for j >= count
 *   set_plaintext           v = nearbyint(coefficient) (half to even); a = |v|; hi = (uint64)(a / 2^64), lo = (uint64)(a - hi * 2^64);
 *                           residue_i = (hi * 2^64 + lo) mod q_i, negated modulo q_i for v < 0; then the forward NTT of every row
 * Both transforms use only IEEE double +, -, * in that order and association (no fused multiply-add on either side), so a device kernel
 * that runs the same butterflies on the same table entries gives the same bits however it divides the layers.
 * |v| >= 2^128 (or a NaN) sets too_large[item] = 1 (0 otherwise); that item's rows are unspecified, every other item is unaffected; with too_large ==
 * NULL such an item is silently unspecified.
 *
 * DECODING CONTRACT (the host path's long double Horner has no device counterpart, so this is defined exactly):
 *   1. inverse NTT of the L rows;  2. x = the centred representative in (-Q/2, Q/2] of the residues, Q = q_0 ... q_{L-1};
 *   3. coefficient j = (x correctly rounded to the nearest double, ties to even) / scale, IEEE division;
 *   4. troyn_ckks_decode_simd continues with the Cooley-Tukey layers of decode_complex64_simd on (coefficient, 0), gap N/2, .., 1:
 *        r = root_powers[root_index++]; u = a[j], w = a[j + gap]; v = (w.re * r.re - w.im * r.im, w.re * r.im + w.im * r.re);
 *        a[j] = u + v; a[j + gap] = u - v;      slot i = a[index_map[i]]
 *   L <= 16; above that TROYN_E_UNSUPPORTED.
 *
 * values [batch][count][2] (re, im; 16-byte aligned), coeffs [batch][count], out u64 [batch][L][N] in NTT form / double [batch][N] /
 * double [batch][N/2][2], too_large u32 [batch]: all device memory.  The encoders need troyn_ckks_encode_workspace_bytes(h, batch) bytes (the points
 * between the two FFT passes at N >= 16384; nothing below, where the workspace may be null), the decoders troyn_ckks_workspace_bytes(h, L, batch),
 * which is never the smaller of the two.
 * TROYN_E_INVALID: a null handle or pointer, a misaligned pointer (16 bytes; 8 for coeffs, 4 for too_large), L outside [1, n_moduli],
 * count above N/2 (N for polynomials), an encoding scale that is not positive or has log2(scale) + 1 >= the total bit count of the L
 * primes.  TROYN_E_WORKSPACE: a workspace below the entry's size.  batch == 0 returns TROYN_OK and touches nothing; only the handle and L
 * are looked at before.  count == 0 encodes zero (the source may then be null).  Everything is enqueued on the caller's stream; no entry synchronises or
 * touches the default stream.  troyn_ckks_get_tables copies the host tables out (index_map [N], root_powers / inv_root_powers [N][2]).
 * ------------------------------------------------------------------------------------- */
typedef struct troyn_ckks troyn_ckks;
int troyn_ckks_create(troyn_ckks** out, const troyn_plan* plan);
int troyn_ckks_destroy(troyn_ckks* h);
int troyn_ckks_get_tables(const troyn_ckks* h, uint32_t* index_map, double* root_powers, double* inv_root_powers);
size_t troyn_ckks_workspace_bytes(const troyn_ckks* h, uint32_t L, size_t batch);
size_t troyn_ckks_encode_workspace_bytes(const troyn_ckks* h, size_t batch);
int troyn_ckks_encode_simd(const troyn_ckks* h, uint32_t L, const double* values, size_t count, double scale, uint64_t* out, uint32_t* too_large,
                           void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);
int troyn_ckks_encode_polynomial(const troyn_ckks* h, uint32_t L, const double* coeffs, size_t count, double scale, uint64_t* out, uint32_t* too_large,
                                 void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);
int troyn_ckks_decode_polynomial(const troyn_ckks* h, uint32_t L, const uint64_t* plain, double scale, double* out, void* workspace, size_t workspace_bytes,
                                 size_t batch, troyn_stream_t stream);
int troyn_ckks_decode_simd(const troyn_ckks* h, uint32_t L, const uint64_t* plain, double scale, double* out, void* workspace, size_t workspace_bytes,
                           size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Matrix diagonals encoded into BSGS weights (an addition to the reference's API): `items` plaintexts, each one diagonal of a complex
 * n x n matrix rotated back by a shift, selected and rotated while the encoder's first FFT pass loads its points -- the pre-rotated
 * diagonals never exist in memory.
 *
 * CONTRACT: the words of `out` ([items][L][N], NTT form) are those troyn_ckks_encode_simd writes for batch = items, count = N/2 and the
 * values array below; that entry is the specification.  Item t carries the two words (a_t, s_t) = pairs[t][0..1]; for 0 <= i < N/2
 *   src_is_matrix = 0   src = diags, double [nd][n][2]:               values[t][i] = diags[a_t][(i - s_t) mod n]
 *   src_is_matrix = 1   src = matrix, double [n][n][2], row-major:    values[t][i] = matrix[j][(j + a_t) mod n], j = (i - s_t) mod n
 * (diagonal a of M is diag_a[j] = M[j][(j + a) mod n]).  n is a power of two, 1 <= n <= N/2; n < N/2 is the sparsely packed case: the
 * diagonal repeats N/(2n) times across the slots.  nd is not read in matrix mode.
 * A word of `pairs` out of range is the caller's error and never reads outside `src`: s_t is masked (s_t mod n); a_t is clamped to nd - 1 in
 * diagonals mode and masked (a_t mod n) in matrix mode.
 * src, pairs (u32 [items][2]), out, too_large (u32 [items] or null, as above): device memory.  The workspace is
 * troyn_ckks_encode_diagonals_workspace_bytes(h, items) bytes (the encoder's: nothing below N = 16384, where it may be null).
 * TROYN_E_INVALID: a null handle or pointer, a misaligned pointer (16 bytes for src, out and the workspace; 4 for pairs and too_large), n not a
 * power of two or above N/2, nd == 0 in diagonals mode, L outside [1, n_moduli], a scale the encoder refuses.  TROYN_E_WORKSPACE: a short
 * workspace.  items == 0 returns TROYN_OK and touches nothing; only the handle and L are looked at before.  Everything is enqueued on the
 * caller's stream; the entry does not synchronise or touch the default stream.
 * ------------------------------------------------------------------------------------- */
size_t troyn_ckks_encode_diagonals_workspace_bytes(const troyn_ckks* h, size_t items);
int troyn_ckks_encode_diagonals(const troyn_ckks* h, uint32_t L, const double* src, int src_is_matrix, uint32_t n, uint32_t nd,
                                const uint32_t* pairs, double scale, uint64_t* out, uint32_t* too_large,
                                void* workspace, size_t workspace_bytes, size_t items, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Factors of the special DFT (an addition to the reference's API): the matrices of CoeffToSlot / SlotToCoeff for the reference's slot order,
 * Galois generator 3, written to device memory by their present diagonals in the layout troyn_ckks_encode_diagonals reads in diagonals mode.
 *
 * N is the ring degree, n = N/2, m = log2 n, zeta = exp(2 pi i / 2N).  With t the N real coefficients, w_k = t_k + i t_{k+n} and z_j the
 * slots, zh_j = z_j (j even) / conj(z_j) (j odd) is an ordinary special FFT on the rotation group (-3)^j (3 = -1 mod 4: odd slots see conj(w)):
 *   zh = L_{m-1} ... L_0 BR w,   BR the bit reversal on m bits; layer b has lh = 2^b, len = 2 lh and tw_b(j) = zeta^(((-3)^j mod 4 len) 2N / 4 len);
 *   rows (i + j, i + j + lh), j < lh, of L_b are [[1, tw], [1, -tw]] and of L_b^-1 they are 1/2 [[1, 1], [1/tw, -1/tw]].
 * The entry writes the product of the layers [first, first + count): forward L_{first+count-1} ... L_first, inverse (inverse != 0)
 * L_first^-1 ... L_{first+count-1}^-1.  out is double [nd][n][2], out[a][i] = M[i][(i + d_a) mod n], d_a ascending mod n: the multiples of
 * 2^first up to +-(2^count - 1) of them, nd = 2^(count+1) - 1, or 2^count when first + count == m (+k and -(2^count - k) then coincide).
 * troyn_ckks_dft_factor_diagonals_count gives nd (0 for a null handle, count == 0 or layers outside [0, m]).
 * col_mask / row_mask: 0 none, 1 keep even columns / rows, 2 keep odd ones; conjugate != 0 conjugates every entry; `constant` (real) is
 * multiplied in.  Absent and masked entries are +0.
 *
 * CONTRACT: the words of `out` equal those of tests/dft_factors_spec.py (table) on the handle's own tables (troyn_ckks_get_tables): an entry
 * is ONE product of butterfly coefficients in the order of application -- acc = (constant, 0); per layer a coefficient 1 is skipped, another
 * one is a complex multiply (re = ar cr - ai ci, im = ar ci + ai cr, every operation rounded on its own, no FMA), the 1/2 of an inverse layer
 * its own multiply after it -- and every twiddle is read from root_powers (zeta^k = root_powers[bitrev(k mod N)], negated for k >= N).
 *
 * No workspace.  out: device memory, 16-byte aligned.  The kernel is enqueued on the caller's stream; the entry does not synchronise or touch
 * the default stream.  count == 0 returns TROYN_OK and touches nothing; only the handle is looked at before.  TROYN_E_INVALID: a null handle or
 * pointer, a misaligned pointer, layers outside [0, log2 n] (first + count > m), an unknown mask, a constant that is not finite.
 * ------------------------------------------------------------------------------------- */
size_t troyn_ckks_dft_factor_diagonals_count(const troyn_ckks* h, uint32_t first, uint32_t count);
int troyn_ckks_dft_factor_diagonals(const troyn_ckks* h, uint32_t first, uint32_t count, int inverse, int col_mask, int row_mask, int conjugate,
                                    double constant, double* out, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Factors of the special DFT on n slots (an addition to the reference's API): the same matrices for a sparsely packed message, n a power of
 * two with 2 <= n <= N/2.  (n = 1 has no such transform: 3 has order 2, not 1, modulo 4.)
 *
 * With s = N/(2n) a sparsely packed message is a polynomial p(Y), Y = X^s, of degree < 2n; t' its coefficients, w_k = t'_k + i t'_{k+n}.  Slot j
 * evaluates p at (zeta^s)^(3^j), zeta^s a primitive 4n-th root, and 3 has order n modulo 4n: the N/2 slots are an n-vector z repeated s times.
 * The derivation above holds verbatim for the ring of degree 2n with m' = log2 n: zh = L_{m'-1} ... L_0 BR w, BR on m' bits, and layer b's
 * twiddle (zeta^s)^(((-3)^j mod 4 len) 4n / 4 len) = zeta^(((-3)^j mod 4 len) 2N / 4 len) is the full ring's layer b, read from the same
 * root_powers.  The table is therefore the one of troyn_ckks_dft_factor_diagonals taken on one n x n block: n rows, diagonal indices mod n,
 * first + count <= m', and the group with first + count == m' is the one where +k and -(2^count - k) coincide (nd = 2^count).
 * out is double [nd][n][2], the layout troyn_ckks_encode_diagonals reads in diagonals mode with that n (which repeats a diagonal s times across
 * the slots).  troyn_ckks_dft_factor_diagonals_sparse_count gives nd (0 for a null handle, an n that is refused, count == 0 or layers outside
 * [0, m']).  Masks, conjugate and constant as above.
 *
 * CONTRACT: the words of `out` equal those of tests/sparse_bootstrap_spec.py (table), which is tests/dft_factors_spec.py's table taken on n
 * rows of the handle's own full-ring tables: ONE product per entry, the same association, every operation rounded on its own, no FMA.  With
 * n = N/2 the words are those of troyn_ckks_dft_factor_diagonals.
 *
 * No workspace; out: device memory, 16-byte aligned; caller's stream, no synchronisation.  count == 0 returns TROYN_OK and touches nothing; only
 * the handle is looked at before.  TROYN_E_INVALID: as above, and n not a power of two, n < 2, n > N/2, layers outside [0, log2 n].
 * ------------------------------------------------------------------------------------- */
size_t troyn_ckks_dft_factor_diagonals_sparse_count(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count);
int troyn_ckks_dft_factor_diagonals_sparse(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count, int inverse, int col_mask, int row_mask,
                                           int conjugate, double constant, double* out, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Factors of the special DFT on n slots, both halves on period 2n (an addition to the reference's API): the table with which a sparsely packed
 * bootstrap keeps the real and the imaginary parts of its slots side by side in ONE ciphertext, n a power of two with 2 <= n <= N/4.
 *
 * Layers [first, first + count) with first + count <= log2 n are block diagonal with blocks of at most n rows.  Taken on 2n rows they are two
 * identical n x n blocks, no entry crosses row n, and the group is never the top one: nd = 2^(count+1) - 1 diagonals, indices mod 2n
 * (diag_a[j] = M[j][(j + a) mod 2n]).  out is double [nd][2n][2]:
 *   rows i <  n   the words of troyn_ckks_dft_factor_diagonals_sparse called with 2n (no masks, no conjugate);
 *   rows i >= n   the same words turned by a quarter: by -i in the inverse direction, (re, im) -> (im, -re), and by +i in the forward one,
 *                 (re, im) -> (-im, re).  The turn is a swap and one IEEE negation, so a present entry with a zero component yields -0.0;
 *                 absent entries stay +0 in both words.
 * Inverse (the last-applied group of CoeffToSlot, layers [0, c)): for u of period n, v = M u has G u in rows < n and -i G u below, and
 * v + conj(v) holds 2 Re(G u) in slots [0, n) and 2 Im(G u) in [n, 2n).  Forward (the first-applied group of SlotToCoeff): for a real
 * operand [a; b] of period 2n, V = M [a; b] = [F a; i F b] and V + rot_n(V) = F (a + i b), of period n.
 * troyn_ckks_encode_diagonals reads the table unchanged with n = 2n.  troyn_ckks_dft_factor_diagonals_packed_count gives nd (0 for a null
 * handle, an n that is refused, count == 0 or layers outside [0, log2 n]).
 *
 * CONTRACT: the words of `out` equal those of tests/packed_bootstrap_spec.py (table) on the handle's own full-ring tables: ONE product per
 * entry, the association and roundings of tests/sparse_bootstrap_spec.py, no FMA; rows < n equal troyn_ckks_dft_factor_diagonals_sparse at 2n.
 *
 * No workspace; out: device memory, 16-byte aligned; caller's stream, no synchronisation.  count == 0 returns TROYN_OK and touches nothing; only
 * the handle is looked at before.  TROYN_E_INVALID: null handle or pointer, misaligned pointer, n not a power of two, n < 2, n > N/4, layers
 * outside [0, log2 n], a constant that is not finite.
 * ------------------------------------------------------------------------------------- */
size_t troyn_ckks_dft_factor_diagonals_packed_count(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count);
int troyn_ckks_dft_factor_diagonals_packed(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count, int inverse, double constant, double* out,
                                           troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Real and imaginary parts of CKKS slots (an addition to the reference's API): the two streaming steps between CoeffToSlot, EvalMod and
 * SlotToCoeff of a bootstrap, on the multiplication by i that costs no key switch, no level and no scale.
 *
 * The slot order is Galois generator 3: slot j evaluates a plaintext at zeta^(3^j), zeta = exp(2 pi i / 2N), and
 * (zeta^(3^j))^(N/2) = i^(3^j) = i (-1)^j.  Multiplying a ciphertext by the monomial X^(N/2) therefore multiplies slot j by i (-1)^j, whatever
 * the slots hold.  With w a ciphertext and wc its complex conjugate (troyn_apply_galois with the element 2N - 1, then a key switch):
 *   s = w + wc                 slots 2 Re w
 *   d = (wc - w) X^(N/2)       slots (-1)^j 2 Im w           (wc - w = -2i Im w, times i (-1)^j)
 *   out = s' + d' X^(N/2)      slots Re' + i Im' when s' holds Re' and d' holds (-1)^j Im'        ((-1)^j squared)
 * The sign pattern (-1)^j passes through any ODD slot-wise function (EvalMod's sine) and cancels in the join.
 *
 * In NTT form the product with X^(N/2) is a dyadic product with mu, the forward transform of the monomial: mu = iota_l on the lower half
 * of a row (indices below N/2) and q_l - iota_l on the upper half, iota_l = psi_l^(N/2) the square root of -1 modulo q_l that
 * troyn_plan_get_root_powers holds at index 1 (tests/bootstrap_spec.py derives the halves from the tables and checks them against the transform).
 *   troyn_ckks_complex_split   s = a + b,  d = mu . (b - a)      (a = w, b = wc)
 *   troyn_ckks_complex_join    out = a + mu . b
 * modulo q_l, canonical words in and out.  a, b, s, d, out: [batch][2][L][N] on the plan's first L moduli, NTT form, device memory, 16-byte
 * aligned.  An output may be one of the inputs (same pointer); s and d must differ.
 *
 * CONTRACT: the words equal those of troyn_add, troyn_sub and troyn_dyadic_product with the transformed monomial (troyn_ntt_forward of
 * X^(N/2)), word for word: every result is the canonical residue of the same integer.  split reads four rows and writes four rows per limb,
 * once each, in ONE launch (composed: three launches and about twice the traffic); join reads two rows and writes one.
 *
 * No workspace.  The kernel is enqueued on the caller's stream; the entries do not synchronise or touch the default stream.  batch == 0
 * returns TROYN_OK and touches nothing; only the plan and L are looked at before.  TROYN_E_INVALID: a null plan or pointer, a misaligned
 * pointer, L == 0, L above the plan's moduli, s == d, a batch too large for one launch.
 * ------------------------------------------------------------------------------------- */
int troyn_ckks_complex_split(const troyn_plan* plan, uint32_t L, const uint64_t* a, const uint64_t* b, uint64_t* s, uint64_t* d, size_t batch,
                             troyn_stream_t stream);
int troyn_ckks_complex_join(const troyn_plan* plan, uint32_t L, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t batch, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * CKKS ModRaise (an addition to the reference's API): the exact centred base extension of a ciphertext from the plan's moduli
 * 0..L_in-1 to its moduli 0..L_out-1, the first step of a bootstrap.  On the troyn_ckks handle, which owns the Garner table q_j^-1 mod q_i.
 * Layouts of troyn_mod_switch_drop: in u64 [batch][pcount][L_in][N], out u64 [batch][pcount][L_out][N], row i under modulus i.
 *
 * MODRAISE CONTRACT (on integers):
 *   1. for every coefficient position in coefficient form, x = the centred representative in (-Q/2, Q/2] of the L_in input residues,
 *      Q = q_0 ... q_{L_in-1} -- the convention of decoding step 2: X > floor(Q/2) stands for X - Q;
 *   2. out_j = x mod q_j in [0, q_j) for every j < L_out.
 *   Input words are canonical (< q_i); under that precondition rows j < L_in of `out` equal the input rows word for word.
 *   is_ntt_form = 1: the map is NTT o extend o INTT.  Rows j < L_in are copied and never transformed; only the L_in input rows take the
 *   inverse transform and only the L_out - L_in new rows the forward one, both through the launch layer of troyn_ntt.
 *   is_ntt_form = 0: no transform runs.
 *   `in` and `out` must not overlap.
 *   1 <= L_in < L_out <= n_moduli.  L_in <= 16 (as the decoder); above that TROYN_E_UNSUPPORTED.
 *
 * The workspace (troyn_ckks_mod_raise_workspace_bytes; device memory, 16-byte aligned) holds the coefficient forms of the input rows and of
 * the new rows in NTT form; it is empty in coefficient form, where it may be null.
 * TROYN_E_INVALID: a null handle or pointer, a misaligned pointer (16 bytes), limb counts outside the range above, `out` overlapping `in`.
 * TROYN_E_WORKSPACE: a workspace below the entry's size.  batch == 0 (or pcount == 0) returns TROYN_OK and touches nothing; only the handle and the
 * limb counts are looked at before.  Everything is enqueued on the caller's stream; no entry synchronises or touches the default stream.
 * ------------------------------------------------------------------------------------- */
size_t troyn_ckks_mod_raise_workspace_bytes(const troyn_ckks* h, uint32_t L_in, uint32_t L_out, size_t pcount, size_t batch, int is_ntt_form);
int troyn_ckks_mod_raise(const troyn_ckks* h, uint32_t L_in, uint32_t L_out, int is_ntt_form, const uint64_t* in, size_t pcount,
                         uint64_t* out, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* RLWE / LWE packing (evaluator_lwes.cu):
 *   troyn_negacyclic_shift     utils::negacyclic_shift_ps (utils/poly_small_mod.cu:927-968): multiply `count` RNS polynomials by
 *                              X^shift, any shift (taken modulo 2N as the reference does); out of place
 *   troyn_multiply_inv_degree  utils::ntt_multiply_inv_degree (utils/ntt.cu:93-134): x * N^-1 * scalar mod q_l
 *                              (Evaluator::divide_by_poly_modulus_degree_inplace, evaluator_lwes.cu:142-151)
 *   troyn_pack_prepare         first step of Evaluator::pack_rlwe_ciphertexts_new(_batched) (evaluator_lwes.cu:361-381, :599-640):
 *                              out[slot] = X^shift * src[slot] * N^-1 * mul, zero where src[slot] == NULL; src = host array of
 *                              `slots` device pointers to coefficient-form ciphertexts u64[pcount][L][N]
 *   troyn_pack_layer           one layer of the packing tree (:441-477, :654-697) on adjacent pairs in[2k] (even), in[2k+1] (odd)
 *                              of two-polynomial ciphertexts:  temp = X^shift*odd, out[k] = even + temp + perm_g(even - temp) with
 *                              the permuted c1 diverted to target[k]; follow with troyn_switch_key(target -> out, ADD_INPLACE,
 *                              batch = pairs, Galois key of g) to finish apply_galois.  in u64[2*pairs][2][L][N],
 *                              out u64[pairs][2][L][N], target u64[pairs][L][N]
 *   troyn_extract_lwe          Evaluator::extract_lwe_new (evaluator_lwes.cu:52-97) for `count` (ciphertext, term) pairs:
 *                              c0 u64[count][L], c1 u64[count][L][N] */
int troyn_negacyclic_shift(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* in, uint64_t* out, size_t shift,
                           size_t count, troyn_stream_t stream);
int troyn_multiply_inv_degree(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, const uint64_t* in, uint64_t* out, uint64_t scalar,
                              size_t count, troyn_stream_t stream);
size_t troyn_pack_prepare_workspace_bytes(size_t slots);
int troyn_pack_prepare(const troyn_plan* plan, uint32_t L, size_t pcount, const uint64_t* const* src, size_t slots, uint64_t mul, size_t shift,
                       uint64_t* out, void* workspace, size_t workspace_bytes, troyn_stream_t stream);
int troyn_pack_layer(const troyn_plan* plan, uint32_t L, uint64_t galois_element, size_t shift, const uint64_t* in, uint64_t* out,
                     uint64_t* target, size_t pairs, troyn_stream_t stream);
size_t troyn_extract_lwe_workspace_bytes(size_t count);
int troyn_extract_lwe(const troyn_plan* plan, uint32_t L, const uint64_t* const* ct, const size_t* terms, uint64_t* c0, uint64_t* c1, size_t count,
                      void* workspace, size_t workspace_bytes, troyn_stream_t stream);
/* Staging for the reference's x_batched(vector<const T*>, ...) forms (batch_utils.h construct_batch + per-item loops inside
 * the kernels): `count` scattered device buffers of `words` words (16-byte aligned) -> one contiguous block, one launch. */
size_t troyn_gather_workspace_bytes(size_t count);
int troyn_gather(const uint64_t* const* src, size_t count, size_t words, uint64_t* out, void* workspace, size_t workspace_bytes, troyn_stream_t stream);
/* The inverse (results of one batched call back to `count` separate buffers; workspace as for troyn_gather).  Up to 64 buffers the
 * pointers of either call travel in the kernel arguments: no upload, no host wait. */
int troyn_scatter(const uint64_t* in, uint64_t* const* dst, size_t count, size_t words, void* workspace, size_t workspace_bytes, troyn_stream_t stream);
size_t troyn_multiply_plain_accumulate_workspace_bytes(size_t count);
int troyn_multiply_plain_accumulate(const troyn_plan* plan, uint32_t mod_start, uint32_t nmod, size_t pcount,
                                    const uint64_t* const* ct, const uint64_t* const* pt, uint64_t* const* dst, size_t count,
                                    int set_zero, void* workspace, size_t workspace_bytes, troyn_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * BEHZ BFV multiply: Evaluator::bfv_multiply (evaluator.cu:29-116) with the RNSTool of the level
 * holding the first L plan moduli and plain modulus t (RNSTool ctor utils/rns_tool.cu:29-275;
 * fused device kernels fgk/rns_tool.cu:7-100, :147-286).  a[batch][pa][L][N] x b[batch][pb][L][N]
 * (coefficient form) -> out[batch][pa+pb-1][L][N].
 * ------------------------------------------------------------------------------------- */
int troyn_behz_create(troyn_behz** behz, const troyn_plan* plan, uint32_t L, uint64_t plain_modulus);
int troyn_behz_destroy(troyn_behz* behz);
uint32_t troyn_behz_base_Bsk_size(const troyn_behz* behz);
int troyn_behz_get_base_Bsk(const troyn_behz* behz, uint64_t* out); /* host copy, KAT hook: the base utils/rns_tool.cu:52-80 picks */
/* Number of primes of the auxiliary base troyn_bfv_multiply actually works in.  Equal to troyn_behz_base_Bsk_size unless every q_i is below
 * 2^50: then the multiply uses primes BELOW 2^50, sized by the reference's own criterion bits(prod(B) m_sk) > 32 + bits(t) + bits(q)
 * (utils/rns_tool.cu:50-62; results are independent of the choice), so that all of its transforms take the exact-FP64 butterflies
 * (plan option TROYN_BEHZ_BASE=ref at creation keeps the reference's base).  Sizes of intermediates follow this count. */
uint32_t troyn_behz_working_base_size(const troyn_behz* behz);
uint64_t troyn_behz_gamma(const troyn_behz* behz);
/* scaling_variant::scale_up / multiply_add_plain / multiply_sub_plain (utils/scaling_variant.cu:17-90,
 * fgk/translate_plain.cu:6-75): dest[item][L][N] = (from[item][L][N] or 0) +/- round(q/t * plain[item][i]);
 * coefficients i >= plain_coeff_count copy `from` (or 0).  Strides in elements; `from` may be NULL or == dest. */
int troyn_bfv_scale_up(const troyn_behz* behz, const uint64_t* plain, size_t plain_coeff_count, size_t plain_bstride,
                       const uint64_t* from, size_t from_bstride, uint64_t* dest, size_t dest_bstride,
                       int subtract, size_t batch, troyn_stream_t stream);
/* RNSTool::decrypt_scale_and_round (utils/rns_tool.cu:1189-1391): phase[batch][L][N] (c0 + c1*s + ..., coefficient
 * form) -> dest[batch][N] mod t. */
int troyn_bfv_decrypt_scale_and_round(const troyn_behz* behz, const uint64_t* phase, uint64_t* dest, size_t batch, troyn_stream_t stream);
size_t troyn_bfv_multiply_workspace_bytes(const troyn_behz* behz, size_t pa, size_t pb, size_t batch);
int troyn_bfv_multiply(const troyn_behz* behz, const uint64_t* a, size_t pa, const uint64_t* b, size_t pb,
                       uint64_t* out, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);

/* BFV inner product: a sum of BEHZ tensor products with ONE scale-down.  Both entries are ADDITIONS to the reference's surface (the reference
 * multiplies pair by pair, Evaluator::bfv_multiply, evaluator.cu:29-116, and relinearizes every product, evaluator_keyswitching.cu:119-144).
 *
 * troyn_bfv_multiply_accumulate:
 *     out = floor_step( INTT( SUM_t NTT(lift(a[t])) (x) NTT(lift(b[t])) ) )
 *   lift        steps (1)-(3) of Evaluator::bfv_multiply: fast_b_conv_m_tilde, sm_mrq, forward transforms in q and in Bsk
 *   (x)         the two-by-two tensor product; the sums are taken modulo each prime of q and of the auxiliary base
 *   floor_step  steps (6)-(8): multiply by t, fast_floor, fast_b_conv_sk
 *   a, b   host arrays of `terms` device pointers, each to u64[batch][2][L][N] in coefficient form, 16-byte aligned; pointers may repeat
 *          and a[t] == b[t] is allowed
 *   out    [batch][3][L][N], coefficient form
 * Contract: every stored word is a canonical residue, so the words depend neither on where reductions happen nor on the auxiliary base the
 * product works in; with terms == 1 they are bit-identical to troyn_bfv_multiply with pa = pb = 2.  The conversions stay exact while
 * terms * N * t * q * (1 + rho)^2 < prod(B) * m_sk; both the reference's base and the working base (troyn_behz_working_base_size) leave
 * 2^31 for terms * N, and the entries accept terms <= 1024 (terms * N <= 2^27 at N = 2^17).
 *
 * troyn_bfv_multiply_accumulate_relinearize: out [batch][2][L][N] = troyn_relinearize(L, is_ckks = 0, is_ntt_form = 0) of the sum above,
 * bit-identical to the two calls; keys as for troyn_switch_key.  One key switch for the whole sum.
 *
 * Terms are lifted and accumulated in chunks of at most 32 (every distinct pointer of a chunk is lifted once), so
 * workspace_bytes(terms) == workspace_bytes(min(terms, 32)).
 * Errors: TROYN_E_INVALID for terms == 0, terms > 1024, a null table or entry, a misaligned pointer, `out` overlapping an input;
 * TROYN_E_WORKSPACE for a workspace below the queried size.  batch == 0 returns TROYN_OK, launches nothing and looks at neither `out` nor
 * the workspace. */
size_t troyn_bfv_multiply_accumulate_workspace_bytes(const troyn_behz* behz, size_t terms, size_t batch);
int troyn_bfv_multiply_accumulate(const troyn_behz* behz, const uint64_t* const* a, const uint64_t* const* b, size_t terms,
                                  uint64_t* out, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream);
size_t troyn_bfv_multiply_accumulate_relinearize_workspace_bytes(const troyn_behz* behz, size_t terms, size_t batch);
int troyn_bfv_multiply_accumulate_relinearize(const troyn_behz* behz, const uint64_t* const* a, const uint64_t* const* b, size_t terms,
                                              const uint64_t* const* keys, uint64_t* out, void* workspace, size_t workspace_bytes,
                                              size_t batch, troyn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TROYN_H */
