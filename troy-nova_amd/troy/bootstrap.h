// bootstrap.h -- troy::BootstrapPlan, an ADDITION to the reference's interface: the CKKS bootstrap of a fully or sparsely packed ciphertext,
//     ModRaise -> (SubSum) -> CoeffToSlot -> (real / imaginary parts) -> EvalMod on both halves at once -> (join) -> SlotToCoeff,
// (a packed sparse plan: both halves in ONE EvalMod operand, no split and no join)
// as one call, Evaluator::bootstrap.  The plan owns the two slot plans (slot_transform.h), chooses every level, scale and normalisation constant and says
// which Galois keys are needed.  Sparse packing (n < N/2 slots) is the section of that name below.  With sparse secrets K shrinks: KeyGenerator::create_sparse draws a
// secret of a fixed Hamming weight, and the sparse-secret encapsulation below keeps a dense evaluation secret while I comes from a sparse one.
//
// Notation.  N the ring degree, n = N/2, q0 the first prime (the only one of the last level), D = message_scale (Delta), K = half_width, r = double_angles.
// An exhausted ciphertext decrypts to D m modulo q0.  After mod_raise it decrypts, modulo the whole chain, to t = D m + q0 I with an integer polynomial I.
//
// Conditions (the caller's):
//   K - 1 >= ||I||_inf.  For a ternary secret of Hamming weight h -- the secret under which mod_raise runs -- the coefficients of I behave like sums of
//     h + 1 uniform fractions: standard deviation sqrt((h + 1) / 12).  Rule of thumb K - 1 >= 6.5 sqrt((h + 1) / 12) = half_width_for(h) - 1.  A dense
//     secret of this key generator has h about 2N/3 and at most N, for which the rule reads K - 1 >= 6.5 sqrt((N + 1) / 12): half_width_for(N) is 61.1
//     at N = 1024 (K = 64 as a power of two) and 241.2 at N = 16384 (K = 256).  h = 192 gives 27.1, and the ephemeral h = 32 of the encapsulation 11.8 (K = 12).  Which h is safe for a chain is the caller's call.
//   |D m| / q0 <= 2^-7, eval_mod's own condition: sin(2 pi x) / (2 pi) is x up to a cubic term.  The constructor asks for q0 / D >= 2 only.
//
// The steps of Evaluator::bootstrap and where each factor goes -- none costs a level:
//   1. mod_switch_to the last level if the operand is above it; its scale must be D (the evaluator's scale comparison).
//   2. mod_raise to first_parms_id().
//   3. 1 / q0: the scale is RELABELLED to q0, so that the coefficients read x = t / q0 = D m / q0 + I.
//   4. coeff_to_slot with the constant c1 (below): slots c1 BR(x_k + i x_{k+n}) at the scale s1 that the evaluator tracks.
//   5. split_real_imag: slots 2 c1 Re and (-1)^j 2 c1 Im.  1 / 2 and c1: both halves are RELABELLED to the scale 2 c1 s1, so that their slots read x.
//   6. eval_mod_batched on the pair.  K: eval_mod relabels the working scale to 2 c1 s1 K.  Its first products are rescaled by the prime q_w under the
//      CoeffToSlot levels, and evaluate_chebyshev asks for a working scale close to the primes, hence
//          c1 = q_w / (2 K s1),   s1 = q0 PROD_g (weight_scale / prime of group g)   computed as the evaluator computes it,
//      which makes the working scale q_w up to rounding.  2 pi: eval_mod's own relabel.  The slots now read D m / q0, (-1)^j on the imaginary half
//      (sine is odd, so the sign passes; the interpolant's error is not odd but stays of its own size).
//   7. join_real_imag: slots D / q0 (m_k + i m_{k+n}) in bit-reversed order, at the scale s_e that eval_mod leaves.
//   8. slot_to_coeff with the constant c2 = q0 / s2, s2 = s_e PROD_g (weight_scale / prime of group g) the scale the evaluator will track: q0 / D.
//   9. The payload is now D z for the message slots z, and the scale is SET to D, a double assignment, as eval_mod does with 2 pi.
//
// Levels: levels() = groups(CoeffToSlot) + depth(EvalMod) + groups(SlotToCoeff), depth(EvalMod) = Evaluator::chebyshev_depth(degree) + r, the depth that
// evaluate_chebyshev documents plus the double angles.  The chain needs levels() + 1 data primes; every prime beyond that is a level the result can still spend.
// Key switches: key_switches() counts the Galois key switches of one call -- the rotations and conjugations of both slot plans and the one conjugation of
// split_real_imag; EvalMod's relinearizations (one per product step) are not Galois key switches and are not counted.  rotation_steps() is the union of
// both slot plans' steps and step 0, which create_galois_keys_from_steps reads as the conjugation.
//
// Sparse packing.  A trailing n (0: N/2), a power of two with 2 <= n <= N/2, is the number of message slots: the message is z tiled s = N/(2n) times, that
// is, a polynomial p(Y) in Y = X^s.  Both slot plans are built on n slots (slot_transform.h): log2 n layers each instead of log2(N/2).
//   2b. Evaluator::sub_sum.  After mod_raise t = D p(Y) + q0 I(X), and I is NOT a polynomial in Y.  The rotations by n i, i < s, are the automorphisms X -> X^g
//       with g = 1 (mod 4n); they fix every X^(s k) and sum to 0 over the other monomials, so SUM_i rot_{n i} decrypts to s (D p(Y) + q0 I'(Y)), I' the
//       Y-coefficients of I.  ||I'||_inf <= ||I||_inf: the K condition is unchanged.  The sum runs as PROD_i (1 + rot_{n 2^i}) in stages of sub_sum_radix terms.
//   4.  1 / s goes into the CoeffToSlot constant, c1 = q_w / (2 K s1 s) (a power of two: exact), and costs no level; step 5 relabels to 2 c1 s1 s.
//   Everything after CoeffToSlot is as above on slots of period n.  With the encapsulation sub_sum runs after the to_dense switch (2a).
// levels() has the shorter plans' groups and nothing for SubSum; key_switches() adds SubSum's radix - 1 per stage; rotation_steps() adds its steps.
//
// Packed (a trailing `packed`; n a power of two with 4 <= n <= N/4, two groups or more in each slot plan).  EvalMod is slot-wise, and with n <= N/4 the
// ciphertext has room for the real and the imaginary parts side by side on period 2n: what "would halve EvalMod" with "a different last CoeffToSlot
// factor".  Both slot plans are built packed (slot_transform.h "Packed"):
//   4'. coeff_to_slot's last group uses the table [G; -i G] on 2n rows and returns P = v + conj(v) = [2 c1 s1 s Re; 2 c1 s1 s Im]: the one complex_conjugate
//       that split_real_imag spent, before the group's rescale.  5'. the same relabel, factor 2 and c1 = q_w / (2 K s1 s); the (-1)^j sign of the level-free i
//       is not used.  6'. ONE eval_mod operand: half the products and relinearizations of steps 6, 7.  There is no join.
//   8'. slot_to_coeff's first group uses [F; i F] on 2n rows, V = [F a; i F b], and adds rot_n(V): F (a + i b) on period n, one rotation by n before the
//       group's rescale.  The remaining groups are the n-slot ones.
// No mask product, no extra level: levels() is the unpacked sparse plan's, key_switches() is its count + 1 (the rotation by n), rotation_steps() has the
// packed groups' steps mod 2n and n.  Evaluator::bootstrap runs it with and without the encapsulation: ModRaise, (to_dense), SubSum to n, 4' .. 8', scale D.
// Refused: n outside [4, N/4], a slot plan with a single group.
//
// Sparse-secret encapsulation (Bossuat, Troncoso-Pastoriza, Hubaux 2022).  The evaluation secret s stays as it is; an ephemeral secret s' of small Hamming
// weight is used around ModRaise only, where the modulus is q0 P (one data prime and the special prime).  Evaluator::bootstrap with SparseEncapsulationKeys:
//   1. mod_switch_to the last level;  1a. apply_keyswitching with to_sparse (s -> s');  2. mod_raise: t = D m + q0 I with I from s';
//   2a. apply_keyswitching with to_dense (s' -> s) at the top level;  3. onward as above.
// The two key switches add their usual noise where the payload is D m against q0, and t against the whole chain.  K is chosen from the weight of s'.
//   to_dense   s' -> s, KeyGenerator(s).create_keyswitching_key(s'): an ordinary key at the full key level.
//   to_sparse  s -> s', KeyGenerator(s').create_keyswitching_key(s), in the standard KSwitchKeys layout so that apply_keyswitching reads it unchanged, but
//              holding ONLY what a key switch at the last level reads: digit 0, limbs {0, K_key - 1} of both polynomials.  Every other word is zero on the
//              device: an RLWE sample under a weight-32 secret at the full key modulus is not something to publish.  It never holds a seed (a seed would
//              regenerate the dropped rows): the makers' save_seed goes to to_dense only.  Using it above the last level gives a wrong result, not an error.
// Both members serialize as KSwitchKeys; there is no wire format of the pair.
#pragma once
#include "slot_transform.h"

namespace troy {

struct SparseEncapsulationKeys {
    KSwitchKeys to_sparse, to_dense;
    size_t hamming_weight = 0;        // of s', as counted when the keys were made
};

class BootstrapPlan {
public:
    // empty layers_per_group: the slot plans' default grouping.  std::invalid_argument "[BootstrapPlan::BootstrapPlan] ..." for a non-CKKS context, a chain
    // with fewer than levels() + 1 data levels, K, degree or double_angles outside eval_mod's ranges (K positive and finite, degree 1 .. 127, at most 16
    // double angles), a message or weight scale that is not positive or not finite, q0 / message_scale < 2, an n that is not a power of two in [2, N/2], a sub_sum_radix that is
    // neither 0 (the default, 4) nor a power of two >= 2, a packed plan with n outside [4, N/4]; the slot plans' own refusals pass through.
    BootstrapPlan(HeContextPointer context, const CKKSEncoder& encoder, double message_scale, double half_width, size_t degree, size_t double_angles,
                  std::vector<size_t> coeff_to_slot_layers = {}, std::vector<size_t> slot_to_coeff_layers = {}, double weight_scale = 1099511627776.0,
                  MemoryPoolHandle pool = MemoryPool::GlobalPool(), size_t n = 0, size_t sub_sum_radix = 0, bool packed = false);
    BootstrapPlan(const BootstrapPlan&) = delete;
    BootstrapPlan& operator=(const BootstrapPlan&) = delete;

    // the rule of thumb of the Conditions above for a secret of Hamming weight h: 1 + 6.5 sqrt((h + 1) / 12).  The plan takes K as given; round up as you like.
    static double half_width_for(size_t hamming_weight);

    double message_scale() const { return message_scale_; }
    double half_width() const { return half_width_; }
    size_t degree() const { return degree_; }
    size_t double_angles() const { return double_angles_; }
    size_t eval_mod_depth() const { return eval_mod_depth_; }
    size_t levels() const { return coeff_to_slot_->levels() + eval_mod_depth_ + slot_to_coeff_->levels(); }
    const ParmsID& output_parms_id() const { return output_parms_id_; }
    double output_scale() const { return message_scale_; }
    const std::vector<int>& rotation_steps() const { return rotation_steps_; }       // both plans' steps and 0, the conjugation; sorted
    // a packed plan has no split_real_imag: its conjugation and the rotation by n are counted by the slot plans
    size_t key_switches() const { return sub_sum_key_switches_ + coeff_to_slot_->rotations() + (packed() ? 0 : 1) + slot_to_coeff_->rotations(); }
    bool packed() const { return coeff_to_slot_->packed(); }                          // real and imaginary parts in one EvalMod operand ("Packed", above)
    size_t n() const { return coeff_to_slot_->n(); }                                  // message slots; slot_count() / n() copies fill the ciphertext
    size_t slot_count() const { return coeff_to_slot_->slot_count(); }
    size_t sub_sum_radix() const { return sub_sum_radix_; }                           // as resolved: never 0
    size_t sub_sum_key_switches() const { return sub_sum_key_switches_; }             // 0 when n() == slot_count()
    double sub_sum_factor() const { return static_cast<double>(slot_count() / n()); } // s, divided out inside c1
    const CoeffToSlotPlan& coeff_to_slot_plan() const { return *coeff_to_slot_; }
    const SlotToCoeffPlan& slot_to_coeff_plan() const { return *slot_to_coeff_; }
    double q0() const { return q0_; }
    double coeff_to_slot_constant() const { return coeff_to_slot_->constant(); }     // c1 (with the 1 / s of a sparse plan)
    double slot_to_coeff_constant() const { return slot_to_coeff_->constant(); }     // c2

private:
    double message_scale_, half_width_, q0_ = 0.0;
    size_t degree_, double_angles_, eval_mod_depth_ = 0, sub_sum_radix_ = 0, sub_sum_key_switches_ = 0;
    ParmsID output_parms_id_;
    std::unique_ptr<CoeffToSlotPlan> coeff_to_slot_;
    std::unique_ptr<SlotToCoeffPlan> slot_to_coeff_;
    std::vector<int> rotation_steps_;
};

}  // namespace troy
