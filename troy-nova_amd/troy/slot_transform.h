// slot_transform.h -- troy::CoeffToSlotPlan and troy::SlotToCoeffPlan, ADDITIONS to the reference's interface: the two linear steps of a CKKS bootstrap
// (ModRaise -> CoeffToSlot -> EvalMod -> SlotToCoeff) on fully packed slots, as a factored special DFT whose factors are written (troyn_ckks_dft_factor_diagonals)
// and encoded (troyn_ckks_encode_diagonals) on the device.  Sparse packing (n < slot_count slots, below) takes the same plans with log2 n layers, and with
// n <= slot_count / 2 a packed plan keeps both halves of the slots in one ciphertext ("Packed", below).
//
// The slot order.  The library keeps the reference's slot order, Galois generator 3, and 3 = -1 (mod 4).  With N the ring degree, n = N/2, m = log2 n,
// zeta = exp(2 pi i / 2N), t the N real coefficients and w_k = t_k + i t_{k+n}: slot j is z_j = t(zeta^(3^j)) and (zeta^(3^j))^n = i^(3^j) is +i for even j
// and -i for odd j, so odd slots see conj(w) and w -> z is only R-linear.  With zh_j = z_j (j even) / conj(z_j) (j odd),
//     zh_j = SUM_k w_k zeta^(e_j k),  e_j = (-3)^j mod 2N,   and   zh = L_{m-1} ... L_0 BR w
// is an ordinary special FFT on the rotation group (-3)^j (-3 = 5 mod 8: its powers are the residues 1 mod 4), BR the bit reversal on m bits.  Layer b has
// the three diagonals {0, +-2^b}; a group of r consecutive layers from `first` has the multiples of 2^first up to +-(2^r - 1) of them, 2^(r+1) - 1
// diagonals (2^r for the group that holds the top layer), every entry one product of r butterfly coefficients (include/troyn.h, "Factors of the special DFT").
//
// The conjugation costs no level.  E and O the even-slot and odd-slot masks, zh = E z + O conj(z):
//     CoeffToSlot   BR w = (L_0^-1 ...) [ (G E) z + (G O) conj(z) ]      G the FIRST-applied group (the top layers, inverse), its COLUMNS masked
//     SlotToCoeff   z = (E G') y + (O conj(G')) conj(y)                  G' the LAST-applied group (the top layers, forward), its ROWS masked
// one complex_conjugate and one extra BSGS transform at the same level, then an add.  The plans conjugate AFTER the weights, (G O) conj(z) = conj(conj(G O) z)
// and (O conj(G')) conj(y) = conj((O G') y): the twin holds conj(G O) / O G', and the key switch of the conjugation meets the product at scale * weight scale,
// where its noise is negligible, instead of the operand at its own scale.
//
// A plan owns one LinearTransform per group, in the order of application, plus the masked twin of the boundary group.  layers_per_group lists the groups in
// the order of application (CoeffToSlot: from the top layer down; SlotToCoeff: from layer 0 up) and sums to log2 n; empty: near-equal groups of at most 4
// layers, the larger ones first.  Group g works at the g-th level below `parms_id` (the level of the operand): every group is followed by rescale_to_next,
// so the chain needs `groups` levels below the operand's.  Every weight is encoded at `scale`.  The real `constant` is multiplied in as its groups-th root in
// every group (its sign in the first), so that a normalisation such as EvalMod's 1 / (q0 K) costs no level.
//
// baby_count for strided diagonals: the diagonals of a group are multiples of 2^first, and n1 = 2^first: the only baby step is 0 and every diagonal is a
// giant step, nd - 1 rotations per transform.  A giant step rotates the weighted product, at scale * weight scale, where the noise of its key switch is
// negligible; a baby step would rotate the operand at its own scale and add that noise at full size in every group.  With n1 = 2^first * 4 a group of three
// layers would need 6 rotations instead of 14 and measured a 10 times larger slot error at N = 1024.
//
// Slot order of the result: coeff_to_slot leaves constant * BR(w) in the slots, slot i holding w_{bitrev(i)} = t_{bitrev(i)} + i t_{bitrev(i) + n}.  EvalMod is
// slot-wise and slot_to_coeff consumes this order, so no permutation is ever applied.
//
// Sparse packing.  A trailing n (0: the slot count), a power of two with 2 <= n <= slot_count, builds the transform of the sub-ring of degree 2n: with
// s = N/(2n) the message is a polynomial p(Y), Y = X^s, its slots an n-vector repeated s times, w_k = t'_k + i t'_{k+n} on the Y-coefficients t', and
// zh = L_{m'-1} ... L_0 BR w with m' = log2 n, layer b the full ring's layer b (troyn_ckks_dft_factor_diagonals_sparse).  layers_per_group sums to log2 n; the
// group holding layer m' - 1 is the top one; diagonal indices are mod n; the transforms are LinearTransforms on n, whose weights repeat s times across the
// slots.  n is even, so the even / odd masks and the conjugation carry over.  The operand must repeat with period n and be a polynomial in Y: after a
// ModRaise that is what Evaluator::sub_sum (troy.h) restores.  Everything above reads with m' for m and t' for t; n = slot_count is the fully packed plan.
//
// Packed (a trailing `packed`, n a power of two with 4 <= n <= slot_count / 2, at least two groups).  The ciphertext has room for the real and the imaginary
// parts of the n slots side by side on period 2n, so that EvalMod, which is slot-wise, runs once.  A group of layers [first, first + count) with
// first + count <= m' is block diagonal with blocks of at most n rows: on 2n rows it is two identical n x n blocks, no entry crosses row n, and it is never
// the top group (2^(count+1) - 1 diagonals, indices mod 2n).  The packed table (troyn_ckks_dft_factor_diagonals_packed) has that group in rows < n and the
// same words times -i (inverse) / +i (forward) in rows >= n; it takes the place of the group of layers [0, c), which with two groups or more is never the
// boundary group that carries the masks and the twin.
//     CoeffToSlot, last-applied group:   u of period n, v = M1 u = [G u; -i G u], and P = v + conj(v) = [2 Re(G u); 2 Im(G u)] on period 2n: one
//         complex_conjugate and one add before the group's rescale (where split_real_imag spent its conjugation).  coeff_to_slot returns P.
//     SlotToCoeff, first-applied group:  P' = [a; b] real of period 2n, V = F1 P' = [F a; i F b], and V + rot_n(V) = F (a + i b) on period n: one rotation
//         by n slots and one add before the group's rescale, the ONE key switch more than the unpacked pair of plans.  slot_to_coeff takes P'.
// No mask product and no extra level.  rotations() counts the conjugation / the rotation by n; rotation_steps() lists the packed group's steps mod 2n and n.
#pragma once
#include <memory>

#include "linear_transform.h"

namespace troy {

class SlotTransformPlan {
public:
    SlotTransformPlan(const SlotTransformPlan&) = delete;
    SlotTransformPlan& operator=(const SlotTransformPlan&) = delete;

    size_t n() const { return n_; }                                      // the slots of the transform; slot_count() / n() copies fill the ciphertext
    size_t slot_count() const { return slot_count_; }
    const ParmsID& parms_id() const { return parms_ids_.front(); }       // the level of the operand
    double scale() const { return scale_; }
    double constant() const { return constant_; }
    size_t groups() const { return transforms_.size(); }
    size_t levels() const { return transforms_.size(); }                 // one rescale per group
    const std::vector<size_t>& layers_per_group() const { return layers_; }
    size_t first_layer(size_t group) const { return firsts_.at(group); }
    size_t boundary_group() const { return boundary_; }
    bool packed() const { return packed_; }                              // real and imaginary parts side by side on period 2n ("Packed" above)
    size_t packed_group() const { return packed_group_; }                // the group of layers [0, c): the last of CoeffToSlot, the first of SlotToCoeff
    const LinearTransform& transform(size_t group) const { return *transforms_.at(group); }
    const LinearTransform& twin() const { return *twin_; }               // applied to the boundary group's operand; its result is conjugated
    const ParmsID& group_parms_id(size_t group) const { return parms_ids_.at(group); }
    bool needs_conjugate() const { return true; }
    const std::vector<int>& rotation_steps() const { return rotation_steps_; }   // the union over the groups, sorted
    size_t rotations() const { return rotations_; }                     // key switches of one evaluation: non-zero baby and giant steps of every transform + the conjugation

protected:
    // throws std::invalid_argument "[CoeffToSlotPlan::CoeffToSlotPlan] ..." / "[SlotToCoeffPlan::SlotToCoeffPlan] ..." for a non-CKKS context, an unknown
    // parms_id, an n that is not a power of two in [2, slot_count], groups that are empty or do not sum to log2 n, a chain with fewer levels below the operand than groups, a constant that is zero or not finite,
    // a packed plan with n outside [4, slot_count / 2] or a single group
    SlotTransformPlan(bool coeff_to_slot, HeContextPointer context, const CKKSEncoder& encoder, const ParmsID& parms_id, double scale, std::vector<size_t> layers_per_group,
                      double constant, MemoryPoolHandle pool, size_t n, bool packed);

private:
    size_t n_, slot_count_, boundary_ = 0, packed_group_ = 0, rotations_ = 0;
    bool packed_ = false;
    double scale_, constant_;
    std::vector<size_t> layers_, firsts_;
    std::vector<ParmsID> parms_ids_;
    std::vector<std::unique_ptr<LinearTransform>> transforms_;
    std::unique_ptr<LinearTransform> twin_;
    std::vector<int> rotation_steps_;
};

// near-equal groups of at most `at_most` layers, the larger ones first: the plans' default
std::vector<size_t> default_layers_per_group(size_t layers, size_t at_most = 4);

class CoeffToSlotPlan : public SlotTransformPlan {
public:
    CoeffToSlotPlan(HeContextPointer context, const CKKSEncoder& encoder, const ParmsID& parms_id, double scale, std::vector<size_t> layers_per_group = {},
                    double constant = 1.0, MemoryPoolHandle pool = MemoryPool::GlobalPool(), size_t n = 0, bool packed = false)
        : SlotTransformPlan(true, context, encoder, parms_id, scale, std::move(layers_per_group), constant, pool, n, packed) {}
};

class SlotToCoeffPlan : public SlotTransformPlan {
public:
    SlotToCoeffPlan(HeContextPointer context, const CKKSEncoder& encoder, const ParmsID& parms_id, double scale, std::vector<size_t> layers_per_group = {},
                    double constant = 1.0, MemoryPoolHandle pool = MemoryPool::GlobalPool(), size_t n = 0, bool packed = false)
        : SlotTransformPlan(false, context, encoder, parms_id, scale, std::move(layers_per_group), constant, pool, n, packed) {}
};

}  // namespace troy
