// linear_transform.h -- troy::LinearTransform, an ADDITION to the reference's interface: a complex n x n matrix as the weights of a baby-step/giant-step
// (BSGS) product on CKKS slots, the building block of an encrypted matrix-vector product, a convolution layer or the CoeffToSlot / SlotToCoeff steps of a
// bootstrap.  The matrix is given by its diagonals, diag_k[i] = M[i][(i + k) mod n] for k in [0, n), or dense and row-major.  With the project's
// rotation convention rot_s(x)[i] = x[(i + s) mod n],
//     M x = SUM_k diag_k (.) rot_k(x) = SUM_G rot_G( SUM_B w[G][B] (.) rot_B(x) ),   w[G][B][i] = diag_{G+B}[(i - G) mod n]:
// the weight of (G, B) is diagonal G + B rotated back by the giant step (shift s = G).
//
// The split is deterministic.  n1 = baby_count, or the smallest power of two >= sqrt(n) when that is 0.  For the present diagonals k: the baby steps are the
// distinct k mod n1, the giant steps the distinct k - k mod n1, both ascending; weights[g][b] is null where giant_steps[g] + baby_steps[b] is not a present
// diagonal.  rotation_steps() are the non-zero baby and giant steps, sorted, without repeats: what KeyGenerator::create_galois_keys_from_steps needs.
//
// Encoding.  The source (the diagonals, or the dense matrix as it is) is uploaded once and every present (giant, baby) pair is encoded by ONE call of the
// device encoder (CKKSEncoder::encode_diagonals_new, troyn_ckks_encode_diagonals): diagonal and shift are selected while the encoder's first FFT pass loads
// its points, so the rotated diagonals never exist in memory.  The weights are at the key level in NTT form, as rotate_bsgs_sum requires, with the given
// scale.  n < slot_count is the sparsely packed case: n must divide the slot count, a diagonal repeats slot_count / n times across the slots, and the
// operand is expected to repeat with period n as well.
//
// Evaluation: Evaluator::linear_transform (rotate_bsgs_sum_double_hoisted) and linear_transform_single_hoisted (rotate_bsgs_sum), troy.h.  `parms_id` is
// the level of the operand the transform will be applied to; the Evaluator refuses another.  The result's scale is operand scale * scale; no rescale.
#pragma once
#include <map>

#include "troy.h"

namespace troy {

class LinearTransform {
public:
    typedef std::vector<const Plaintext*> WeightRow;
    typedef std::map<size_t, std::vector<std::complex<double>>> Diagonals;
    // throws std::invalid_argument "[LinearTransform::LinearTransform] ..." for a non-CKKS context, n not a power of two dividing the slot count, an
    // unknown parms_id, a baby_count that is not a power of two of at most n, no diagonal, a diagonal index >= n or a diagonal / matrix of the wrong length
    LinearTransform(HeContextPointer context, const CKKSEncoder& encoder, size_t n, const ParmsID& parms_id, double scale, const Diagonals& diagonals,
                    size_t baby_count = 0, MemoryPoolHandle pool = MemoryPool::GlobalPool());
    // the dense matrix, row-major [n][n]: every diagonal is present; the device reads the matrix itself
    LinearTransform(HeContextPointer context, const CKKSEncoder& encoder, size_t n, const ParmsID& parms_id, double scale, const std::vector<std::complex<double>>& matrix,
                    size_t baby_count = 0, MemoryPoolHandle pool = MemoryPool::GlobalPool());
    LinearTransform(const LinearTransform&) = delete;               // the weight rows point into weights_
    LinearTransform& operator=(const LinearTransform&) = delete;

    size_t n() const { return n_; }
    size_t baby_count() const { return n1_; }
    const ParmsID& parms_id() const { return parms_id_; }
    double scale() const { return scale_; }
    const std::vector<int>& baby_steps() const { return baby_steps_; }
    const std::vector<int>& giant_steps() const { return giant_steps_; }
    const std::vector<WeightRow>& weights() const { return rows_; }
    const std::vector<int>& rotation_steps() const { return rotation_steps_; }

private:
    friend class SlotTransformPlan;     // slot_transform.h
    // the diagonals `present` (ascending) as a table [present.size()][n] of double pairs that is already in device memory (CKKSEncoder::dft_factor_diagonals):
    // the split and the weights of the constructors above, nothing but the (diagonal, shift) pairs uploaded
    struct DeviceTable { const double* diagonals; };
    LinearTransform(HeContextPointer context, const CKKSEncoder& encoder, size_t n, const ParmsID& parms_id, double scale, const std::vector<size_t>& present,
                    DeviceTable table, size_t baby_count, MemoryPoolHandle pool);
    void build(HeContextPointer context, const CKKSEncoder& encoder, const std::vector<size_t>& present, const std::complex<double>* source, bool matrix,
               MemoryPoolHandle pool, const double* device_source = nullptr);
    size_t n_, n1_;
    ParmsID parms_id_;
    double scale_;
    std::vector<int> baby_steps_, giant_steps_, rotation_steps_;
    std::vector<Plaintext> weights_;
    std::vector<WeightRow> rows_;
};

}  // namespace troy
